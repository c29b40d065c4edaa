// check_vp8_enc.cpp -- the host side of the lossy WebP encoder (ffhip_vp8_enc.c, ffhip_vp8_enc_body.h) as a program of its own, to be
// built with -fsanitize=address,undefined (tests/test_vp8_encode_capi.py does): small pictures of every size class in heap buffers of
// exactly their size, RGB, grey and a strided BGR form, at four qualities; the file into a buffer of exactly the bound, then every cap from
// 0 to the file's length into a buffer of exactly cap bytes.  Prints "ok <files>" and exits 0, or says what failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffpic_hip.h"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static uint32_t state = 12345;
static int next_byte() { state = state * 1664525u + 1013904223u; return (int)(state >> 24); }

int main()
{
    static const int sizes[][2] = {{1, 1}, {16, 16}, {17, 16}, {33, 47}, {16, 130}, {48, 24}};
    static const int qualities[] = {0, 30, 75, 100};
    int files = 0;
    for (const auto &wh : sizes)
        for (int form = 0; form < 3; form++) { /* RGB, grey, BGR with a padded pitch */
            const int w = wh[0], h = wh[1], ch = form == 1 ? 1 : 3;
            const size_t pitch = (size_t)w * ch + (form == 2 ? 5 : 0), bytes = pitch * (size_t)(h - 1) + (size_t)w * ch;
            uint8_t *px = (uint8_t *)std::malloc(bytes);
            for (size_t k = 0; k < bytes; k++) px[k] = (uint8_t)((form ? 128 : 8 * (int)(k % 29)) + next_byte() % 24);
            ffhip_jpeg_source s;
            std::memset(&s, 0, sizeof(s));
            s.pixels = px; s.row_stride = (int64_t)pitch; s.pixel_stride = ch; s.channels = ch; s.width = w; s.height = h;
            if (ch == 3) { s.chan[0] = form == 2 ? 2 : 0; s.chan[1] = 1; s.chan[2] = form == 2 ? 0 : 2; }
            const int cols = (w + 15) / 16, rows = (h + 15) / 16;
            const size_t n = (size_t)cols * rows;
            std::vector<uint8_t> y(n * 256), u(n * 64), v(n * 64), ym(n), uvm(n);
            std::vector<int16_t> levels(n * 400);
            if (ffhip_vp8_encode_planes(&s, y.data(), u.data(), v.data()) != FFHIP_OK) FAIL("planes %dx%d", w, h);
            for (int quality : qualities) {
                if (ffhip_vp8_encode_mbs(&s, quality, ym.data(), uvm.data(), levels.data(), y.data(), u.data(), v.data()) != FFHIP_OK) FAIL("mbs %dx%d", w, h);
                const size_t bound = ffhip_vp8_encode_bound(w, h);
                uint8_t *full = (uint8_t *)std::malloc(bound);
                size_t len = 0;
                if (ffhip_vp8_encode_picture(&s, quality, quality == 30 ? -1 : quality % 64, full, bound, &len) != FFHIP_OK || len > bound || len < 30)
                    FAIL("picture %dx%d form %d quality %d", w, h, form, quality);
                const size_t step = len > 600 ? 37 : 1; /* the longer files by steps, their last caps all the same */
                for (size_t cap = 0; cap <= len; cap += (cap + step + 40 > len ? 1 : step)) {
                    uint8_t *out = cap ? (uint8_t *)std::malloc(cap) : nullptr;
                    size_t m = 0;
                    const int rc = ffhip_vp8_encode_picture(&s, quality, quality == 30 ? -1 : quality % 64, out, cap, &m);
                    if (rc != (cap < len ? FFHIP_EVP8_NOSPACE : FFHIP_OK) || m != len || (cap && std::memcmp(out, full, cap)))
                        FAIL("cap %zu of %zu: %dx%d form %d quality %d rc %d", cap, len, w, h, form, quality, rc);
                    std::free(out);
                }
                std::free(full);
                files++;
            }
            std::free(px);
        }
    std::printf("ok %d\n", files);
    return 0;
}
