/* vp8l_enc_asan_main.c -- the host lossless WebP encoder (ffhip_vp8l_encode_picture, with ffhip_vp8l_encode_residual) under
 * -fsanitize=address,undefined: a few hundred pictures from a fixed generator, every input in a heap buffer of exactly its size, every
 * output in a heap buffer of exactly cap bytes -- the bound, the exact size and one byte less.  A stand-alone program
 * (tests/test_vp8l_encode_capi.py builds and runs it); prints "ok: <pictures> pictures". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffpic_hip.h"

static uint32_t state = 4321u;
static uint32_t rnd(void) { state = state * 1664525u + 1013904223u; return state >> 8; }

static void fill(uint8_t *p, size_t n, int kind)
{
    for (size_t i = 0; i < n; i++) {
        switch (kind % 5) {
        case 0: p[i] = (uint8_t)rnd(); break;
        case 1: p[i] = (uint8_t)(rnd() & 3); break;
        case 2: p[i] = 77; break;
        case 3: p[i] = (uint8_t)(i % 7); break;
        default: p[i] = (uint8_t)(i / 3); break;
        }
    }
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int one_picture(int w, int h, int c, int flags, int kind)
{
    const size_t bytes = (size_t)w * h * c;
    uint8_t *px = (uint8_t *)malloc(bytes);
    if (!px) FAIL("no memory");
    fill(px, bytes, kind);
    ffhip_vp8l_source s;
    memset(&s, 0, sizeof(s));
    /* every second picture bottom-up: the first byte read is the buffer's last row */
    const int flip = kind & 1;
    s.pixels = flip ? px + (size_t)(h - 1) * w * c : px;
    s.row_stride = flip ? -(int64_t)w * c : (int64_t)w * c;
    s.pixel_stride = c;
    for (int k = 0; k < c; k++) s.chan[k] = k;
    s.channels = c; s.width = w; s.height = h;
    const int tile = 1 << FFHIP_VP8L_ENC_TILE_BITS;
    const size_t tiles = (size_t)((w + tile - 1) / tile) * (size_t)((h + tile - 1) / tile), bound = ffhip_vp8l_encode_bound(w, h);
    uint32_t *res = (uint32_t *)malloc((size_t)w * h * 4);
    uint8_t *modes = (uint8_t *)malloc(tiles), *full = (uint8_t *)malloc(bound);
    size_t n = 0, m = 0;
    if (!res || !modes || !full) FAIL("no memory");
    if (ffhip_vp8l_encode_residual(&s, flags, res, modes) != FFHIP_OK) FAIL("residual %dx%dx%d", w, h, c);
    if (ffhip_vp8l_encode_picture(&s, flags, full, bound, &n) != FFHIP_OK || n > bound || n < 26 || (n & 1)) FAIL("encode %dx%dx%d", w, h, c);
    uint8_t *exact = (uint8_t *)malloc(n), *shorter = (uint8_t *)malloc(n - 1);
    if (!exact || !shorter) FAIL("no memory");
    if (ffhip_vp8l_encode_picture(&s, flags, exact, n, &m) != FFHIP_OK || m != n || memcmp(exact, full, n)) FAIL("exact cap %dx%dx%d", w, h, c);
    if (ffhip_vp8l_encode_picture(&s, flags, shorter, n - 1, &m) != FFHIP_EVP8L_NOSPACE || m != n || memcmp(shorter, full, n - 1)) FAIL("short cap %dx%dx%d", w, h, c);
    free(px); free(res); free(modes); free(full); free(exact); free(shorter);
    return 0;
}

int main(void)
{
    int pictures = 0;
    for (int k = 0; k < 300; k++, pictures++) {
        const int w = 1 + (int)(rnd() % (k % 10 == 0 ? 1200 : 40)), h = 1 + (int)(rnd() % (k % 7 == 0 ? 60 : 12));
        if (one_picture(w, h, 1 + k % 4, k % 4, k)) return 1;
    }
    if (one_picture(64, 65, 4, 3, 1) || one_picture(100, 83, 3, 3, 2)) return 1; /* two and three chunks */
    pictures += 2;
    printf("ok: %d pictures\n", pictures);
    return 0;
}
