/* png_enc_asan_main.c -- the two host encoders (ffhip_deflate, ffhip_png_encode_picture, with ffhip_png_filter_picture) under
 * -fsanitize=address,undefined: a few hundred streams and pictures from a fixed generator, every input in a heap buffer of exactly its
 * size, every output in a heap buffer of exactly cap bytes -- the bound, the exact size and one byte less.  A stand-alone program
 * (tests/test_png_encode_capi.py builds and runs it); prints "ok: <streams> streams, <pictures> pictures". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffpic_hip.h"

static uint32_t state = 12345u;
static uint32_t rnd(void) { state = state * 1664525u + 1013904223u; return state >> 8; }

static void fill(uint8_t *p, size_t n, int kind)
{
    for (size_t i = 0; i < n; i++) {
        switch (kind % 5) {
        case 0: p[i] = (uint8_t)rnd(); break;
        case 1: p[i] = (uint8_t)(rnd() & 3); break;
        case 2: p[i] = 0; break;
        case 3: p[i] = (uint8_t)(i % 7); break;
        default: p[i] = (uint8_t)(i / 3); break;
        }
    }
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int one_stream(size_t len, int kind)
{
    uint8_t *src = (uint8_t *)malloc(len ? len : 1);
    if (!src) FAIL("no memory");
    fill(src, len, kind);
    const size_t bound = ffhip_deflate_bound(len);
    uint8_t *full = (uint8_t *)malloc(bound);
    size_t n = 0, m = 0;
    if (!full || ffhip_deflate(len ? src : NULL, len, full, bound, &n) != FFHIP_OK || n > bound) FAIL("deflate of %zu bytes (kind %d)", len, kind);
    uint8_t *exact = (uint8_t *)malloc(n), *shorter = (uint8_t *)malloc(n - 1);
    if (!exact || !shorter) FAIL("no memory");
    if (ffhip_deflate(len ? src : NULL, len, exact, n, &m) != FFHIP_OK || m != n || memcmp(exact, full, n)) FAIL("exact cap, %zu bytes", len);
    if (ffhip_deflate(len ? src : NULL, len, shorter, n - 1, &m) != FFHIP_EDEFLATE_NOSPACE || m != n || memcmp(shorter, full, n - 1)) FAIL("short cap, %zu bytes", len);
    free(src); free(full); free(exact); free(shorter);
    return 0;
}

static int one_picture(int w, int h, int c, int filter, int kind)
{
    const size_t bytes = (size_t)w * h * c;
    uint8_t *px = (uint8_t *)malloc(bytes);
    if (!px) FAIL("no memory");
    fill(px, bytes, kind);
    ffhip_png_source s;
    memset(&s, 0, sizeof(s));
    /* every second picture bottom-up: the first byte read is the buffer's last row */
    const int flip = kind & 1;
    s.pixels = flip ? px + (size_t)(h - 1) * w * c : px;
    s.row_stride = flip ? -(int64_t)w * c : (int64_t)w * c;
    s.pixel_stride = c;
    for (int k = 0; k < c; k++) s.chan[k] = k;
    s.channels = c; s.width = w; s.height = h;
    const size_t fsize = ffhip_png_filtered_size(w, h, c), bound = ffhip_png_encode_bound(w, h, c);
    uint8_t *filt = (uint8_t *)malloc(fsize), *full = (uint8_t *)malloc(bound);
    size_t n = 0, m = 0;
    if (!filt || !full) FAIL("no memory");
    if (ffhip_png_filter_picture(&s, filter, filt, fsize, &m) != FFHIP_OK || m != fsize) FAIL("filter %dx%dx%d", w, h, c);
    if (ffhip_png_encode_picture(&s, filter, full, bound, &n) != FFHIP_OK || n > bound) FAIL("encode %dx%dx%d", w, h, c);
    uint8_t *exact = (uint8_t *)malloc(n), *shorter = (uint8_t *)malloc(n - 1);
    if (!exact || !shorter) FAIL("no memory");
    if (ffhip_png_encode_picture(&s, filter, exact, n, &m) != FFHIP_OK || m != n || memcmp(exact, full, n)) FAIL("exact cap %dx%dx%d", w, h, c);
    if (ffhip_png_encode_picture(&s, filter, shorter, n - 1, &m) != FFHIP_EPNG_NOSPACE || m != n || memcmp(shorter, full, n - 1)) FAIL("short cap %dx%dx%d", w, h, c);
    free(px); free(filt); free(full); free(exact); free(shorter);
    return 0;
}

int main(void)
{
    static const size_t lens[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 258, 259, 1000, FFHIP_DEFLATE_CHUNK - 1, FFHIP_DEFLATE_CHUNK, FFHIP_DEFLATE_CHUNK + 1,
                                  2 * FFHIP_DEFLATE_CHUNK + 3};
    int streams = 0, pictures = 0;
    for (int kind = 0; kind < 5; kind++)
        for (size_t k = 0; k < sizeof(lens) / sizeof(lens[0]); k++, streams++)
            if (one_stream(lens[k], kind)) return 1;
    for (int k = 0; k < 120; k++, streams++)
        if (one_stream(rnd() % 700, k)) return 1;
    for (int k = 0; k < 300; k++, pictures++) {
        const int w = 1 + (int)(rnd() % (k % 10 == 0 ? 1200 : 40)), h = 1 + (int)(rnd() % (k % 7 == 0 ? 60 : 12));
        if (one_picture(w, h, 1 + k % 4, k % 6, k)) return 1;
    }
    if (one_picture(910, 9, 4, FFHIP_PNG_FILTER_ADAPTIVE, 1)) return 1; /* 2 x CHUNK + 1 filtered bytes */
    pictures++;
    printf("ok: %d streams, %d pictures\n", streams, pictures);
    return 0;
}
