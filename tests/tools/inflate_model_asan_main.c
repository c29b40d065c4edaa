/* inflate_model_asan_main.c -- a stand-alone program over ffhip_inflate_model, the host model of k_inflate, to be built with
 * -fsanitize=address,undefined together with ffhip_inflate_model.c and ffhip_inflate.c (plain C, no HIP): the stream in the file named on
 * the command line, every proper prefix and every single-bit flip of it go through the model from an exact-size heap copy into heap
 * buffers of exactly `cap` bytes -- the output's size, one byte less, half of it and none, with and without `partial` -- so that a byte
 * read or written beside them is a sanitizer report: the loads and stores of the body are the kernel's.  Every verdict is held against
 * ffhip_inflate_upto's, and where both accept, the bytes. */
#include "ffpic_hip.h"
#include "ffhip_png_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int run(const uint8_t *data, size_t len, size_t cap, int partial)
{
    uint8_t *z = (uint8_t *)malloc(len ? len : 1); /* exact size: the first byte behind the stream is poisoned */
    uint8_t *a = (uint8_t *)malloc(cap ? cap : 1), *b = (uint8_t *)malloc(cap ? cap : 1);
    if (!z || !a || !b) return 1;
    if (len) memcpy(z, data, len);
    size_t got_a = 0, got_b = 0;
    const int ra = ffhip_inflate_model(z, len, cap ? a : NULL, cap, &got_a, partial);
    const int rb = ffhip_inflate_upto(z, len, cap ? b : NULL, cap, &got_b, partial);
    int bad = ra != rb || (ra != FFHIP_OK && ra != FFHIP_EINVAL);
    if (!bad && ra == FFHIP_OK) bad = got_a != got_b || got_a > cap || memcmp(a, b, got_a) != 0;
    free(z); free(a); free(b);
    return bad;
}

static int run_all(const uint8_t *data, size_t len, size_t out)
{
    const size_t caps[4] = {out, out ? out - 1 : 0, out / 2, 0};
    for (int k = 0; k < 4; k++)
        for (int partial = 0; partial < 2; partial++)
            if (run(data, len, caps[k], partial)) return 1;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s stream.z\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    static uint8_t data[1 << 16], whole[1 << 20];
    const size_t len = fread(data, 1, sizeof(data), f);
    fclose(f);
    size_t out = 0;
    if (ffhip_inflate(data, len, whole, sizeof(whole), &out) != FFHIP_OK) { fprintf(stderr, "the stream itself fails\n"); return 1; }
    long runs = 0;
    if (run_all(data, len, out)) { fprintf(stderr, "the stream itself differs\n"); return 1; }
    for (size_t n = 0; n < len; n++, runs++)
        if (run_all(data, n, out)) { fprintf(stderr, "prefix %zu\n", n); return 1; }
    for (size_t i = 0; i < 8 * len; i++, runs++) {
        data[i >> 3] ^= (uint8_t)(1 << (i & 7));
        const int bad = run_all(data, len, out);
        data[i >> 3] ^= (uint8_t)(1 << (i & 7));
        if (bad) { fprintf(stderr, "byte %zu bit %d\n", i >> 3, (int)(i & 7)); return 1; }
    }
    printf("ok: %ld streams\n", runs);
    return 0;
}
