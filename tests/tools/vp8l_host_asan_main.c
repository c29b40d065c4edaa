/* vp8l_host_asan_main.c -- a stand-alone program over the host side of the lossless WebP calls, to be built with
 * -fsanitize=address,undefined together with ffhip_vp8l.c (plain C, no HIP): for every file named on the command line, every prefix and
 * every single-byte change of it goes through ffhip_vp8l_probe, ffhip_vp8l_read_info and ffhip_vp8l_picture, from an exact-size heap copy
 * into an exact-size heap buffer, so that a byte read or written beside them is a sanitizer report.  Results are not compared here (the
 * tests do that); a good file must decode, and its changes must return FFHIP_OK, FFHIP_EINVAL or FFHIP_EWEBP_ANIMATION. */
#include "ffpic_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int known(int rc) { return rc == FFHIP_OK || rc == FFHIP_EINVAL || rc == FFHIP_EWEBP_ANIMATION; }

static int run(const uint8_t *data, size_t len, int must_decode)
{
    uint8_t *file = (uint8_t *)malloc(len ? len : 1); /* exact size: the first byte behind the file is poisoned */
    if (!file) return 1;
    memcpy(file, data, len);
    int w = 0, h = 0, alpha = 0;
    ffhip_vp8l_info info;
    int rc = ffhip_vp8l_probe(file, len, &w, &h, &alpha);
    if (!known(rc) || !known(ffhip_vp8l_read_info(file, len, &info))) { free(file); return 1; }
    if (rc == FFHIP_OK && (long long)w * h <= 1 << 22) { /* a changed size field: up to 16 MiB of picture is tried */
        const int64_t pitch = 4LL * w;
        uint8_t *bgra = (uint8_t *)malloc((size_t)pitch * (size_t)h);
        if (!bgra) { free(file); return 1; }
        rc = ffhip_vp8l_picture(file, len, bgra, pitch);
        free(bgra);
        if (!known(rc)) { free(file); return 1; }
    }
    free(file);
    return must_decode && rc != FFHIP_OK;
}

int main(int argc, char **argv)
{
    long runs = 0;
    for (int k = 1; k < argc; k++) {
        FILE *f = fopen(argv[k], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        static uint8_t data[1 << 16];
        const size_t len = fread(data, 1, sizeof(data), f);
        fclose(f);
        if (run(data, len, 1)) { fprintf(stderr, "%s: the file itself fails\n", argv[k]); return 1; }
        for (size_t n = 0; n < len; n++, runs++)
            if (run(data, n, 0)) { fprintf(stderr, "%s: prefix %zu\n", argv[k], n); return 1; }
        for (size_t i = 0; i < len; i++) {
            for (int bit = 0; bit < 8; bit += 7, runs++) { /* the lowest and the highest bit of every byte */
                data[i] ^= (uint8_t)(1 << bit);
                const int bad = run(data, len, 0);
                data[i] ^= (uint8_t)(1 << bit);
                if (bad) { fprintf(stderr, "%s: byte %zu bit %d\n", argv[k], i, bit); return 1; }
            }
        }
    }
    printf("ok: %ld runs\n", runs);
    return 0;
}
