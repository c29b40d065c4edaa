/* png_host_asan_main.c -- a stand-alone program over the host side of the PNG calls, to be built with -fsanitize=address,undefined together
 * with ffhip_inflate.c and ffhip_png.c (plain C, no HIP): for every file named on the command line, every prefix and every single-byte
 * change of it goes through ffhip_png_probe, ffhip_png_picture and -- its IDAT payload -- ffhip_inflate, from an exact-size heap copy into
 * exact-size heap buffers, so that a byte read or written beside them is a sanitizer report.  Results are not compared here (the tests do
 * that); a good file must decode, and its changes must return FFHIP_OK or FFHIP_EINVAL. */
#include "ffpic_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int run(const uint8_t *data, size_t len, int must_decode)
{
    uint8_t *file = (uint8_t *)malloc(len ? len : 1); /* exact size: the first byte behind the file is poisoned */
    if (!file) return 1;
    memcpy(file, data, len);
    ffhip_png_info info;
    int rc = ffhip_png_probe(file, len, &info);
    if (rc != FFHIP_OK && rc != FFHIP_EINVAL) { free(file); return 1; }
    if (rc == FFHIP_OK) {
        const int64_t pitch = 4LL * info.width;
        uint8_t *bgra = (uint8_t *)malloc((size_t)pitch * (size_t)info.height);
        if (!bgra) { free(file); return 1; }
        rc = ffhip_png_picture(file, len, bgra, pitch);
        free(bgra);
        if (rc != FFHIP_OK && rc != FFHIP_EINVAL) { free(file); return 1; }
    }
    if (must_decode && rc != FFHIP_OK) { free(file); return 1; }
    /* the first IDAT's payload as a zlib stream of its own, into a buffer of exactly the filtered size and into one a byte short */
    for (size_t at = 8; rc == FFHIP_OK && at + 12 <= len;) {
        const size_t n = (size_t)file[at] << 24 | (size_t)file[at + 1] << 16 | (size_t)file[at + 2] << 8 | file[at + 3];
        if (n > len - at - 12) break;
        if (memcmp(file + at + 4, "IDAT", 4) == 0) {
            uint8_t *z = (uint8_t *)malloc(n ? n : 1);
            const size_t cap = (size_t)info.filtered_bytes;
            uint8_t *out = (uint8_t *)malloc(cap), *tight = (uint8_t *)malloc(cap - 1 ? cap - 1 : 1);
            size_t got = 0;
            if (!z || !out || !tight) return 1;
            memcpy(z, file + at + 8, n);
            const int a = ffhip_inflate(z, n, out, cap, &got), b = ffhip_inflate(z, n, tight, cap - 1, &got);
            free(z); free(out); free(tight);
            if ((a != FFHIP_OK && a != FFHIP_EINVAL) || (b != FFHIP_OK && b != FFHIP_EINVAL)) { free(file); return 1; }
            break;
        }
        at += n + 12;
    }
    free(file);
    return 0;
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
