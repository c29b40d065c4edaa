/* webp_alpha_host_asan_main.c -- a stand-alone program over the host side of FFHIP_WEBP_ALPHA, to be built with
 * -fsanitize=address,undefined together with ffhip_webp_alpha.c and ffhip_vp8l.c (plain C, no HIP): for every file named on
 * the command line, every prefix and two single-bit changes of every byte go through ffhip_webp_alpha_probe and ffhip_webp_alpha_plane,
 * from an exact-size heap copy into an exact-size heap buffer, so that a byte read or written beside them is a sanitizer report.  Results
 * are not compared here (the tests do that); a good file must decode, and its changes must return a code the calls are documented to.
 * The plane's size comes from the library's own chunk walk (ffhip_webp_alpha_find), which runs under the sanitizers with the rest. */
#include "ffhip_webp_alpha_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int known(int rc)
{
    return rc == FFHIP_OK || rc == FFHIP_EINVAL || rc == FFHIP_EWEBP_ANIMATION || rc == FFHIP_EWEBP_LOSSLESS || rc == FFHIP_EWEBP_INTER_FRAME;
}

static int run(const uint8_t *data, size_t len, int must_decode)
{
    uint8_t *file = (uint8_t *)malloc(len ? len : 1); /* exact size: the first byte behind the file is poisoned */
    if (!file) return 1;
    memcpy(file, data, len);
    int has = 0, compression = 0, filter = 0, pre = 0;
    int rc = ffhip_webp_alpha_probe(file, len, &has, &compression, &filter, &pre);
    if (!known(rc)) { free(file); return 1; }
    if (rc == FFHIP_OK && has) {
        ffhip_webp_alpha_head head;
        if (ffhip_webp_alpha_find(file, len, &head) != FFHIP_OK || !head.has_alpha) { free(file); return 1; }
        uint8_t *plane = (uint8_t *)malloc((size_t)head.width * head.height); /* at most 2^28 */
        if (!plane) { free(file); return 1; }
        rc = ffhip_webp_alpha_plane(file, len, plane, head.width);
        free(plane);
        if (!known(rc)) { free(file); return 1; }
    } else if (must_decode) {
        rc = FFHIP_EINVAL;
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
