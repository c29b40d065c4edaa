/* ffhip_jpeg_exif_orientation / ffhip_webp_exif_orientation (ffpic_amd/csrc/ffhip_exif.c) over damaged files, built together with that
 * file with -fsanitize=address,undefined.  Every file named on the command line (a RIFF header says WebP, anything else is taken as JPEG)
 * is truncated to each of its lengths and has every byte of its Exif block (the APP1 segment / the EXIF chunk; the first 256 bytes where
 * none is found) set to each of the 255 other values; every variant is copied into a malloc of exactly its size, so that a read one byte
 * past it is reported.  Each call has to return FFHIP_OK with a value in 1..8.  Exit 0 and no output when all is well. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffpic_hip.h"

typedef int (*reader)(const uint8_t *, size_t, int *);

static int one(reader f, const uint8_t *bytes, size_t len, const char *what, size_t at)
{
    uint8_t *exact = malloc(len ? len : 1); /* (length 0: one byte that must not be read either -- the call gets len 0) */
    if (!exact) return 1;
    memcpy(exact, bytes, len);
    int o = -1;
    const int rc = f(exact, len, &o);
    free(exact);
    if (rc == FFHIP_OK && o >= 1 && o <= 8) return 0;
    fprintf(stderr, "%s at %zu: returned %d, orientation %d\n", what, at, rc, o);
    return 1;
}

/* [*first, *end): the bytes of the file that hold its Exif block */
static void exif_block(const uint8_t *b, size_t len, int webp, size_t *first, size_t *end)
{
    *first = 0;
    *end = len < 256 ? len : 256;
    for (size_t p = webp ? 12 : 2; p + 8 <= len; p++) {
        if (webp ? memcmp(b + p, "EXIF", 4) == 0 : (b[p] == 0xFF && b[p + 1] == 0xE1 && memcmp(b + p + 4, "Exif", 4) == 0)) {
            const size_t size = webp ? 8 + ((size_t)b[p + 4] | (size_t)b[p + 5] << 8 | (size_t)b[p + 6] << 16) : 2 + ((size_t)b[p + 2] << 8 | b[p + 3]);
            *first = p;
            *end = p + size < len ? p + size : len;
            return;
        }
    }
}

int main(int argc, char **argv)
{
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(fp, 0, SEEK_END);
        const size_t len = (size_t)ftell(fp);
        fseek(fp, 0, SEEK_SET);
        uint8_t *bytes = malloc(len ? len : 1);
        if (!bytes || fread(bytes, 1, len, fp) != len) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(fp);
        const int webp = len >= 4 && memcmp(bytes, "RIFF", 4) == 0;
        const reader f = webp ? ffhip_webp_exif_orientation : ffhip_jpeg_exif_orientation;
        for (size_t cut = 0; cut <= len; cut++) bad += one(f, bytes, cut, "truncated", cut);
        size_t first, end;
        exif_block(bytes, len, webp, &first, &end);
        for (size_t at = first; at < end; at++) {
            const uint8_t keep = bytes[at];
            for (int v = 0; v < 256; v++) {
                if (v == keep) continue;
                bytes[at] = (uint8_t)v;
                bad += one(f, bytes, len, "mutated", at);
            }
            bytes[at] = keep;
        }
        /* the contract's other half */
        int o = 5;
        if (f(NULL, len, &o) != FFHIP_EINVAL || f(bytes, len, NULL) != FFHIP_EINVAL) { fprintf(stderr, "NULL arguments are not refused\n"); bad++; }
        free(bytes);
    }
    return bad ? 1 : 0;
}
