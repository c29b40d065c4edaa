/*
 * tests/tools/fuzz_progressive.c -- robustness driver for the progressive JPEG front end (ffpic_amd/csrc/ffhip_jpeg_progressive.c with
 * the body it shares with the kernel, ffhip_jpeg_prog_body.h), built with -fsanitize=address,undefined by tests/test_jpeg_progressive.py.
 * A stand-alone program: every truncation of the given file, then seeded byte mutations of it, through ffhip_jpeg_probe_any /
 * ffhip_jpeg_progressive_decode.  The file bytes and the planes are malloc'd at their exact size, so a read behind the file or a store
 * outside the planes aborts the process; every run must end in FFHIP_OK or FFHIP_EINVAL.  No GPU involved.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffpic_hip.h"

static unsigned long long s_rng = 88172645463325252ULL;
static unsigned rnd(void) { s_rng ^= s_rng << 13; s_rng ^= s_rng >> 7; s_rng ^= s_rng << 17; return (unsigned)(s_rng >> 11); }

static int ok, rejected;
static ffhip_jpeg_geom g0;

/* one run on a copy of exactly len bytes */
static int run(const unsigned char *bytes, size_t len, int k_max)
{
    unsigned char *file = malloc(len ? len : 1);
    if (!file) return 2;
    memcpy(file, bytes, len);
    const size_t mcus = (size_t)g0.mcu_cols * g0.mcu_rows;
    int16_t *cy = malloc(mcus * g0.h * g0.v * 128), *cu = malloc(mcus * 128), *cv = malloc(mcus * 128);
    uint16_t *q = malloc(512);
    ffhip_jpeg_geom g;
    int w, h, pg;
    int rc = ffhip_jpeg_probe_any(file, len, &g, &w, &h, &pg);
    /* decode against the ORIGINAL geometry: a corrupted header that changes the geometry must be refused */
    if (rc == 0) rc = ffhip_jpeg_progressive_decode(file, len, &g0, cy, g0.ncomp == 3 ? cu : NULL, g0.ncomp == 3 ? cv : NULL, q, k_max);
    free(file); free(cy); free(cu); free(cv); free(q);
    if (rc != FFHIP_OK && rc != FFHIP_EINVAL) { printf("unexpected code %d at length %zu\n", rc, len); return 4; }
    if (rc == 0) ok++; else rejected++;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const int iters = atoi(argv[1]);
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *orig = malloc((size_t)n), *buf = malloc((size_t)n);
    if (fread(orig, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    int w, h, pg = 0;
    if (ffhip_jpeg_probe_any(orig, (size_t)n, &g0, &w, &h, &pg) || !pg) return 3; /* the pristine file must parse as progressive */
    int rc = run(orig, (size_t)n, 63);
    if (rc || !ok) return rc ? rc : 3;                                              /* ... and decode */
    for (long len = 0; len < n && !rc; len++) rc = run(orig, (size_t)len, 63);       /* every truncation */
    for (int it = 0; it < iters && !rc; it++) {
        memcpy(buf, orig, (size_t)n);
        const int kind = it % 4;
        if (kind == 0) for (int k = 0; k < 1 + (int)(rnd() % 8); k++) buf[rnd() % n] ^= (unsigned char)(1u << (rnd() % 8));
        else if (kind == 1) for (int k = 0; k < 1 + (int)(rnd() % 4); k++) buf[rnd() % n] = (unsigned char)rnd();
        else if (kind == 2) { size_t p = rnd() % n, l = rnd() % 16; if (p + l < (size_t)n) memset(buf + p, rnd() & 1 ? 0xFF : 0, l); }
        else { /* a scan header: component count, selectors, Ss, Se, Ah/Al */
            size_t hits[FFHIP_JPEG_MAX_SCANS], nh = 0;
            for (size_t p = 2; p + 12 < (size_t)n && nh < FFHIP_JPEG_MAX_SCANS; p++)
                if (buf[p] == 0xFF && buf[p + 1] == 0xDA) hits[nh++] = p;
            if (nh) buf[hits[rnd() % nh] + 4 + rnd() % 8] = (unsigned char)(rnd() % 3 ? rnd() % 64 : rnd());
        }
        rc = run(buf, (size_t)n, it % 7 == 0 ? (int)(rnd() % 64) : 63);
    }
    free(orig); free(buf);
    printf("decoded %d, rejected %d\n", ok, rejected);
    return rc;
}
