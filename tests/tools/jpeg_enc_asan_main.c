/* jpeg_enc_asan_main.c -- a stand-alone program over the host side of the JPEG encoder, to be built with -fsanitize=address,undefined
 * together with ffhip_jpeg_enc.c (plain C, no HIP).  Pictures of every layout, sizes around the MCU borders, qualities 1 .. 100 and restart
 * intervals 0 .. 3, noise and 0/255 content, in HEAP buffers of exactly their size, read through the three source forms (RGB by strides,
 * BGR by a negative pixel stride's worth of offsets, BGRA) and written into heap buffers of exactly `cap` bytes: cap = the file's size (the
 * file must come out whole and below the bound), cap one byte short (FFHIP_EJPEG_NOSPACE, the same length, the same bytes below cap) and
 * cap = 0.  Prints "ok <pictures>" and exits 0; any mismatch exits 1, and the sanitizers abort on their own findings. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffpic_hip.h"

static uint32_t lcg = 12345u;
static int rnd(void) { lcg = lcg * 1664525u + 1013904223u; return (int)(lcg >> 24); }

static int fail(const char *what, int w, int h, int layout, int q, int r)
{
    fprintf(stderr, "FAIL %s: %dx%d layout %d quality %d restart %d\n", what, w, h, layout, q, r);
    return 1;
}

int main(void)
{
    static const int sizes[][2] = {{1, 1}, {8, 8}, {7, 9}, {16, 16}, {17, 13}, {33, 9}, {9, 33}, {40, 24}, {65, 31}};
    static const int qualities[] = {1, 50, 75, 100};
    int count = 0;
    for (size_t si = 0; si < sizeof sizes / sizeof sizes[0]; si++)
        for (int layout = 0; layout < 4; layout++)
            for (int qi = 0; qi < 4; qi++)
                for (int restart = 0; restart < 4; restart++) {
                    const int w = sizes[si][0], h = sizes[si][1], q = qualities[qi], grey = layout == FFHIP_JPEG_ENC_GREY;
                    const int form = grey ? 0 : count % 3; /* 0 strides, 1 BGR through the offsets, 2 BGRA */
                    const int bpp = grey ? 1 : (form == 2 ? 4 : 3);
                    const size_t nbytes = (size_t)w * h * bpp;
                    uint8_t *px = (uint8_t *)malloc(nbytes);
                    if (!px) return 2;
                    for (size_t k = 0; k < nbytes; k++) px[k] = (uint8_t)(count & 1 ? (rnd() & 1) * 255 : rnd());
                    ffhip_jpeg_source s;
                    memset(&s, 0, sizeof s);
                    s.pixels = px; s.width = w; s.height = h; s.row_stride = (int64_t)w * bpp; s.pixel_stride = bpp;
                    s.channels = grey ? 1 : (form == 2 ? 4 : 3);
                    if (form == 0 && !grey) { s.chan[0] = 0; s.chan[1] = 1; s.chan[2] = 2; }
                    if (form == 1) { s.chan[0] = 2; s.chan[1] = 1; s.chan[2] = 0; }
                    size_t need = 0, len = 0;
                    if (ffhip_jpeg_encode_picture(&s, layout, q, restart, NULL, 0, &need) != FFHIP_EJPEG_NOSPACE) return fail("cap 0", w, h, layout, q, restart);
                    if (need < 100 || need > ffhip_jpeg_encode_bound(w, h, layout, restart)) return fail("bound", w, h, layout, q, restart);
                    uint8_t *whole = (uint8_t *)malloc(need), *shorter = (uint8_t *)malloc(need - 1);
                    if (!whole || !shorter) return 2;
                    if (ffhip_jpeg_encode_picture(&s, layout, q, restart, whole, need, &len) != FFHIP_OK || len != need) return fail("exact cap", w, h, layout, q, restart);
                    if (whole[0] != 0xFF || whole[1] != 0xD8 || whole[need - 2] != 0xFF || whole[need - 1] != 0xD9) return fail("SOI/EOI", w, h, layout, q, restart);
                    if (ffhip_jpeg_encode_picture(&s, layout, q, restart, shorter, need - 1, &len) != FFHIP_EJPEG_NOSPACE || len != need) return fail("short cap", w, h, layout, q, restart);
                    if (memcmp(whole, shorter, need - 1)) return fail("bytes below a short cap", w, h, layout, q, restart);
                    free(whole); free(shorter); free(px);
                    count++;
                }
    printf("ok %d\n", count);
    return 0;
}
