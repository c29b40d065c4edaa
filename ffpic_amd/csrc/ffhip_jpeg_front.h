/* ffhip_jpeg_front.h -- where a JPEG header is read (ffhip_jpeg_front.c): what the baseline parser (ffhip_entropy.c), the progressive
 * parser (ffhip_jpeg_progressive.c), the EXIF reader (ffhip_exif.c) and the device front ends share.  The parsers differ in policy, not in reading:
 * every difference is an argument here and a commented choice at the call site.  Internal to libffpic_hip.so. */
#ifndef FFHIP_JPEG_FRONT_H
#define FFHIP_JPEG_FRONT_H

#include <stddef.h>
#include <stdint.h>
#include "ffpic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the zig-zag order (natural index of the k-th coefficient of a scan), as an initialiser: every table of it chooses its own storage */
#define FFHIP_JPEG_ZIGZAG                                                                                                                  \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,         \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

#define LOOK 9
struct huff { /* uploaded whole and read by the kernels: size and offsets are fixed */
    uint16_t look[1 << LOOK]; /* (length << 8) | symbol, 0 = not resolvable in LOOK bits */
    int32_t maxcode[18];      /* per length, -1 if none */
    int32_t valptr[17], mincode[17];
    uint8_t vals[256];
    int present;
    /* AC tables: when code and magnitude bits both fit into LOOK bits, the whole coefficient in one
     * look-up: (value << 8) | (run << 4) | (code length + magnitude bits), 0 = take the slow path */
    int16_t fast[1 << LOOK];
};
/* the table of a DHT entry: look, maxcode, valptr, mincode, vals, present; fast[] zero.  -1: more codes than values, or over-subscribed */
int ffhip_jpeg_huff_build(struct huff *h, const uint8_t counts[16], const uint8_t *vals, int nvals);
void ffhip_jpeg_huff_fast(struct huff *h); /* fast[] from look[], behind the build */

struct jpeg_frame {
    int width, height, ncomp;
    int h[3], v[3], tq[3], cid[3];
    uint16_t quant[4][64]; /* natural order; 1 where no DQT has spoken */
};

/* The marker walk, from behind SOI: the fill bytes, the length and both bounds checks are here; what an event means is the caller's.  A SEGMENT
 * (marker, its payload seg[0 .. seg_len) inside the file), a STANDALONE marker (TEM, RSTn), EOI, MALFORMED (no FF where a marker stands, fill
 * bytes up to the end, a length below 2 or past the end), END (fewer than two bytes left). */
enum jpeg_event { JPEG_SEGMENT, JPEG_STANDALONE, JPEG_EOI, JPEG_MALFORMED, JPEG_END };
struct jpeg_walk {
    const uint8_t *f, *seg;
    size_t len, p, seg_len; /* p: where the next marker stands; the caller's to move (behind a scan's bytes) */
    int marker;
};
int ffhip_jpeg_walk_open(struct jpeg_walk *w, const uint8_t *f, size_t len); /* -1: fewer than 4 bytes, or no SOI */
enum jpeg_event ffhip_jpeg_walk_next(struct jpeg_walk *w);

/* The segment readers: 0, or -1 for a segment that is refused. */
int ffhip_jpeg_read_dqt(const uint8_t *s, size_t sl, uint16_t quant[4][64], int max_prec); /* entries of prec + 1 bytes, the first two kept; prec <= max_prec */
/* fast: every table built gets its one-look-up step; defined (or NULL): |= 1 << slot for every table built (0..3 DC, 4..7 AC), also of a segment refused further on */
int ffhip_jpeg_read_dht(const uint8_t *s, size_t sl, struct huff dc[4], struct huff ac[4], int fast, unsigned *defined);
int ffhip_jpeg_read_sof(const uint8_t *s, size_t sl, struct jpeg_frame *fr); /* 8-bit, 1 or 3 components, no zero size, tq <= 3; quant untouched */
int ffhip_jpeg_read_dri(const uint8_t *s, size_t sl, int *restart);
/* the layouts the reconstruction takes: one component is 1 x 1 whatever it says (set here), h x v <= 4 for the first, chroma 1 x 1; -1 otherwise */
int ffhip_jpeg_frame_layout(struct jpeg_frame *fr);
void ffhip_jpeg_frame_geom(const struct jpeg_frame *fr, ffhip_jpeg_geom *geom);
static inline int ffhip_jpeg_geom_same(const ffhip_jpeg_geom *a, const ffhip_jpeg_geom *b) /* same layout and MCU grid (qt_id is not compared) */
{
    return a->mcu_cols == b->mcu_cols && a->mcu_rows == b->mcu_rows && a->ncomp == b->ncomp && a->h == b->h && a->v == b->v;
}

#ifdef __cplusplus
}
#endif
#endif
