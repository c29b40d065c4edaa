/* ffhip_vp8_bool.h -- the VP8 bool decoder and the two per-macroblock parsers behind it, written once for the host front end
 * (ffhip_webp.c, plain C) and the device front end (ffhip_vp8_bool_gpu.hip): the arithmetic of coding/booldec.c:95-119,
 * vp8_decode_mb_header (format/webp.c:1277-1450) and vp8_get_coefficients / vp8_decode_residual_block's parse order
 * (webp.c:992-1064, 1147-1196), restated as they ARE, not as RFC 6386 has them:
 *   - `range` is kept as the range itself; a decode works on range - 1, takes split = ((range - 1) * prob) >> 8 and
 *     renormalises by 7 ^ floor(log2(range)); a byte is loaded only when `count` is negative (booldec.c:98-117);
 *   - the 11 extra bits of a cat6 token are summed in a uint8_t (DCTextra, webp.c:965-971), so they wrap modulo 256;
 *   - a block's token count is n - first at the end-of-block token and 16 when the loop runs out (webp.c:1039, 1063).
 * A decoder that wants a byte beyond its partition sets `err` and reads zeros from then on (every loop here is bounded); the
 * reference reads one byte of heap there and then exits (utils/bitstream.c:115-120).  libwebp has the same rule (a load past the
 * end sets its eof flag), yet decodes files this rule refuses: what runs those files off their first partition is the segment id
 * that ffb_mb_header reads with probabilities 0 while segmentation is off, a zero bit of which costs seven shifts. */
#ifndef FFHIP_VP8_BOOL_H
#define FFHIP_VP8_BOOL_H

#include <stdint.h>

#include "ffhip_vp8_tables.h"

#if defined(__HIPCC__)
#define FFB_FN __host__ __device__ static inline
#define FFB_TBL static constexpr
#else
#define FFB_FN static inline
#define FFB_TBL static const
#endif

typedef struct ffb_dec {
    const uint8_t *p; /* the partition */
    uint32_t pos, len;
    uint32_t value, range; /* value stays below 2^16: at most 8 bits are ever pending behind `count` */
    int32_t count;
    int32_t err; /* a byte beyond `len` was wanted */
} ffb_dec;

FFB_FN void ffb_load(ffb_dec *d)
{
    uint32_t byte = 0;
    if (d->pos < d->len) byte = d->p[d->pos++];
    else d->err = 1;
    d->value = byte | (d->value << 8);
    d->count += 8;
}

/* bool_dec_init (booldec.c:46-56) loads the first byte at once; here the first decode loads it (`count` is negative), which is the
 * same arithmetic.  So a partition that nothing is decoded from -- more token partitions than macroblock rows, or rows of skipped
 * macroblocks only -- may have any length, zero included: the reference decodes such a file (its init reads one byte it never uses). */
FFB_FN void ffb_init(ffb_dec *d, const uint8_t *p, uint32_t len)
{
    d->p = p;
    d->pos = 0;
    d->len = len;
    d->value = 0;
    d->range = 255;
    d->count = -8;
    d->err = 0;
}

FFB_FN int ffb_bit(ffb_dec *d, int prob)
{
    if (d->count < 0) ffb_load(d);
    uint32_t range = d->range - 1;
    const int pos = d->count;
    const uint32_t split = (range * (uint32_t)prob) >> 8;
    const int bit = (d->value >> pos) > split;
    if (bit) {
        range -= split;
        d->value -= (split + 1) << pos;
    } else {
        range = split + 1;
    }
    const int shift = 7 ^ (31 - __builtin_clz(range)); /* range is 1..254 here */
    d->range = range << shift;
    d->count -= shift;
    return bit;
}

FFB_FN int ffb_bits(ffb_dec *d, int n) /* bool_dec_bits: most significant bit first, probability 128 */
{
    int v = 0;
    while (n-- > 0) v |= ffb_bit(d, 128) << n;
    return v;
}

FFB_FN int ffb_sbits(ffb_dec *d, int n) /* bool_dec_signed_bits: magnitude, then the sign */
{
    const int v = ffb_bits(d, n);
    return ffb_bit(d, 128) ? -v : v;
}

/* What the frame header leaves for the macroblock headers (webp.c:1291-1300). */
typedef struct ffb_mbhdr_probs {
    uint8_t update_map;  /* update_mb_segmentation_map: 1 also when segmentation is OFF (webp.c:393), so a segment id is then read
                            from every macroblock header with the zero probabilities of the calloc'ed decoder */
    uint8_t seg_prob[3]; /* 0 unless the header set them: the reference has no 255 default */
    uint8_t no_skip;     /* mb_no_skip_coeff */
    uint8_t prob_skip;   /* prob_skip_false */
} ffb_mbhdr_probs;

/* One macroblock header.  rec[20]: the mode record of include/ffpic_hip.h ([0] y mode, [1] uv mode, [2..17] 4x4 modes, [18] segment
 * id, [19] 0); a 16x16 macroblock gets rec[2] = its y mode (webp.c:1430) and zeros behind it, where the reference leaves what
 * malloc gave it.  above4 / *left4: the four 4x4 modes along the bottom edge of the macroblock above / the right edge of the one
 * to the left, one per byte (x or y = 0 in the low byte), a 16x16 neighbour standing for four copies of its own mode and a missing
 * one for DC (webp.c:1228-1285); *left4 is replaced by this macroblock's.  Returns mb_skip_coeff. */
FFB_FN int ffb_mb_header(ffb_dec *d, const ffb_mbhdr_probs *fp, uint32_t above4, uint32_t *left4, uint8_t *rec)
{
    FFB_TBL uint8_t bmode_probs[900] = FFB_KF_BMODE_PROBS;
    int seg = 0;
    if (fp->update_map) seg = !ffb_bit(d, fp->seg_prob[0]) ? ffb_bit(d, fp->seg_prob[1]) : ffb_bit(d, fp->seg_prob[2]) + 2;
    const int skip = fp->no_skip ? ffb_bit(d, fp->prob_skip) : 0;
    int ymode; /* kf_ymode_tree with probabilities 145, 156, 163, 128 */
    if (!ffb_bit(d, 145)) ymode = 4;
    else if (!ffb_bit(d, 156)) ymode = ffb_bit(d, 163) ? 2 : 0;
    else ymode = ffb_bit(d, 128) ? 1 : 3;
    uint32_t im[16];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 16; i++) im[i] = 0;
    im[0] = (uint32_t)ymode;
    uint32_t left_out = (uint32_t)ymode * 0x01010101u;
    if (ymode == 4) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 16; i++) {
            const uint32_t a = i < 4 ? (above4 >> (8 * i)) & 255u : im[i < 4 ? 0 : i - 4];
            const uint32_t l = (i & 3) == 0 ? (*left4 >> (8 * (i >> 2))) & 255u : im[(i & 3) == 0 ? 0 : i - 1];
            const uint8_t *p = bmode_probs + (a * 10u + l) * 9u;
            uint32_t m; /* bmode_tree */
            if (!ffb_bit(d, p[0])) m = 0;                                 /* DC */
            else if (!ffb_bit(d, p[1])) m = 1;                            /* TM */
            else if (!ffb_bit(d, p[2])) m = 2;                            /* VE */
            else if (!ffb_bit(d, p[3])) {
                if (!ffb_bit(d, p[4])) m = 3;                             /* HE */
                else m = ffb_bit(d, p[5]) ? 5 : 4;                        /* VR : RD */
            } else if (!ffb_bit(d, p[6])) m = 6;                          /* LD */
            else if (!ffb_bit(d, p[7])) m = 7;                            /* VL */
            else m = ffb_bit(d, p[8]) ? 9 : 8;                            /* HU : HD */
            im[i] = m;
        }
        left_out = im[3] | im[7] << 8 | im[11] << 16 | im[15] << 24;
    }
    *left4 = left_out;
    int uv; /* uv_mode_tree with probabilities 142, 114, 183 */
    if (!ffb_bit(d, 142)) uv = 0;
    else if (!ffb_bit(d, 114)) uv = 2;
    else uv = ffb_bit(d, 183) ? 1 : 3;
    rec[0] = (uint8_t)ymode;
    rec[1] = (uint8_t)uv;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 16; i++) rec[2 + i] = (uint8_t)im[i];
    rec[18] = (uint8_t)seg;
    rec[19] = 0;
    return skip;
}

/* the bottom edge of a finished record, as the macroblock below wants it in above4 */
FFB_FN uint32_t ffb_rec_bottom4(const uint8_t *rec)
{
    if (rec[0] != 4) return (uint32_t)rec[0] * 0x01010101u;
    return (uint32_t)rec[14] | (uint32_t)rec[15] << 8 | (uint32_t)rec[16] << 16 | (uint32_t)rec[17] << 24;
}

/* vp8_get_coefficients (webp.c:992-1064) without its dequantising multiply: the LEVELS at their raster position in out[16].
 * probs: the 8 bands x 3 contexts x 11 probabilities of the block's type. */
FFB_FN int ffb_coefficients(ffb_dec *d, const uint8_t *probs, int first, int ctx, int16_t *out)
{
    FFB_TBL uint8_t pcat[4][12] = {{173, 148, 140, 0}, {176, 155, 140, 135, 0}, {180, 157, 141, 134, 130, 0},
                                   {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0}};
    const uint64_t bands = 0x7666666665463210ull;  /* coeff_bands[16], a nibble each (webp.c:1129) */
    const uint64_t zigzag = 0xfeb7adc963258410ull; /* kZigzag[16] (webp.c:1013) */
    int prev_zero = 0;
    for (int n = first; n < 16; ++n) {
        const uint8_t *p = probs + (int)((bands >> (4 * n)) & 15) * 33 + ctx * 11;
        int v;
        if (!prev_zero && !ffb_bit(d, p[0])) return n - first; /* dct_eob; not coded behind a zero */
        if (!ffb_bit(d, p[1])) {
            prev_zero = 1;
            ctx = 0;
            continue; /* out[] was cleared by the caller */
        }
        prev_zero = 0;
        if (!ffb_bit(d, p[2])) {
            v = 1;
        } else if (!ffb_bit(d, p[3])) {
            if (!ffb_bit(d, p[4])) v = 2;
            else v = 3 + ffb_bit(d, p[5]);
        } else if (!ffb_bit(d, p[6])) {
            if (!ffb_bit(d, p[7])) {
                v = 5 + ffb_bit(d, 159); /* cat1 */
            } else {
                v = 7 + 2 * ffb_bit(d, 165); /* cat2 */
                v += ffb_bit(d, 145);
            }
        } else {
            const int b1 = ffb_bit(d, p[8]);
            const int cat = 2 * b1 + ffb_bit(d, p[9 + b1]); /* 0..3 = cat3..cat6 */
            uint32_t extra = 0;
            for (const uint8_t *q = pcat[cat]; *q; ++q) extra = (2 * extra + (uint32_t)ffb_bit(d, *q)) & 255u; /* a uint8_t in the reference */
            v = (int)extra + (cat == 0 ? 11 : cat == 1 ? 19 : cat == 2 ? 35 : 67);
        }
        ctx = v == 1 ? 1 : 2;
        if (ffb_bit(d, 128)) v = -v;
        out[(zigzag >> (4 * n)) & 15] = (int16_t)v;
    }
    return 16;
}

/* The token parse of one coded macroblock (webp.c:1147-1196).  probs [4][8][3][11]; *top9 / *left9: the nine "had tokens" flags
 * of the column above / of the row so far, bit 0 the Y2 block, 1-4 luma, 5-6 U, 7-8 V; levels [25][16] must be ZERO on entry
 * (only non-zero levels are stored), counts [25] receives every block's token count. */
FFB_FN void ffb_mb_tokens(ffb_dec *d, const uint8_t *probs, int has_y2, uint32_t *top9, uint32_t *left9, int16_t *levels, uint8_t *counts)
{
    uint32_t top = *top9, left = *left9;
    int first = 0;
    const uint8_t *yp = probs + 3 * 264;
    if (has_y2) {
        const int nz = ffb_coefficients(d, probs + 264, 0, (int)(top & 1) + (int)(left & 1), levels + 24 * 16);
        counts[24] = (uint8_t)nz;
        top = (top & ~1u) | (nz > 0);
        left = (left & ~1u) | (nz > 0);
        first = 1;
        yp = probs;
    } else {
        counts[24] = 0;
    }
    for (int y = 0; y < 4; ++y) {
        uint32_t l = (left >> (y + 1)) & 1;
        for (int x = 0; x < 4; ++x) {
            const int nz = ffb_coefficients(d, yp, first, (int)((top >> (x + 1)) & 1) + (int)l, levels + (y * 4 + x) * 16);
            counts[y * 4 + x] = (uint8_t)nz;
            l = nz > 0;
            top = (top & ~(2u << x)) | (l << (x + 1));
        }
        left = (left & ~(2u << y)) | (l << (y + 1));
    }
    int blk = 16;
    for (int ch = 5; ch <= 7; ch += 2)
        for (int y = 0; y < 2; ++y) {
            uint32_t l = (left >> (y + ch)) & 1;
            for (int x = 0; x < 2; ++x, ++blk) {
                const int nz = ffb_coefficients(d, probs + 2 * 264, 0, (int)l + (int)((top >> (x + ch)) & 1), levels + blk * 16);
                counts[blk] = (uint8_t)nz;
                l = nz > 0;
                top = (top & ~(1u << (x + ch))) | (l << (x + ch));
            }
            left = (left & ~(1u << (y + ch))) | (l << (y + ch));
        }
    *top9 = top;
    *left9 = left;
}

/* a skipped macroblock's contexts (webp.c:1213-1221): 1-8 cleared always, 0 only when it has a Y2 block */
FFB_FN uint32_t ffb_skip_ctx(uint32_t ctx9, int has_y2) { return has_y2 ? 0u : ctx9 & 1u; }

#endif
