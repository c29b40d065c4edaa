/* ffhip_vp8_bool.h -- the VP8 bool decoder and the two per-macroblock parsers behind it, written once for the host front end
 * (ffhip_webp.c, plain C) and the device front end (ffhip_vp8_bool_gpu.hip): the arithmetic of coding/booldec.c:95-119,
 * vp8_decode_mb_header (format/webp.c:1277-1450) and vp8_get_coefficients / vp8_decode_residual_block's parse order
 * (webp.c:992-1064, 1147-1196), restated as they ARE, not as RFC 6386 has them (under WEBP_RULE_LIBWEBP, below, as RFC 6386 has them):
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

/* WebpPixelRule: which pixels a lossy WebP call gives, ONE compile-time value wherever it reaches generated code.  Plain host code takes it as a
 * `const int rule` that its callers pass as a literal.  Text that kernels compile is included once per rule with the rule as a macro
 * (ffhip_vp8_bool_tokens.inc, ffhip_vp8_bool_kernels.inc, ffhip_vp8_frame_items.inc, ffhip_vp8_frame_row.inc): as a function argument or a template parameter it changed
 * the names of static tables and the address arithmetic of the reference's instances, which are held to their code instruction by instruction
 * (tests/tools/isa_diff.py).
 *   WEBP_RULE_REFERENCE  the reference's WEBP_load bit for bit, with its named deviations from RFC 6386: the default
 *   WEBP_RULE_LIBWEBP    RFC 6386 as libwebp decodes it: tests/vp8_spec.py with rules=SPEC is its witness */
typedef int WebpPixelRule;
#define WEBP_RULE_REFERENCE 0
#define WEBP_RULE_LIBWEBP 1

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
                            from every macroblock header with the zero probabilities of the calloc'ed decoder.  WEBP_RULE_LIBWEBP: the
                            header reader leaves 1 here only when segmentation AND the map update are on */
    uint8_t seg_prob[3]; /* 0 unless the header set them: the reference has no 255 default (WEBP_RULE_LIBWEBP: 255) */
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

/* the token parsers, an instance per rule (ffhip_vp8_bool_tokens.inc): ffb_coefficients + ffb_mb_tokens (the reference's) and ffb_coefficients_libwebp +
 * ffb_mb_tokens_libwebp (cat6 extra bits not wrapped) */
#define FFB_COEF_NAME ffb_coefficients
#define FFB_TOKENS_NAME ffb_mb_tokens
#define FFB_COEF_RULE WEBP_RULE_REFERENCE
#include "ffhip_vp8_bool_tokens.inc"
#undef FFB_COEF_NAME
#undef FFB_TOKENS_NAME
#undef FFB_COEF_RULE
#define FFB_COEF_NAME ffb_coefficients_libwebp
#define FFB_TOKENS_NAME ffb_mb_tokens_libwebp
#define FFB_COEF_RULE WEBP_RULE_LIBWEBP
#include "ffhip_vp8_bool_tokens.inc"
#undef FFB_COEF_NAME
#undef FFB_TOKENS_NAME
#undef FFB_COEF_RULE
/* a skipped macroblock's contexts (webp.c:1213-1221): 1-8 cleared always, 0 only when it has a Y2 block */
FFB_FN uint32_t ffb_skip_ctx(uint32_t ctx9, int has_y2) { return has_y2 ? 0u : ctx9 & 1u; }

#endif
