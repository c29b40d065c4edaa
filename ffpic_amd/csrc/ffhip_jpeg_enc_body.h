/* ffhip_jpeg_enc_body.h -- the baseline JPEG ENCODER's rule (include/ffpic_hip.h, "JPEG encoding") as the host functions
 * (ffhip_jpeg_enc.c) and the kernels (ffhip_jpeg_enc_gpu.hip) compile it: libjpeg's rule, integers only.  Three parts:
 *   the SAMPLE rule (steps 2 to 4): RGB -> YCbCr, which source pixel a padded sample comes from, the two downsampling means with their
 *     alternating bias, which luma blocks of a last MCU are dummy blocks;
 *   a block's forward DCT ("islow", jfdctint.c) and QUANTISATION (steps 5 and 6);
 *   a block's CODE (step 7): its DC predecessor in the scan, its walk in zig-zag order -- one function that counts the bits and, given a
 *     sink, emits them -- the sink, and where a block's bits start behind the block in front of it.
 * Plain C; nothing here allocates or loops to a bound that depends on data. */
#ifndef FFHIP_JPEG_ENC_BODY_H
#define FFHIP_JPEG_ENC_BODY_H

#include <stddef.h>
#include <stdint.h>
#include "ffhip_jpeg_front.h" /* the zig-zag order */

#ifdef __HIPCC__
#define JE_FN __host__ __device__ static inline __attribute__((always_inline))
#define JE_UNROLL _Pragma("unroll")
#else
#define JE_FN static inline
#define JE_UNROLL
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define JE_TABLE static __constant__ const
#else
#define JE_TABLE static const
#endif

/* layouts (FFHIP_JPEG_ENC_*): luma sampling factors and components */
JE_FN int je_layout_ok(int layout) { return layout >= 0 && layout <= 3; }
JE_FN int je_layout_h(int layout) { return layout == 1 || layout == 2 ? 2 : 1; }
JE_FN int je_layout_v(int layout) { return layout == 2 ? 2 : 1; }
JE_FN int je_layout_ncomp(int layout) { return layout == 3 ? 1 : 3; }

/* ---- the sample rule ---- */
/* step 2 */
JE_FN void je_ycc(int r, int g, int b, int *y, int *cb, int *cr)
{
    *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
/* step 3.  The source column of full-resolution column x, and the source row of luma row y: the last one beyond the picture */
JE_FN int je_src_col(int x, int width) { return x < width ? x : width - 1; }
JE_FN int je_luma_src_row(int y, int height) { return y < height ? y : height - 1; }
/* the source row of row `dy` (0 .. v - 1) under chroma row cy: rows exist up to a multiple of v (copies of the last row), which gives
 * ceil(height / v) chroma rows; the chroma rows beyond them are copies of the last of THOSE */
JE_FN int je_chroma_src_row(int cy, int dy, int height, int v)
{
    const int rows = (height + v - 1) / v;
    const int r = (cy < rows ? cy : rows - 1) * v + dy;
    return r < height ? r : height - 1;
}
/* the means; cx: the chroma column (the bias alternates along a row and starts anew in every row) */
JE_FN int je_h2v2(int a, int b, int c, int d, int cx) { return (a + b + c + d + 1 + (cx & 1)) >> 2; }
JE_FN int je_h2v1(int a, int b, int cx) { return (a + b + (cx & 1)) >> 1; }
/* step 4: luma block (bx, by) of the coded picture holds no sample of the picture's own blocks */
JE_FN int je_block_is_dummy(int bx, int by, int width, int height) { return bx >= (width + 7) / 8 || by >= (height + 7) / 8; }
/* the block whose DC a luma block j of its MCU takes: itself when real, else the nearest real block in front of it in the MCU's order (block 0
 * of an MCU is real).  (mx, my): the MCU; h, v <= 2 */
JE_FN int je_dc_source(int j, int mx, int my, int h, int v, int width, int height)
{
    int src = j;
    JE_UNROLL
    for (int k = 0; k < 3; k++)
        if (src > 0 && je_block_is_dummy(mx * h + src % h, my * v + src / h, width, height)) src--;
    return src;
}

/* ---- steps 5 and 6 ---- */
#define JE_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
/* one pass over d[0], d[s], .. d[7 s]: first = the row pass (PASS1_BITS = 2 kept), else the column pass */
JE_FN void je_fdct_pass(int32_t *d, int s, int first)
{
    const int32_t t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
    const int32_t t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 11 : 15;
    d[0] = first ? (t10 + t11) * 4 : JE_DESCALE(t10 + t11, 2);
    d[4 * s] = first ? (t10 - t11) * 4 : JE_DESCALE(t10 - t11, 2);
    int32_t z1 = (t12 + t13) * 4433;
    d[2 * s] = JE_DESCALE(z1 + t13 * 6270, n);
    d[6 * s] = JE_DESCALE(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 = -z1 * 7373; z2 = -z2 * 20995; z3 = -z3 * 16069 + z5; z4 = -z4 * 3196 + z5;
    d[7 * s] = JE_DESCALE(u4 + z1 + z3, n);
    d[5 * s] = JE_DESCALE(u5 + z2 + z4, n);
    d[3 * s] = JE_DESCALE(u6 + z2 + z3, n);
    d[s] = JE_DESCALE(u7 + z1 + z4, n);
}
JE_FN int je_quantise(int32_t x, int t)
{
    const int32_t d = 8 * t, a = x < 0 ? -x : x, c = (a + (d >> 1)) / d;
    return x < 0 ? -c : c;
}
/* d: 64 samples, natural order, in; the quantised coefficients out */
JE_FN void je_fdct_quant(int32_t *d, const uint16_t *quant)
{
    JE_UNROLL
    for (int k = 0; k < 64; k++) d[k] -= 128;
    JE_UNROLL
    for (int y = 0; y < 8; y++) je_fdct_pass(d + 8 * y, 1, 1);
    JE_UNROLL
    for (int x = 0; x < 8; x++) je_fdct_pass(d + x, 8, 0);
    JE_UNROLL
    for (int k = 0; k < 64; k++) d[k] = je_quantise(d[k], quant[k]);
}

/* ---- step 7 ---- */
JE_TABLE uint8_t je_zz[64] = FFHIP_JPEG_ZIGZAG;

/* The code tables as the walk reads them: per table set (0 luma, 1 chroma) JE_TAB_WORDS words, length << 16 | code: the AC code of symbol
 * (run << 4 | size) at [symbol], the DC code of size t at [256 + t]; 0: no such code */
#define JE_TAB_WORDS 272
#define JE_BLOCK_MAX_BITS 1660 /* 11 + 11 (the longest DC code, chroma's, and its magnitude) + 63 x (16 + 10) */

JE_FN int je_nbits(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

/* Blocks of an MCU in the scan, and block g of a picture's scan: the MCU and the place in it (j < h v: luma block j; then Cb, then Cr) */
JE_FN int je_mcu_blocks(int layout) { return layout == 3 ? 1 : je_layout_h(layout) * je_layout_v(layout) + 2; }
JE_FN const int16_t *je_scan_block(const int16_t *cy, const int16_t *cu, const int16_t *cv, int hv, long long mcu, int j)
{
    return j < hv ? cy + (mcu * hv + j) * 64 : (j == hv ? cu : cv) + mcu * 64;
}
/* the DC prediction of that block: the DC of the component's block in front of it in the scan, 0 at the start of a restart interval */
JE_FN int je_scan_pred(const int16_t *cy, const int16_t *cu, const int16_t *cv, int hv, long long mcu, int j, int restart)
{
    if (j > 0 && j < hv) return cy[(mcu * hv + j - 1) * 64];
    if (mcu == 0 || (restart && mcu % restart == 0)) return 0;
    return j < hv ? cy[(mcu * hv - 1) * 64] : (j == hv ? cu : cv)[(mcu - 1) * 64];
}

/* The bit sink: bits go out most significant first in 32-bit words, stored so that the bytes in memory are the stream's.  A block's first
 * and last word may hold bits of its neighbours: those are OR-ed in (the words start as zeros; atomically on the device), the words
 * between them are its own and are stored. */
typedef struct je_sink {
    uint64_t acc;
    int n;            /* bits held in acc (below 32 between calls) */
    int shared;       /* the next word out may hold another block's bits */
    uint64_t idx;     /* the next word */
    uint32_t *words;
} je_sink;
JE_FN void je_word_out(uint32_t *words, uint64_t idx, uint32_t w, int shared)
{
    const uint32_t v = __builtin_bswap32(w);
#ifdef __HIP_DEVICE_COMPILE__
    if (shared) atomicOr(words + idx, v);
    else words[idx] = v;
#else
    (void)shared;
    words[idx] |= v;
#endif
}
JE_FN void je_sink_open(je_sink *s, uint32_t *words, uint64_t bit)
{
    s->acc = 0; s->n = (int)(bit & 31); s->shared = s->n != 0; s->idx = bit >> 5; s->words = words;
}
/* len <= 27 bits of `code` (nothing set above them) */
JE_FN void je_put(je_sink *s, uint32_t code, int len)
{
    s->acc = (s->acc << len) | code;
    s->n += len;
    if (s->n >= 32) {
        je_word_out(s->words, s->idx++, (uint32_t)(s->acc >> (s->n - 32)), s->shared);
        s->shared = 0;
        s->n -= 32;
    }
}
JE_FN void je_sink_close(je_sink *s)
{
    if (s->n > 0) je_word_out(s->words, s->idx, (uint32_t)(s->acc << (32 - s->n)), 1);
}

/* One block's code (T.81 F.1.2): the bits it takes; with a sink they are emitted too.  tab: the component's JE_TAB_WORDS words.  A DC
 * difference beyond +-2047 or an AC magnitude beyond 1023 has no code in Annex K's tables: *bad is set, the size is taken as the largest
 * (the count and the emission still agree, and stay below JE_BLOCK_MAX_BITS). */
JE_FN int je_block_code(const int16_t *blk, int pred, const uint32_t *tab, je_sink *s, int *bad)
{
    const int diff = (int)blk[0] - pred;
    int t = je_nbits(diff < 0 ? -diff : diff);
    if (t > 11) { *bad = 1; t = 11; }
    uint32_t e = tab[256 + t];
    int bits = (int)(e >> 16) + t;
    if (s) je_put(s, ((e & 0xffffu) << t) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << t) - 1u)), (int)(e >> 16) + t);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = blk[je_zz[k]];
        if (v == 0) { run++; continue; }
        JE_UNROLL
        for (int z = 0; z < 3; z++) /* a run of up to 62 zeros: up to three ZRL */
            if (run > 15) {
                const uint32_t zrl = tab[0xF0];
                bits += (int)(zrl >> 16);
                if (s) je_put(s, zrl & 0xffffu, (int)(zrl >> 16));
                run -= 16;
            }
        t = je_nbits(v < 0 ? -v : v);
        if (t > 10) { *bad = 1; t = 10; }
        e = tab[(run << 4) | t];
        bits += (int)(e >> 16) + t;
        if (s) je_put(s, ((e & 0xffffu) << t) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << t) - 1u)), (int)(e >> 16) + t);
        run = 0;
    }
    if (run > 0) {
        e = tab[0];
        bits += (int)(e >> 16);
        if (s) je_put(s, e & 0xffffu, (int)(e >> 16));
    }
    return bits;
}

/* Where bits go in the UNSTUFFED stream of a picture's scan: block after block; a block that starts a restart interval (not the picture's
 * first) starts behind the padding of the interval in front of it and the two bytes of its RSTn marker.  The stream ends with the last
 * interval's padding and the two bytes of EOI.  The markers lie in the unstuffed stream with a bit set for their FF in a mask of one bit per
 * byte: the stuffing pass leaves those FF alone.
 * As a function of the position p in front of a run of blocks this is p -> p + a (no interval starts in the run) or
 * p -> roundup8(p + a) + c (one does: what follows the first start no longer depends on p, a multiple of 8 being in front of it).  je_span is
 * that function and je_span_join its composition -- associative, so the positions are a prefix scan. */
typedef struct je_span { uint64_t a, c; int starts; } je_span;
JE_FN uint64_t je_up8(uint64_t p) { return (p + 7) & ~(uint64_t)7; }
JE_FN je_span je_span_block(int bits, int starts_interval)
{
    je_span r;
    r.starts = starts_interval; r.a = starts_interval ? 0 : (uint64_t)bits; r.c = starts_interval ? 16 + (uint64_t)bits : 0;
    return r;
}
JE_FN je_span je_span_join(je_span x, je_span y) /* x, then y */
{
    je_span r;
    if (!x.starts) { r.starts = y.starts; r.a = x.a + y.a; r.c = y.c; }
    else { r.starts = 1; r.a = x.a; r.c = y.starts ? je_up8(x.c + y.a) + y.c : x.c + y.a; }
    return r;
}
JE_FN uint64_t je_span_apply(je_span x, uint64_t p) { return x.starts ? je_up8(p + x.a) + x.c : p + x.a; }

/* what the LAST block of an interval emits behind its own bits, its bits ending at `end`: ones up to the byte, then the marker (RSTn of the
 * interval that follows, n = its number - 1 modulo 8; or EOI), whose first byte gets its bit in the mask */
JE_FN void je_interval_end(je_sink *s, uint64_t end, int marker, uint32_t *mask)
{
    const int pad = (int)(je_up8(end) - end);
    if (pad) je_put(s, (1u << pad) - 1u, pad);
    je_put(s, 0xFF00u | (uint32_t)marker, 16);
    const uint64_t byte = je_up8(end) >> 3;
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(mask + (byte >> 5), 1u << (byte & 31));
#else
    mask[byte >> 5] |= 1u << (byte & 31);
#endif
}

#endif
