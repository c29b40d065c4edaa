/* ffhip_vp8_enc_body.h -- the lossy WebP encoder's rule (include/ffpic_hip.h "Lossy WebP encoding") as ONE body for the
 * host entries (ffhip_vp8_enc.c, gcc) and the kernels (ffhip_vp8_enc_gpu.hip, hipcc).  Five parts:
 *   COLOUR        a source pixel, a luma sample and a chroma sample of the padded planes
 *   TRANSFORMS    the forward DCT and WHT, RFC 6386's inverse pair, the quantiser
 *   MACROBLOCK    v8e_mb: one macroblock from the source planes and its neighbours' reconstruction to modes, levels, its own reconstruction
 *                 and its non-zero mask.  Written for lanes lane, lane + nl, ..: the host runs it with (0, 1), a wave with (lane, 64); what a
 *                 wave synchronises and reduces is V8E_SYNC and v8e_reduce8, which are nothing on the host
 *   BOOL CODER    tests/vp8_writer.py's BoolEncoder; the first partition and a token partition written with it
 *   FILE          the head, the sizes and a copy of any range of the file's bytes
 * Integers only; every loop runs to a bound known at its entry, but for the carry of the bool coder, which walks back over the bytes it wrote. */
#ifndef FFHIP_VP8_ENC_BODY_H
#define FFHIP_VP8_ENC_BODY_H

#include <stddef.h>
#include <stdint.h>

#include "ffpic_hip.h"
#include "ffhip_vp8_tables.h"

#ifdef __HIPCC__
#define V8E_FN __host__ __device__ static inline
#else
#define V8E_FN static inline
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define V8E_TABLE static __constant__ const
#define V8E_SYNC() __syncthreads()
#else
#define V8E_TABLE static const
#define V8E_SYNC() ((void)0)
#endif

#define V8E_MAX_SIDE 16383
#define V8E_LEVEL_MAX 2047
#define V8E_P0_MAX ((1u << 19) - 1)   /* the frame tag holds the first partition's size in 19 bits */
#define V8E_PART_MAX ((1u << 24) - 1) /* a partition size is three bytes */
/* BOUND.  A coded bit shifts the coder by 7 bits at most (the range stays in 128..255, a split is 1 at least), whatever its probability; a
 * flush adds 4 bytes.  The header is 1094 coded bits, a macroblock header 7 (skip, three of the luma tree, three of the chroma tree).  A
 * coefficient is 19 at most -- not end-of-block, the six nodes down to cat6, cat6's eleven extra bits for a level up to 2047 + 67, the sign
 * -- so a block of 16 is 16 x 19 + 1 for the end-of-block, a luma block behind Y2 15 x 19 + 1: 16 x 286 + 9 x 305 = 7321 a macroblock. */
#define V8E_HEADER_BITS 1094
#define V8E_MB_HEADER_BITS 7
#define V8E_MB_TOKEN_BITS 7321

V8E_TABLE uint8_t v8e_probs[1056] = FFB_DEFAULT_COEFF_PROBS;
V8E_TABLE uint8_t v8e_update_probs[1056] = FFB_COEFF_UPDATE_PROBS;
V8E_TABLE uint8_t v8e_zigzag[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
V8E_TABLE uint8_t v8e_bands[16] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7};
V8E_TABLE uint8_t v8e_pcat[4][11] = {{173, 148, 140}, {176, 155, 140, 135}, {180, 157, 141, 134, 130}, {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129}};
V8E_TABLE uint8_t v8e_cat_bits[4] = {3, 4, 5, 11};
V8E_TABLE uint8_t v8e_cat_base[4] = {11, 19, 35, 67};

V8E_FN int v8e_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
V8E_FN int v8e_mb_cols(int width) { return (width + 15) >> 4; }
V8E_FN uint64_t v8e_p0_bound(uint64_t n_mb) { return (7 * (V8E_HEADER_BITS + V8E_MB_HEADER_BITS * n_mb) + 7) / 8 + 4; }
V8E_FN uint64_t v8e_part_bound(uint64_t n_mb) { return (7 * V8E_MB_TOKEN_BITS * n_mb + 7) / 8 + 4; }
/* token partitions: the largest power of two <= min(8, rows), as its logarithm */
V8E_FN int v8e_log2_parts(int rows) { return rows >= 8 ? 3 : rows >= 4 ? 2 : rows >= 2 ? 1 : 0; }
V8E_FN int v8e_part_rows(int rows, int parts, int p) { return (rows - p + parts - 1) / parts; }
V8E_FN int v8e_auto_filter(int y_ac_qi) { const int f = (5 * y_ac_qi) >> 4; return f > 63 ? 63 : f; }

/* ---------------------------------------------------------------------------------------------------------------- COLOUR */
/* pixel (x, y), the last column and row repeated beyond the picture */
V8E_FN void v8e_rgb(const ffhip_jpeg_source *s, int x, int y, int *r, int *g, int *b)
{
    if (x >= s->width) x = s->width - 1;
    if (y >= s->height) y = s->height - 1;
    const uint8_t *p = s->pixels + (int64_t)y * s->row_stride + (int64_t)x * s->pixel_stride;
    if (s->channels == 1) {
        *r = *g = *b = p[s->chan[0]];
    } else {
        *r = p[s->chan[0]]; *g = p[s->chan[1]]; *b = p[s->chan[2]];
    }
}
V8E_FN int v8e_luma(const ffhip_jpeg_source *s, int x, int y)
{
    int r, g, b;
    v8e_rgb(s, x, y, &r, &g, &b);
    return (16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16;
}
/* chroma sample (cx, cy) of the padded planes: the sums over its 2 x 2 cell; the chroma planes' own last column and row repeated */
V8E_FN void v8e_chroma(const ffhip_jpeg_source *s, int cx, int cy, int *u, int *v)
{
    const int cw = (s->width + 1) >> 1, ch = (s->height + 1) >> 1;
    if (cx >= cw) cx = cw - 1;
    if (cy >= ch) cy = ch - 1;
    int r = 0, g = 0, b = 0;
    for (int k = 0; k < 4; k++) {
        int pr, pg, pb;
        v8e_rgb(s, 2 * cx + (k & 1), 2 * cy + (k >> 1), &pr, &pg, &pb);
        r += pr; g += pg; b += pb;
    }
    *u = v8e_clip8((-9719 * r - 19081 * g + 28800 * b + (128 << 18) + (1 << 17)) >> 18);
    *v = v8e_clip8((28800 * r - 24116 * g - 4684 * b + (128 << 18) + (1 << 17)) >> 18);
}

/* ---------------------------------------------------------------------------------------------------------------- TRANSFORMS */
/* d: source less prediction, 4 x 4 in raster order; o: the coefficients */
V8E_FN void v8e_fdct(const int *d, int *o)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
        t[4 * i] = (a0 + a1) * 8;
        t[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
        t[4 * i + 2] = (a0 - a1) * 8;
        t[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
    }
    for (int i = 0; i < 4; i++) {
        const int a0 = t[i] + t[12 + i], a1 = t[4 + i] + t[8 + i], a2 = t[4 + i] - t[8 + i], a3 = t[i] - t[12 + i];
        o[i] = (a0 + a1 + 7) >> 4;
        o[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0);
        o[8 + i] = (a0 - a1 + 7) >> 4;
        o[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
    }
}
/* x: the sixteen luma DC coefficients, blocks in raster order; o: the Y2 block */
V8E_FN void v8e_fwht(const int *x, int *o)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = x[4 * i] + x[4 * i + 2], a1 = x[4 * i + 1] + x[4 * i + 3], a2 = x[4 * i + 1] - x[4 * i + 3], a3 = x[4 * i] - x[4 * i + 2];
        t[4 * i] = a0 + a1; t[4 * i + 1] = a3 + a2; t[4 * i + 2] = a3 - a2; t[4 * i + 3] = a0 - a1;
    }
    for (int i = 0; i < 4; i++) {
        const int a0 = t[i] + t[8 + i], a1 = t[4 + i] + t[12 + i], a2 = t[4 + i] - t[12 + i], a3 = t[i] - t[8 + i];
        o[i] = (a0 + a1) >> 1; o[4 + i] = (a3 + a2) >> 1; o[8 + i] = (a3 - a2) >> 1; o[12 + i] = (a0 - a1) >> 1;
    }
}
/* RFC 6386 section 14.3: the vertical pass first */
V8E_FN int v8e_mul1(int x) { return x + ((x * 20091) >> 16); }
V8E_FN int v8e_mul2(int x) { return (x * 35468) >> 16; }
V8E_FN void v8e_idct(const int *c, int *o)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
        const int cc = v8e_mul2(c[4 + i]) - v8e_mul1(c[12 + i]), dd = v8e_mul1(c[4 + i]) + v8e_mul2(c[12 + i]);
        t[i] = a + dd; t[4 + i] = b + cc; t[8 + i] = b - cc; t[12 + i] = a - dd;
    }
    for (int r = 0; r < 4; r++) {
        const int a = t[4 * r] + t[4 * r + 2], b = t[4 * r] - t[4 * r + 2];
        const int cc = v8e_mul2(t[4 * r + 1]) - v8e_mul1(t[4 * r + 3]), dd = v8e_mul1(t[4 * r + 1]) + v8e_mul2(t[4 * r + 3]);
        o[4 * r] = (a + dd + 4) >> 3; o[4 * r + 1] = (b + cc + 4) >> 3; o[4 * r + 2] = (b - cc + 4) >> 3; o[4 * r + 3] = (a - dd + 4) >> 3;
    }
}
V8E_FN void v8e_iwht(const int *c, int *o)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = c[i] + c[12 + i], a1 = c[4 + i] + c[8 + i], a2 = c[4 + i] - c[8 + i], a3 = c[i] - c[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
    for (int r = 0; r < 4; r++) {
        const int a0 = t[4 * r] + t[4 * r + 3], a1 = t[4 * r + 1] + t[4 * r + 2], a2 = t[4 * r + 1] - t[4 * r + 2], a3 = t[4 * r] - t[4 * r + 3];
        o[4 * r] = (a0 + a1 + 3) >> 3; o[4 * r + 1] = (a3 + a2 + 3) >> 3; o[4 * r + 2] = (a0 - a1 + 3) >> 3; o[4 * r + 3] = (a3 - a2 + 3) >> 3;
    }
}
V8E_FN int v8e_quantise(int c, int step, int bias)
{
    const int a = c < 0 ? -c : c;
    int l = (a + bias) / step;
    if (l > V8E_LEVEL_MAX) l = V8E_LEVEL_MAX;
    return c < 0 ? -l : l;
}
/* a decoder holds a dequantised coefficient in 16 bits */
V8E_FN int v8e_dequantise(int level, int step) { return (int16_t)(level * step); }

/* ---------------------------------------------------------------------------------------------------------------- MACROBLOCK */
/* a picture as the macroblock and partition bodies see it: planes of the whole macroblock grid (luma stride 16 cols, chroma 8 cols) */
typedef struct v8e_pic {
    const uint8_t *sy, *su, *sv; /* the source planes, padded */
    uint8_t *ry, *ru, *rv;       /* the reconstruction */
    int16_t *levels;             /* [n][25][16]: raster positions; 16 Y, 4 U, 4 V, Y2 */
    uint8_t *ymode, *uvmode;     /* [n]: 0 DC, 1 TM, 2 V, 3 H */
    uint32_t *mask;              /* [n]: bit b set: block b has a non-zero level; 0: the macroblock is skipped */
    int32_t cols, rows;
    uint16_t q[6];               /* the steps: y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac */
    uint16_t pad[2];
} v8e_pic;

/* a macroblock's working store: LDS of its wave on the device */
typedef struct v8e_mb_store {
    uint8_t src[384];             /* Y 16 x 16, U 8 x 8, V 8 x 8 */
    uint8_t above[3][16], left[3][16];
    uint8_t corner[4], dc[4];
    int16_t coef[24][16];
    int16_t dcs[16];              /* the luma DCs the inverse WHT gives back */
    uint8_t nz[28];
} v8e_mb_store;

/* sample i of src[]: its plane (0 Y, 1 U, 2 V) and where it lies in it */
V8E_FN int v8e_sample_plane(int i, int *x, int *y)
{
    if (i < 256) { *x = i & 15; *y = i >> 4; return 0; }
    *x = i & 7; *y = (i >> 3) & 7;
    return i < 320 ? 1 : 2;
}
/* block b of the 24: its plane and the sample its first coefficient stands for */
V8E_FN int v8e_block_plane(int b, int *x0, int *y0)
{
    if (b < 16) { *x0 = 4 * (b & 3); *y0 = 4 * (b >> 2); return 0; }
    *x0 = 4 * (b & 1); *y0 = 4 * ((b >> 1) & 1);
    return b < 20 ? 1 : 2;
}
V8E_FN int v8e_pred(const v8e_mb_store *m, int pl, int mode, int x, int y)
{
    const int a = m->above[pl][x], l = m->left[pl][y];
    if (mode == 0) return m->dc[pl];
    if (mode == 1) return v8e_clip8(l + a - m->corner[pl]);
    return mode == 2 ? a : l;
}
/* the lowest mode with the smallest sum */
V8E_FN int v8e_best4(const uint32_t *s)
{
    int best = 0;
    for (int k = 1; k < 4; k++)
        if (s[k] < s[best]) best = k;
    return best;
}
/* the eight sums over the wave; nothing on the host, whose one "lane" has them all */
V8E_FN void v8e_reduce8(uint32_t *s)
{
#ifdef __HIP_DEVICE_COMPILE__
    for (int k = 0; k < 8; k++)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
#else
    (void)s;
#endif
}

V8E_FN void v8e_mb(const v8e_pic *p, v8e_mb_store *m, int mbx, int mby, int lane, int nl)
{
    const int64_t ys = 16 * (int64_t)p->cols, cs = 8 * (int64_t)p->cols, mb = (int64_t)mby * p->cols + mbx;
    /* the source, and the edges: the neighbours' reconstruction, 127 above the picture, 129 left of it */
    for (int i = lane; i < 384; i += nl) {
        int x, y;
        const int pl = v8e_sample_plane(i, &x, &y);
        const uint8_t *s = pl == 0 ? p->sy : pl == 1 ? p->su : p->sv;
        const int64_t st = pl ? cs : ys;
        const int n = pl ? 8 : 16;
        m->src[i] = s[((int64_t)mby * n + y) * st + (int64_t)mbx * n + x];
    }
    for (int i = lane; i < 96; i += nl) {
        const int pl = i >> 5, k = i & 15, n = pl ? 8 : 16;
        if (k >= n) continue;
        const uint8_t *r = pl == 0 ? p->ry : pl == 1 ? p->ru : p->rv;
        const int64_t st = pl ? cs : ys;
        if (i & 16)
            m->left[pl][k] = (uint8_t)(mbx ? r[((int64_t)mby * n + k) * st + (int64_t)mbx * n - 1] : 129);
        else
            m->above[pl][k] = (uint8_t)(mby ? r[((int64_t)mby * n - 1) * st + (int64_t)mbx * n + k] : 127);
    }
    for (int pl = lane; pl < 3; pl += nl) {
        const uint8_t *r = pl == 0 ? p->ry : pl == 1 ? p->ru : p->rv;
        const int64_t st = pl ? cs : ys;
        const int n = pl ? 8 : 16;
        m->corner[pl] = (uint8_t)(mby == 0 ? 127 : mbx == 0 ? 129 : r[((int64_t)mby * n - 1) * st + (int64_t)mbx * n - 1]);
    }
    V8E_SYNC();
    for (int pl = lane; pl < 3; pl += nl) {
        const int n = pl ? 8 : 16, sh = pl ? 3 : 4;
        int sa = 0, sl = 0;
        for (int k = 0; k < n; k++) { sa += m->above[pl][k]; sl += m->left[pl][k]; }
        m->dc[pl] = (uint8_t)(!mbx && !mby ? 128 : !mby ? (sl + (1 << (sh - 1))) >> sh : !mbx ? (sa + (1 << (sh - 1))) >> sh : (sa + sl + (1 << sh)) >> (sh + 1));
    }
    V8E_SYNC();
    /* MODES: the sums of squared differences, luma modes in [0, 4), chroma in [4, 8) */
    uint32_t sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lane; i < 384; i += nl) {
        int x, y;
        const int pl = v8e_sample_plane(i, &x, &y), s = m->src[i];
        for (int k = 0; k < 4; k++) {
            const int d = s - v8e_pred(m, pl, k, x, y);
            sums[(pl ? 4 : 0) + k] += (uint32_t)(d * d);
        }
    }
    v8e_reduce8(sums);
    const int ym = v8e_best4(sums), uvm = v8e_best4(sums + 4);
    /* the 24 forward DCTs, a block a lane */
    for (int b = lane; b < 24; b += nl) {
        int x0, y0, d[16], o[16];
        const int pl = v8e_block_plane(b, &x0, &y0), n = pl ? 8 : 16, base = pl == 0 ? 0 : pl == 1 ? 256 : 320, mode = pl ? uvm : ym;
        for (int i = 0; i < 16; i++) {
            const int x = x0 + (i & 3), y = y0 + (i >> 2);
            d[i] = m->src[base + y * n + x] - v8e_pred(m, pl, mode, x, y);
        }
        v8e_fdct(d, o);
        for (int i = 0; i < 16; i++) m->coef[b][i] = (int16_t)o[i];
    }
    V8E_SYNC();
    /* the WHT pair: the Y2 block's levels, and the luma DCs a decoder gets back from them */
    for (int t = lane; t < 1; t += nl) {
        int x[16], o[16], c[16];
        int16_t *lv = p->levels + (mb * 25 + 24) * 16;
        for (int b = 0; b < 16; b++) x[b] = m->coef[b][0];
        v8e_fwht(x, o);
        int any = 0;
        for (int i = 0; i < 16; i++) {
            const int step = p->q[i ? 3 : 2], l = v8e_quantise(o[i], step, step >> 1);
            lv[i] = (int16_t)l;
            any |= l;
            c[i] = v8e_dequantise(l, step);
        }
        v8e_iwht(c, o);
        for (int b = 0; b < 16; b++) m->dcs[b] = (int16_t)o[b];
        m->nz[24] = (uint8_t)(any != 0);
    }
    V8E_SYNC();
    /* levels, and the 24 inverse DCTs onto the prediction: the reconstruction */
    for (int b = lane; b < 24; b += nl) {
        int x0, y0, c[16], o[16];
        const int pl = v8e_block_plane(b, &x0, &y0), n = pl ? 8 : 16, mode = pl ? uvm : ym;
        const int dcq = p->q[pl ? 4 : 0], acq = p->q[pl ? 5 : 1];
        int16_t *lv = p->levels + (mb * 25 + b) * 16;
        int any = 0;
        for (int i = 0; i < 16; i++) {
            int l = 0;
            if (i) l = v8e_quantise(m->coef[b][i], acq, (3 * acq) >> 3);
            else if (pl) l = v8e_quantise(m->coef[b][0], dcq, dcq >> 1);
            lv[i] = (int16_t)l;
            any |= l;
            c[i] = v8e_dequantise(l, i ? acq : dcq);
        }
        if (!pl) c[0] = m->dcs[b];
        m->nz[b] = (uint8_t)(any != 0);
        v8e_idct(c, o);
        uint8_t *r = pl == 0 ? p->ry : pl == 1 ? p->ru : p->rv;
        const int64_t st = pl ? cs : ys;
        for (int i = 0; i < 16; i++) {
            const int x = x0 + (i & 3), y = y0 + (i >> 2);
            r[((int64_t)mby * n + y) * st + (int64_t)mbx * n + x] = (uint8_t)v8e_clip8(v8e_pred(m, pl, mode, x, y) + o[i]);
        }
    }
    V8E_SYNC();
    for (int t = lane; t < 1; t += nl) {
        uint32_t mask = 0;
        for (int b = 0; b < 25; b++) mask |= (uint32_t)m->nz[b] << b;
        p->mask[mb] = mask;
        p->ymode[mb] = (uint8_t)ym;
        p->uvmode[mb] = (uint8_t)uvm;
    }
}

/* ---------------------------------------------------------------------------------------------------------------- BOOL CODER */
typedef struct v8e_bool {
    uint8_t *out;
    uint64_t n;
    uint32_t range, bottom;
    int32_t count;
} v8e_bool;

V8E_FN void v8e_bool_init(v8e_bool *e, uint8_t *out) { e->out = out; e->n = 0; e->range = 255; e->bottom = 0; e->count = 24; }
V8E_FN void v8e_carry(v8e_bool *e)
{
    uint64_t i = e->n;
    while (i > 0 && e->out[i - 1] == 255) e->out[--i] = 0;
    if (i > 0) e->out[i - 1]++;
}
V8E_FN void v8e_put(v8e_bool *e, int bit, int prob)
{
    const uint32_t split = 1 + (((e->range - 1) * (uint32_t)prob) >> 8);
    if (bit) {
        e->bottom += split;
        e->range -= split;
    } else
        e->range = split;
    while (e->range < 128) {
        e->range <<= 1;
        if (e->bottom & 0x80000000u) v8e_carry(e);
        e->bottom <<= 1;
        if (!--e->count) {
            e->out[e->n++] = (uint8_t)(e->bottom >> 24);
            e->bottom &= 0xffffffu;
            e->count = 8;
        }
    }
}
V8E_FN void v8e_bits(v8e_bool *e, int v, int n)
{
    for (int k = n - 1; k >= 0; k--) v8e_put(e, (v >> k) & 1, 128);
}
/* -> the partition's size */
V8E_FN uint64_t v8e_flush(v8e_bool *e)
{
    int c = e->count;
    uint32_t v = e->bottom;
    if (v & (1u << (32 - c))) v8e_carry(e);
    v <<= c & 7;
    for (c >>= 3; c > 0; c--) v <<= 8;
    for (int k = 0; k < 4; k++) {
        e->out[e->n++] = (uint8_t)(v >> 24);
        v <<= 8;
    }
    return e->n;
}

/* prob_skip_false of a picture with `coded` macroblocks that are not skipped among `total` */
V8E_FN int v8e_prob_skip(uint64_t coded, uint64_t total)
{
    const uint64_t v = (256 * coded + total / 2) / total;
    return v < 1 ? 1 : v > 255 ? 255 : (int)v;
}

/* the first partition: the frame header and a header a macroblock, into out[] (v8e_p0_bound bytes at least) -> its size */
V8E_FN uint64_t v8e_first_partition(const v8e_pic *p, int y_ac_qi, int filter, uint8_t *out)
{
    const int64_t n_mb = (int64_t)p->cols * p->rows;
    uint64_t coded = 0;
    for (int64_t mb = 0; mb < n_mb; mb++) coded += p->mask[mb] != 0;
    const int prob_skip = v8e_prob_skip(coded, (uint64_t)n_mb);
    v8e_bool e;
    v8e_bool_init(&e, out);
    v8e_put(&e, 0, 128);      /* colour space */
    v8e_put(&e, 0, 128);      /* clamping needed */
    v8e_put(&e, 0, 128);      /* no segmentation */
    v8e_put(&e, 0, 128);      /* the normal filter */
    v8e_bits(&e, filter, 6);
    v8e_bits(&e, 0, 3);       /* sharpness */
    v8e_put(&e, 0, 128);      /* no filter deltas */
    v8e_bits(&e, v8e_log2_parts(p->rows), 2);
    v8e_bits(&e, y_ac_qi, 7);
    for (int k = 0; k < 5; k++) v8e_put(&e, 0, 128); /* no quantiser deltas */
    v8e_put(&e, 0, 128);      /* refresh_entropy_probs */
    for (int i = 0; i < 1056; i++) v8e_put(&e, 0, v8e_update_probs[i]);
    v8e_put(&e, 1, 128);      /* mb_no_skip_coeff */
    v8e_bits(&e, prob_skip, 8);
    for (int64_t mb = 0; mb < n_mb; mb++) {
        v8e_put(&e, p->mask[mb] == 0, prob_skip);
        const int ym = p->ymode[mb], uvm = p->uvmode[mb];
        v8e_put(&e, 1, 145);  /* not B_PRED */
        v8e_put(&e, ym & 1, 156);                      /* DC, V | TM, H */
        if (ym & 1) v8e_put(&e, ym == 1, 128);
        else v8e_put(&e, ym == 2, 163);
        v8e_put(&e, uvm != 0, 142);
        if (uvm) {
            v8e_put(&e, uvm != 2, 114);
            if (uvm != 2) v8e_put(&e, uvm == 1, 183);
        }
    }
    return v8e_flush(&e);
}

/* one block's tokens (RFC 6386 section 13): levels at raster positions, from position `first`, an end-of-block behind the last non-zero */
V8E_FN void v8e_put_block(v8e_bool *e, const int16_t *lv, int type, int first, int ctx)
{
    int last = -1;
    for (int n = first; n < 16; n++)
        if (lv[v8e_zigzag[n]]) last = n;
    int prev_zero = 0;
    for (int n = first; n < 16; n++) {
        const uint8_t *pr = v8e_probs + type * 264 + v8e_bands[n] * 33 + ctx * 11;
        if (!prev_zero) {
            if (n > last) {
                v8e_put(e, 0, pr[0]);
                return;
            }
            v8e_put(e, 1, pr[0]);
        }
        const int c = lv[v8e_zigzag[n]], v = c < 0 ? -c : c;
        if (!v) {
            v8e_put(e, 0, pr[1]);
            prev_zero = 1; ctx = 0;
            continue;
        }
        v8e_put(e, 1, pr[1]);
        if (v == 1) {
            v8e_put(e, 0, pr[2]);
        } else {
            v8e_put(e, 1, pr[2]);
            if (v <= 4) {
                v8e_put(e, 0, pr[3]);
                if (v == 2) {
                    v8e_put(e, 0, pr[4]);
                } else {
                    v8e_put(e, 1, pr[4]);
                    v8e_put(e, v - 3, pr[5]);
                }
            } else {
                v8e_put(e, 1, pr[3]);
                if (v <= 6) {
                    v8e_put(e, 0, pr[6]); v8e_put(e, 0, pr[7]);
                    v8e_put(e, v - 5, 159);
                } else if (v <= 10) {
                    v8e_put(e, 0, pr[6]); v8e_put(e, 1, pr[7]);
                    v8e_put(e, (v - 7) >> 1, 165); v8e_put(e, (v - 7) & 1, 145);
                } else {
                    const int cat = v <= 18 ? 0 : v <= 34 ? 1 : v <= 66 ? 2 : 3; /* cat3 .. cat6 */
                    v8e_put(e, 1, pr[6]);
                    v8e_put(e, cat >> 1, pr[8]);
                    v8e_put(e, cat & 1, pr[9 + (cat >> 1)]);
                    const int nb = v8e_cat_bits[cat], x = v - v8e_cat_base[cat];
                    for (int k = 0; k < nb; k++) v8e_put(e, (x >> (nb - 1 - k)) & 1, v8e_pcat[cat][k]);
                }
            }
        }
        v8e_put(e, c < 0, 128);
        prev_zero = 0; ctx = v == 1 ? 1 : 2;
    }
}

/* block b's context: the non-zero flags of the block above and the block to the left, from the masks of this macroblock, the one above
 * and the one to the left (0 beyond the picture: a skipped macroblock's mask is 0 as well, and every macroblock has a Y2 block) */
V8E_FN int v8e_ctx(int b, uint32_t m, uint32_t ma, uint32_t ml)
{
    if (b == 24) return (int)(((ma >> 24) & 1) + ((ml >> 24) & 1));
    if (b < 16) {
        const int bx = b & 3, by = b >> 2;
        return (int)(((by ? m >> (b - 4) : ma >> (12 + bx)) & 1) + ((bx ? m >> (b - 1) : ml >> (b + 3)) & 1));
    }
    const int base = b < 20 ? 16 : 20, bx = b & 1, by = (b >> 1) & 1;
    return (int)(((by ? m >> (b - 2) : ma >> (base + 2 + bx)) & 1) + ((bx ? m >> (b - 1) : ml >> (base + 2 * by + 1)) & 1));
}

/* token partition `part` of `parts`: the rows part, part + parts, ..; into out[] (v8e_part_bound of its macroblocks at least) -> its size */
V8E_FN uint64_t v8e_token_partition(const v8e_pic *p, int part, int parts, uint8_t *out)
{
    v8e_bool e;
    v8e_bool_init(&e, out);
    for (int y = part; y < p->rows; y += parts)
        for (int x = 0; x < p->cols; x++) {
            const int64_t mb = (int64_t)y * p->cols + x;
            const uint32_t m = p->mask[mb];
            if (!m) continue;
            const uint32_t ma = y ? p->mask[mb - p->cols] : 0, ml = x ? p->mask[mb - 1] : 0;
            const int16_t *lv = p->levels + mb * 400;
            v8e_put_block(&e, lv + 24 * 16, 1, 0, v8e_ctx(24, m, ma, ml));
            for (int b = 0; b < 16; b++) v8e_put_block(&e, lv + b * 16, 0, 1, v8e_ctx(b, m, ma, ml));
            for (int b = 16; b < 24; b++) v8e_put_block(&e, lv + b * 16, 2, 0, v8e_ctx(b, m, ma, ml));
        }
    return v8e_flush(&e);
}

/* ---------------------------------------------------------------------------------------------------------------- FILE */
typedef struct v8e_file {
    uint64_t file_len;   /* set by v8e_file_plan */
    int32_t status;
    int32_t parts;
    uint32_t p0, part[8]; /* the partitions' sizes */
    uint8_t head[30], sizes[22];
} v8e_file;

V8E_FN void v8e_le(uint8_t *o, uint32_t v, int n)
{
    for (int k = 0; k < n; k++) o[k] = (uint8_t)(v >> (8 * k));
}
/* from the sizes: the verdict on the partitions, the head, the size table, the file's length */
V8E_FN void v8e_file_plan(v8e_file *f, int width, int height)
{
    uint64_t chunk = 10 + (uint64_t)f->p0 + 3 * (uint64_t)(f->parts - 1);
    f->status = f->p0 > V8E_P0_MAX ? FFHIP_EVP8_PARTITION : FFHIP_OK;
    f->sizes[21] = 0;
    for (int k = 0; k < f->parts; k++) {
        chunk += f->part[k];
        if (f->part[k] > V8E_PART_MAX) f->status = FFHIP_EVP8_PARTITION;
        if (k < f->parts - 1) v8e_le(f->sizes + 3 * k, f->part[k], 3);
    }
    const uint8_t tags[13] = "RIFFWEBPVP8 ";
    for (int k = 0; k < 4; k++) { f->head[k] = tags[k]; f->head[8 + k] = tags[4 + k]; f->head[12 + k] = tags[8 + k]; }
    v8e_le(f->head + 4, (uint32_t)(12 + chunk + (chunk & 1)), 4);
    v8e_le(f->head + 16, (uint32_t)chunk, 4);
    v8e_le(f->head + 20, f->p0 << 5 | 1 << 4, 3); /* key frame, version 0, shown */
    f->head[23] = 0x9d; f->head[24] = 0x01; f->head[25] = 0x2a;
    v8e_le(f->head + 26, (uint32_t)width, 2); /* scale 0 */
    v8e_le(f->head + 28, (uint32_t)height, 2);
    f->file_len = 20 + chunk + (chunk & 1);
}
/* where partition k's bytes lie behind `base`: the first partition, then the token partitions, each with its bound's room rounded to 16 */
V8E_FN uint64_t v8e_part_room(uint64_t n_mb) { return (v8e_part_bound(n_mb) + 15) & ~(uint64_t)15; }
V8E_FN uint64_t v8e_p0_room(uint64_t n_mb) { return (v8e_p0_bound(n_mb) + 15) & ~(uint64_t)15; }
V8E_FN uint64_t v8e_part_at(int k, int cols, int rows, int parts)
{
    uint64_t at = v8e_p0_room((uint64_t)cols * rows);
    for (int j = 0; j < k; j++) at += v8e_part_room((uint64_t)cols * v8e_part_rows(rows, parts, j));
    return at;
}
/* the file's bytes [from, to) into out[], to <= file_len; lanes lane, lane + nl, .. */
V8E_FN void v8e_file_copy(const v8e_file *f, const uint8_t *base, int cols, int rows, uint8_t *out, uint64_t from, uint64_t to, int lane, int nl)
{
    uint64_t seg0 = 0;
    for (int k = 0; k < f->parts + 4; k++) {
        /* segments: the head, the first partition, the sizes, the token partitions, the padding byte */
        const uint8_t *src;
        uint64_t len;
        if (k == 0) { src = f->head; len = 30; }
        else if (k == 1) { src = base; len = f->p0; }
        else if (k == 2) { src = f->sizes; len = 3 * (uint64_t)(f->parts - 1); }
        else if (k < f->parts + 3) { src = base + v8e_part_at(k - 3, cols, rows, f->parts); len = f->part[k - 3]; }
        else { src = f->sizes + 21; len = f->file_len - seg0; } /* sizes[21] is 0 */
        const uint64_t a = from > seg0 ? from : seg0, b = to < seg0 + len ? to : seg0 + len;
        for (uint64_t o = a + (uint64_t)lane; o < b; o += (uint64_t)nl) out[o] = src[o - seg0];
        seg0 += len;
    }
}

#endif
