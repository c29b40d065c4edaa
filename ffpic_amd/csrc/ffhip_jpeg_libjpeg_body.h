/* ffhip_jpeg_libjpeg_body.h -- libjpeg's pixel rule (include/ffpic_hip.h, "JPEG pictures with libjpeg's pixels") and the record
 * of an item of ffhip_jpeg_recon_items_libjpeg (ffhip_jpeg_libjpeg.hip).  Plain C++ without builtins, __host__ too: the host functions
 * ffhip_jpeg_libjpeg_block / _picture and the two kernels run the same functions, and a CPU program can hold them against the rule written
 * another way.
 *
 * All arithmetic is 32-bit two's complement and wraps: sums, products and left shifts are made on uint32_t, so nothing is undefined for any
 * int16 coefficient and uint16 quantiser; every right shift is made on int32_t and is arithmetic.  The constants fit in 14 bits, but an
 * operand of the first pass is a full int32 (32 767 x 65 535 does not fit in 31 bits), so the products are plain 32-bit low products:
 * no 24-bit multiply form is exact over the range this header promises. */
#ifndef FFHIP_JPEG_LIBJPEG_BODY_H
#define FFHIP_JPEG_LIBJPEG_BODY_H

#include <stdint.h>

#include "ffpic_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

/* wrapping int32 arithmetic */
__host__ __device__ inline int32_t jl_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__host__ __device__ inline int32_t jl_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
__host__ __device__ inline int32_t jl_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
__host__ __device__ inline int32_t jl_shl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }
/* DESCALE(x, n) = (x + (1 << (n - 1))) >> n */
__host__ __device__ inline int32_t jl_descale(int32_t x, int n) { return jl_add(x, (int32_t)1 << (n - 1)) >> n; }
__host__ __device__ inline int jl_clamp255(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

/* step 1 */
__host__ __device__ inline int32_t jl_dequant(int16_t coef, uint16_t quant) { return jl_mul((int32_t)coef, (int32_t)quant); }

/* step 2: one 1-D pass over v[0..7] with the final shift S (11 for the columns, 18 for the rows).  The constants are 8192 x 0.298631336,
 * 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602, 1.501321110, 1.847759065, 1.961570560, 2.053119869, 2.562915447,
 * 3.072711026 */
template <int S> __host__ __device__ inline void jl_idct_pass(const int32_t (&v)[8], int32_t (&out)[8])
{
    int32_t z1 = jl_mul(jl_add(v[2], v[6]), 4433);
    const int32_t t2 = jl_sub(z1, jl_mul(v[6], 15137)), t3 = jl_add(z1, jl_mul(v[2], 6270));
    const int32_t t0 = jl_shl(jl_add(v[0], v[4]), 13), t1 = jl_shl(jl_sub(v[0], v[4]), 13);
    const int32_t t10 = jl_add(t0, t3), t13 = jl_sub(t0, t3), t11 = jl_add(t1, t2), t12 = jl_sub(t1, t2);
    int32_t a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = jl_add(a0, a3);
    int32_t z2 = jl_add(a1, a2), z3 = jl_add(a0, a2), z4 = jl_add(a1, a3);
    const int32_t z5 = jl_mul(jl_add(z3, z4), 9633);
    a0 = jl_mul(a0, 2446); a1 = jl_mul(a1, 16819); a2 = jl_mul(a2, 25172); a3 = jl_mul(a3, 12299);
    z1 = jl_mul(z1, -7373); z2 = jl_mul(z2, -20995);
    z3 = jl_add(jl_mul(z3, -16069), z5); z4 = jl_add(jl_mul(z4, -3196), z5);
    a0 = jl_add(a0, jl_add(z1, z3)); a1 = jl_add(a1, jl_add(z2, z4));
    a2 = jl_add(a2, jl_add(z2, z3)); a3 = jl_add(a3, jl_add(z1, z4));
    out[0] = jl_descale(jl_add(t10, a3), S); out[7] = jl_descale(jl_sub(t10, a3), S);
    out[1] = jl_descale(jl_add(t11, a2), S); out[6] = jl_descale(jl_sub(t11, a2), S);
    out[2] = jl_descale(jl_add(t12, a1), S); out[5] = jl_descale(jl_sub(t12, a1), S);
    out[3] = jl_descale(jl_add(t13, a0), S); out[4] = jl_descale(jl_sub(t13, a0), S);
}

/* steps 1 and 2 for a block: c[v][u] the dequantised coefficients (row v, column u) in, s[y][x] the samples 0..255 out.  libjpeg's
 * zero-column and zero-row shortcuts give the values of the full passes and are not taken: a lane of a wave would wait for its neighbours'
 * full passes anyway. */
__host__ __device__ inline void jl_idct_block(const int32_t (&c)[8][8], int (&s)[8][8])
{
    int32_t ws[8][8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        int32_t col[8], o[8];
#pragma unroll
        for (int v = 0; v < 8; v++) col[v] = c[v][u];
        jl_idct_pass<11>(col, o);
#pragma unroll
        for (int v = 0; v < 8; v++) ws[v][u] = o[v];
    }
#pragma unroll
    for (int y = 0; y < 8; y++) {
        int32_t o[8];
        jl_idct_pass<18>(ws[y], o);
#pragma unroll
        for (int x = 0; x < 8; x++) s[y][x] = jl_clamp255(jl_add(o[x], 128));
    }
}

/* step 4, for one output sample or sample pair given its neighbours (a neighbour outside the component's real grid is the edge sample itself:
 * the caller's business).
 * ratio (2, 1): the outputs 2 i and 2 i + 1 of p[i] with p[i - 1] and p[i + 1] */
__host__ __device__ inline void jl_h2v1_pair(int prev, int p, int next, int *even, int *odd)
{
    *even = (3 * p + prev + 1) >> 2;
    *odd = (3 * p + next + 2) >> 2;
}
/* ratio (1, 2): the upper (lower = 0; `other` is the sample above) or lower (lower = 1; the sample below) output row of p */
__host__ __device__ inline int jl_h1v2(int p, int other, int lower) { return (3 * p + other + 1 + lower) >> 2; }
/* ratio (2, 2): the column sum s = 3 p[r][i] + p[r -+ 1][i] of an output row, and the outputs 2 i and 2 i + 1 of s[i] with s[i - 1], s[i + 1] */
__host__ __device__ inline int jl_h2v2_sum(int p, int other) { return 3 * p + other; }
__host__ __device__ inline void jl_h2v2_pair(int sprev, int s, int snext, int *even, int *odd)
{
    *even = (3 * s + sprev + 8) >> 4;
    *odd = (3 * s + snext + 7) >> 4;
}

/* step 5: B, G, R, 0xFF.  The three samples are 0 .. 255 by construction (a clamped IDCT output, or a rounded mean of such); the masks say so
 * to the compiler, which then takes the 24-bit multiply-adds, four times the rate of a 32-bit product on the device */
__host__ __device__ inline uint32_t jl_bgra(int y_sample, int cb_sample, int cr_sample)
{
    const int32_t y = y_sample & 255, cb = (cb_sample & 255) - 128, cr = (cr_sample & 255) - 128;
    const int r = jl_clamp255(y + ((91881 * cr + 32768) >> 16));
    const int b = jl_clamp255(y + ((116130 * cb + 32768) >> 16));
    const int g = jl_clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16) | 0xff000000u;
}
__host__ __device__ inline uint32_t jl_grey(int y) { return (uint32_t)y * 0x010101u | 0xff000000u; }

/* step 3: a display length n against the component's sampling: ceil(n x f / f_max) with f_max / f = ratio = 1, 2 or 4 */
__host__ __device__ inline int jl_grid_len(int n, int ratio) { return (int)(((long long)n + ratio - 1) / ratio); }
/* a display length fits `blocks` luma blocks: it ends inside the last MCU (of f luma blocks) */
__host__ __device__ inline bool jl_len_fits(int n, int f, int mcus) { return n >= 1 && (long long)n <= 8LL * f * mcus && (long long)n > 8LL * f * (mcus - 1); }

/* One item of a call, as the two kernels read it.  The sample planes are raster, uint8, of the component's CODED size (luma 8 h mcu_cols x
 * 8 v mcu_rows, chroma 8 mcu_cols x 8 mcu_rows), in the call's scratch.
 * k_jpeg_idct_islow: a thread takes one block; the item's workgroups (256 blocks each) cover the luma blocks, then Cb's, then Cr's, each
 * component from a workgroup of its own on (wg_u, wg_v: the first workgroup of Cb and of Cr inside the item).
 * k_jpeg_upsample_color: a thread takes 8 pixels of two rows; the item's workgroups cover (rows / 2) x (coded width / 8) such units, row-major. */
struct JpegLibjpegDesc { /* 144 bytes */
    const int16_t *coef_y, *coef_u, *coef_v;
    const uint16_t *quant;
    uint8_t *bgra;
    uint8_t *plane_y, *plane_u, *plane_v;
    long long pitch;
    int mcu_cols, mcu_rows;
    int h_log2, v_log2; /* luma sampling = the chroma upsampling ratio: 1, 2 or 4 each */
    int ncomp, qt_y, qt_u, qt_v;
    int dw_c, dh_c;     /* the chroma components' real sample grid */
    uint32_t idct_first_wg, idct_n_wgs, wg_u, wg_v;
    uint32_t color_first_wg, color_n_wgs;
    uint32_t pad[2];
};
static_assert(sizeof(JpegLibjpegDesc) == 144, "JpegLibjpegDesc layout");

#endif
