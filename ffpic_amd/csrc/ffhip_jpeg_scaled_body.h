/* ffhip_jpeg_scaled_body.h -- the block rule of the reduced-size JPEG reconstruction (include/ffpic_hip.h, "JPEG pictures at 1/2, 1/4 and
 * 1/8 size") and the record of an item of ffhip_jpeg_recon_items_scaled (ffhip_jpeg_scaled.hip).  Plain C++ without
 * builtins, __host__ too: ffhip_jpeg_scaled_block on the host and the kernel on the device run the same functions, and a CPU program can
 * hold them against the rule written another way.
 *
 * N = 8 / denominator is 4, 2 or 1.  A block gives N x N samples from its N x N leading coefficients, by the steps of the full-size path
 * (dequantise to int16, columns with + 1024 >> 11 to int16, rows with + (257 << 17) >> 18) with the N-point matrix T_N[x][u] =
 * round(8192 sqrt(2) alpha(u) cos((2 x + 1) u pi / 2 N)) in place of the 8-point one.
 * Every sum is int32 and none can leave it: the largest row of absolute values is T_4's, 8192 + 10703 + 8192 + 4433 = 31 520, its inputs are
 * int16, and 31 520 x 32 768 + (257 << 17) < 2^31.  A sample is at most (31 520 x 32 767 + (257 << 17)) >> 18 = 4068: the upper clamp of
 * the full-size path (65 535) cannot bind, only max(0, .) is kept, and the samples stay inside the range on which the colour conversion's
 * forms are defined. */
#ifndef FFHIP_JPEG_SCALED_BODY_H
#define FFHIP_JPEG_SCALED_BODY_H

#include <stdint.h>

#include "ffpic_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

/* T_N[x][u]; the loops over x and u below are unrolled, so that the entries become immediates on the device */
template <int N> __host__ __device__ inline int jpeg_scaled_basis(int x, int u)
{
    if (N == 1) return 8192;
    if (N == 2) return (x & u) ? -8192 : 8192;
    /* N == 4: column 0 is 8192, column 2 is 8192 x (+, -, -, +), columns 1 and 3 are 10703 / 4433 with the signs of the cosines */
    constexpr int t4[4][4] = {{8192, 10703, 8192, 4433}, {8192, 4433, -8192, -10703}, {8192, -4433, -8192, 10703}, {8192, -10703, 8192, -4433}};
    return t4[x & 3][u & 3];
}

/* step 1: the int16 store of format/jpg.c:251 */
__host__ __device__ inline int jpeg_scaled_dequant(int16_t coef, uint16_t quant) { return (int16_t)((int)coef * (int)quant); }

/* step 2 for ONE output row y of a block: c[u] = (int16)((sum_v T[y][v] F[v][u] + 1024) >> 11), F the dequantised N x N corner */
template <int N> __host__ __device__ inline void jpeg_scaled_columns(const int (&F)[N][N], int y, int (&c)[N])
{
#pragma unroll
    for (int u = 0; u < N; u++) {
        int sum = 1024;
#pragma unroll
        for (int v = 0; v < N; v++) {
            int t = 0; /* T[y][v] with y a run-time value: picked from the unrolled rows */
#pragma unroll
            for (int yy = 0; yy < N; yy++) t = y == yy ? jpeg_scaled_basis<N>(yy, v) : t;
            sum += t * F[v][u];
        }
        c[u] = (int16_t)(sum >> 11);
    }
}

/* step 3: s[x] = max(0, (sum_u T[x][u] c[u] + (257 << 17)) >> 18) */
template <int N> __host__ __device__ inline void jpeg_scaled_row(const int (&c)[N], int (&s)[N])
{
#pragma unroll
    for (int x = 0; x < N; x++) {
        int sum = 257 << 17;
#pragma unroll
        for (int u = 0; u < N; u++) sum += jpeg_scaled_basis<N>(x, u) * c[u];
        sum >>= 18;
        s[x] = sum < 0 ? 0 : sum;
    }
}

/* row y of a block's N x N samples from its coefficients and quantisers (64 each, natural order): only the N leading values of the N
 * leading rows are read */
template <int N> __host__ __device__ inline void jpeg_scaled_block_row(const int16_t *coef, const uint16_t *quant, int y, int (&s)[N])
{
    int F[N][N], c[N];
#pragma unroll
    for (int v = 0; v < N; v++)
#pragma unroll
        for (int u = 0; u < N; u++) F[v][u] = jpeg_scaled_dequant(coef[8 * v + u], quant[8 * v + u]);
    jpeg_scaled_columns<N>(F, y, c);
    jpeg_scaled_row<N>(c, s);
}

/* the last coefficient, in zig-zag order, that the transform at denominator d reads: the largest index of the leading 1 x 1, 2 x 2, 4 x 4
 * corner; a progressive file's scans that start behind it need not be decoded */
inline int jpeg_scaled_k_max(int d) { return d == 8 ? 0 : d == 4 ? 4 : d == 2 ? 24 : 63; }

/* the sizes of a picture at denominator d: ceil(W / d) x ceil(H / d) displayed; a rectangle of the full-size display picture mapped onto
 * it: x0' = x0 / d, x1' = min(ceil(W / d), ceil((x0 + w) / d)), likewise y -- its edges lie up to d - 1 source pixels outside the request */
__host__ __device__ inline bool jpeg_denom_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8; }
__host__ __device__ inline int jpeg_scaled_len(int n, int d) { return (int)(((long long)n + d - 1) / d); }
inline ffhip_rect jpeg_scaled_rect_of(int width, int height, int d, const ffhip_rect &r)
{
    const int x0 = r.x0 / d, y0 = r.y0 / d;
    int x1 = jpeg_scaled_len((int)((long long)r.x0 + r.width < 0x7fffffffLL ? r.x0 + r.width : 0x7fffffff), d);
    int y1 = jpeg_scaled_len((int)((long long)r.y0 + r.height < 0x7fffffffLL ? r.y0 + r.height : 0x7fffffff), d);
    if (x1 > jpeg_scaled_len(width, d)) x1 = jpeg_scaled_len(width, d);
    if (y1 > jpeg_scaled_len(height, d)) y1 = jpeg_scaled_len(height, d);
    return ffhip_rect{x0, y0, x1 - x0, y1 - y0};
}

/* One item of a call, as the kernel reads it.  A wave takes one picture row of one column chunk: FFHIP_JPEG_SCALED_WG_BLOCKS luma blocks
 * side by side, a lane the N pixels of its block's row.  The item's waves are numbered chunk-major, row fastest: the four waves of a
 * workgroup take four rows of one chunk, which share their blocks' coefficient lines. */
struct JpegScaledDesc { /* 96 bytes */
    const int16_t *coef_y, *coef_u, *coef_v;
    const uint16_t *quant;
    uint8_t *bgra;
    long long pitch;
    int mcu_cols, mcu_rows;
    int h_log2, v_log2;       /* the seven fused layouts have h, v in 1, 2, 4 */
    int ncomp, qt_y, qt_u, qt_v;
    uint32_t first_wg, n_wgs; /* the item's range of the per-workgroup table */
    uint32_t rows, n_waves;   /* N v mcu_rows picture rows; rows x column chunks */
};
static_assert(sizeof(JpegScaledDesc) == 96, "JpegScaledDesc layout");

#endif
