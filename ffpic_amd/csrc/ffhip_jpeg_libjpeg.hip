/*
 * ffhip_jpeg_libjpeg.hip -- JPEG reconstruction to the pixels libjpeg gives: int32 dequantisation, the "islow" inverse DCT,
 * "fancy" chroma upsampling over the component's real sample grid and the JFIF matrix in 16-bit fixed point.  The rule is
 * ffhip_jpeg_libjpeg_body.h's, shared by the host functions and the kernels below.
 *
 * TWO kernels, because the upsampling reads chroma samples of the neighbouring blocks and MCUs on every side:
 *   k_jpeg_idct_islow      a thread takes one 8 x 8 block of any component: 8 x 16-byte loads, both passes in registers, 8 x 8-byte stores
 *                          into the component's RASTER uint8 plane (the lanes of a wave take neighbouring blocks of a block row: a wave's
 *                          stores of one sample row are one run of 512 bytes)
 *   k_jpeg_upsample_color  a thread takes 8 pixels of two rows (a pair lies over one chroma row of the vertical ratio 2): 8 luma bytes a row,
 *                          the chroma samples under them with one neighbour on each side (and the same of the row above or below for the
 *                          vertical ratio 2), two 16-byte stores a row; the lanes of a wave take neighbouring units: 2 KiB of a row
 * The planes of all items lie back to back in the call's scratch; h, v and the component count come from the item's record, so every layout
 * class is one code path and a mixed batch is one pair of launches (behind the records' upload and the per-workgroup tables' kernel, as in
 * ffhip_jpeg_recon_items).
 */
#include "ffhip_items.h"
#include "ffhip_jpeg_libjpeg_body.h"

#include <string.h>

#define LJ_WG_THREADS 256
/* The planes, coefficients and pictures are global memory; a pointer read out of a record is generic to the compiler, and a generic load is a
 * flat one (it waits on both counters and is decoded for three address spaces).  G(T): T in global memory */
#define G(T) __attribute__((address_space(1))) T

namespace {

struct JpegLibjpegArgs {
    const JpegLibjpegDesc *desc;
    const u32 *wg_item; /* per workgroup of the call (of this kernel): its item */
    u32 wg_base;        /* the launch's first workgroup */
};

/* one workgroup per item: the item's index over its ranges of the two per-workgroup tables */
__global__ __launch_bounds__(256) void k_jpeg_libjpeg_table(const JpegLibjpegDesc *desc, u32 *idct_item, u32 *color_item)
{
    const u32 item = blockIdx.x;
    const u32 f0 = desc[item].idct_first_wg, n0 = desc[item].idct_n_wgs, f1 = desc[item].color_first_wg, n1 = desc[item].color_n_wgs;
    for (u32 k = threadIdx.x; k < n0; k += 256) idct_item[f0 + k] = item;
    for (u32 k = threadIdx.x; k < n1; k += 256) color_item[f1 + k] = item;
}

__device__ __forceinline__ void unpack8(const u32x4 w, int (&out)[8])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        out[2 * k] = (int)(w[k] & 0xffffu);
        out[2 * k + 1] = (int)(w[k] >> 16);
    }
}

__global__ __launch_bounds__(LJ_WG_THREADS) void k_jpeg_idct_islow(JpegLibjpegArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JpegLibjpegDesc &d = a.desc[item];
    const u32 local = wg - d.idct_first_wg;
    /* the workgroup's component: luma, then Cb, then Cr (grey: wg_u = wg_v = idct_n_wgs) */
    const int comp = local >= d.wg_v ? 2 : (local >= d.wg_u ? 1 : 0);
    const u32 first = comp == 2 ? d.wg_v : (comp == 1 ? d.wg_u : 0u);
    const int hs = comp ? 0 : d.h_log2, vs = comp ? 0 : d.v_log2;
    const u32 bw = (u32)d.mcu_cols << hs, bh = (u32)d.mcu_rows << vs; /* the component's blocks across and down */
    const u32 b = (local - first) * LJ_WG_THREADS + threadIdx.x;      /* the thread's block, raster order */
    if (b >= bw * bh) return;
    const u32 by = b / bw, bx = b - by * bw;
    const long long mcu = (long long)(by >> vs) * d.mcu_cols + (bx >> hs);
    const long long blk = (mcu << (hs + vs)) + (long long)(((by & ((1u << vs) - 1u)) << hs) + (bx & ((1u << hs) - 1u)));
    G(const int16_t) *coef = (G(const int16_t) *)(comp == 2 ? d.coef_v : (comp == 1 ? d.coef_u : d.coef_y)) + blk * 64;
    G(const uint16_t) *quant = (G(const uint16_t) *)d.quant + (comp == 2 ? d.qt_v : (comp == 1 ? d.qt_u : d.qt_y)) * 64;
    int32_t c[8][8];
#pragma unroll
    for (int v = 0; v < 8; v++) {
        int cf[8], qf[8];
        unpack8(*(G(const u32x4) *)(coef + 8 * v), cf);
        unpack8(*(G(const u32x4) *)(quant + 8 * v), qf);
#pragma unroll
        for (int u = 0; u < 8; u++) c[v][u] = jl_dequant((int16_t)cf[u], (uint16_t)qf[u]);
    }
    int s[8][8];
    jl_idct_block(c, s);
    G(uint8_t) *plane = (G(uint8_t) *)(comp == 2 ? d.plane_v : (comp == 1 ? d.plane_u : d.plane_y));
    const long long stride = (long long)bw * 8;
    G(uint8_t) *dst = plane + (long long)by * 8 * stride + (long long)bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        u32x2 w;
        w[0] = (u32)s[y][0] | ((u32)s[y][1] << 8) | ((u32)s[y][2] << 16) | ((u32)s[y][3] << 24);
        w[1] = (u32)s[y][4] | ((u32)s[y][5] << 8) | ((u32)s[y][6] << 16) | ((u32)s[y][7] << 24);
        *(G(u32x2) *)(dst + y * stride) = w;
    }
}

__device__ __forceinline__ void bytes8(const u32x2 w, int (&out)[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

/* the samples i0 - 1 .. i0 + 4 of a chroma row (i0 a multiple of 4), an index outside 0 .. e being the edge sample: t[k] = p[clamp(i0 - 1 + k)].
 * Every address read lies inside the coded row of `cw` samples: i0 + 3 does by the caller's geometry, and the two neighbours are read at
 * max(i0 - 1, 0) and min(i0 + 4, cw - 1) by EVERY lane and picked afterwards -- a load under a lane's condition would be a branch with its
 * own wait, eight of them in a row for a 4:2:0 unit. */
__device__ __forceinline__ void chroma_row6(G(const uint8_t) *row, int i0, int e, int cw, int (&t)[6])
{
    const u32 w = *(G(const u32) *)(row + i0);
    const int left = row[i0 > 0 ? i0 - 1 : 0], right = row[i0 + 4 < cw ? i0 + 4 : cw - 1];
    const int m = e - i0 < 0 ? 0 : (e - i0 > 3 ? 3 : e - i0); /* the last sample of the word inside the grid (a unit wholly outside it: unspecified pixels) */
#pragma unroll
    for (int k = 0; k < 4; k++) t[k + 1] = (int)((w >> (8 * (k < m ? k : m))) & 0xffu);
    t[0] = i0 > 0 ? left : t[1];
    t[5] = i0 + 4 <= e ? right : t[4];
}

/* the 8 chroma samples under the pixels x0 .. x0 + 7 of row y, upsampled by the item's ratio (step 4 of the rule) */
__device__ __forceinline__ void chroma8(G(const uint8_t) *plane, const JpegLibjpegDesc &d, u32 x0, u32 y, int (&c)[8])
{
    const int hs = d.h_log2, vs = d.v_log2;
    const long long cw = (long long)d.mcu_cols * 8;
    const int r = (int)(y >> vs), lower = (int)(y & 1u);
    int rn = r + (lower ? 1 : -1); /* the other row of the vertical ratio 2 */
    rn = rn < 0 ? 0 : (rn > d.dh_c - 1 ? d.dh_c - 1 : rn);
    G(const uint8_t) *row = plane + r * cw, *other = plane + rn * cw;
    if (hs == 0) {
        bytes8(*(G(const u32x2) *)(row + x0), c);
        if (vs == 1) {
            int o[8];
            bytes8(*(G(const u32x2) *)(other + x0), o);
#pragma unroll
            for (int k = 0; k < 8; k++) c[k] = jl_h1v2(c[k], o[k], lower);
        }
    } else if (hs == 1) {
        int t[6];
        chroma_row6(row, (int)(x0 >> 1), d.dw_c - 1, (int)cw, t);
        if (d.dw_c <= 2) { /* each sample twice, or 2 x 2 */
#pragma unroll
            for (int k = 0; k < 4; k++) c[2 * k] = c[2 * k + 1] = t[k + 1];
        } else if (vs == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) jl_h2v1_pair(t[k], t[k + 1], t[k + 2], &c[2 * k], &c[2 * k + 1]);
        } else {
            int o[6];
            chroma_row6(other, (int)(x0 >> 1), d.dw_c - 1, (int)cw, o);
#pragma unroll
            for (int k = 0; k < 6; k++) t[k] = jl_h2v2_sum(t[k], o[k]);
#pragma unroll
            for (int k = 0; k < 4; k++) jl_h2v2_pair(t[k], t[k + 1], t[k + 2], &c[2 * k], &c[2 * k + 1]);
        }
    } else { /* ratio (4, 1): each sample four times */
        const int p0 = row[x0 >> 2], p1 = row[(x0 >> 2) + 1];
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = k < 4 ? p0 : p1;
    }
}

__global__ __launch_bounds__(LJ_WG_THREADS) void k_jpeg_upsample_color(JpegLibjpegArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JpegLibjpegDesc &d = a.desc[item];
    const u32 upr = (u32)d.mcu_cols << d.h_log2;           /* units of 8 pixels across the coded picture */
    const u32 pairs = ((u32)d.mcu_rows << d.v_log2) * 4u;  /* pairs of coded rows */
    const u32 idx = (wg - d.color_first_wg) * LJ_WG_THREADS + threadIdx.x;
    if (idx >= upr * pairs) return; /* nothing is loaded or stored beyond the coded picture */
    const u32 yp = idx / upr, x0 = (idx - yp * upr) * 8u;
    /* both rows' pixels first, then the stores: the two rows of a pair lie over ONE chroma row of the vertical ratios 2 and 4, whose loads
     * and unpacking the compiler then makes once */
    u32 px[2][8];
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        const u32 y = 2u * yp + (u32)dy;
        int ys[8];
        bytes8(*(G(const u32x2) *)((G(const uint8_t) *)d.plane_y + (long long)y * ((long long)upr * 8) + x0), ys);
        if (d.ncomp == 3) {
            int cb[8], cr[8];
            chroma8((G(const uint8_t) *)d.plane_u, d, x0, y, cb);
            chroma8((G(const uint8_t) *)d.plane_v, d, x0, y, cr);
#pragma unroll
            for (int k = 0; k < 8; k++) px[dy][k] = jl_bgra(ys[k], cb[k], cr[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) px[dy][k] = jl_grey(ys[k]);
        }
    }
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        G(uint8_t) *dst = (G(uint8_t) *)d.bgra + (long long)(2u * yp + (u32)dy) * d.pitch + (long long)x0 * 4;
        *(G(u32x4) *)dst = (u32x4){px[dy][0], px[dy][1], px[dy][2], px[dy][3]};
        *(G(u32x4) *)(dst + 16) = (u32x4){px[dy][4], px[dy][5], px[dy][6], px[dy][7]};
    }
}

int log2_of(int x) { return x == 1 ? 0 : (x == 2 ? 1 : 2); }

/* geometry and display size: a layout ffhip_jpeg_recon_items takes, the size ending inside the last MCU column and row */
bool picture_ok(const ffhip_jpeg_geom *g, int width, int height)
{
    return jpeg_geom_class(g) >= 0 && jl_len_fits(width, g->h, g->mcu_cols) && jl_len_fits(height, g->v, g->mcu_rows);
}

/* step 4 on the host, sample by sample: the chroma value under pixel (x, y) from the component's raster plane (rows `cw` apart) */
int chroma_at(const uint8_t *plane, long long cw, int dw, int dh, int h, int v, int x, int y)
{
    const int i = x / h, r = y / v;
    const uint8_t *row = plane + r * cw;
    if (h == 4 || v == 4 || (h == 1 && v == 1) || (h == 2 && dw <= 2)) return row[i];
    const int lower = y & 1, odd = x & 1;
    int rn = r + (lower ? 1 : -1), prev = i - 1, next = i + 1;
    rn = rn < 0 ? 0 : (rn > dh - 1 ? dh - 1 : rn);
    prev = prev < 0 ? 0 : prev;
    next = next > dw - 1 ? dw - 1 : next;
    const uint8_t *other = plane + rn * cw;
    int even_out, odd_out;
    if (h == 1) return jl_h1v2(row[i], other[i], lower);
    if (v == 1) jl_h2v1_pair(row[prev], row[i], row[next], &even_out, &odd_out);
    else
        jl_h2v2_pair(jl_h2v2_sum(row[prev], other[prev]), jl_h2v2_sum(row[i], other[i]), jl_h2v2_sum(row[next], other[next]), &even_out, &odd_out);
    return odd ? odd_out : even_out;
}

/* steps 1 and 2 on the host: a component's MCU-order blocks into its raster plane */
void plane_host(const int16_t *coef, const uint16_t *quant, int mcu_cols, int mcu_rows, int h, int v, uint8_t *plane)
{
    const long long stride = 8LL * h * mcu_cols;
    for (long long my = 0; my < mcu_rows; my++)
        for (long long mx = 0; mx < mcu_cols; mx++)
            for (int vi = 0; vi < v; vi++)
                for (int hi = 0; hi < h; hi++) {
                    uint8_t s[64];
                    ffhip_jpeg_libjpeg_block(coef + (((my * mcu_cols + mx) * v + vi) * h + hi) * 64, quant, s);
                    uint8_t *dst = plane + (my * v + vi) * 8 * stride + (mx * h + hi) * 8;
                    for (int y = 0; y < 8; y++) memcpy(dst + y * stride, s + 8 * y, 8);
                }
}

} // namespace

/* ---- host only ---- */
extern "C" int ffhip_jpeg_libjpeg_block(const int16_t *coef, const uint16_t *quant, uint8_t *out)
{
    if (!coef || !quant || !out) return FFHIP_EINVAL;
    int32_t c[8][8];
    int s[8][8];
    for (int k = 0; k < 64; k++) c[k >> 3][k & 7] = jl_dequant(coef[k], quant[k]);
    jl_idct_block(c, s);
    for (int k = 0; k < 64; k++) out[k] = (uint8_t)s[k >> 3][k & 7];
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_libjpeg_picture(const ffhip_jpeg_geom *g, int width, int height, const int16_t *coef_y, const int16_t *coef_u,
                                          const int16_t *coef_v, const uint16_t *quant, uint8_t *bgra, int64_t pitch)
{
    if (!g || !picture_ok(g, width, height)) return FFHIP_EINVAL;
    if (!coef_y || !quant || !bgra || (g->ncomp == 3 && (!coef_u || !coef_v)) || pitch < 4LL * width) return FFHIP_EINVAL;
    const long long cw = 8LL * g->mcu_cols, chh = 8LL * g->mcu_rows, yw = cw * g->h;
    std::vector<uint8_t> py((size_t)(yw * chh * g->v)), pu, pv;
    plane_host(coef_y, quant + g->qt_id[0] * 64, g->mcu_cols, g->mcu_rows, g->h, g->v, py.data());
    if (g->ncomp == 3) {
        pu.resize((size_t)(cw * chh));
        pv.resize((size_t)(cw * chh));
        plane_host(coef_u, quant + g->qt_id[1] * 64, g->mcu_cols, g->mcu_rows, 1, 1, pu.data());
        plane_host(coef_v, quant + g->qt_id[2] * 64, g->mcu_cols, g->mcu_rows, 1, 1, pv.data());
    }
    const int dw = jl_grid_len(width, g->h), dh = jl_grid_len(height, g->v);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const int lum = py[(size_t)(y * yw + x)];
            const uint32_t px = g->ncomp == 3 ? jl_bgra(lum, chroma_at(pu.data(), cw, dw, dh, g->h, g->v, x, y), chroma_at(pv.data(), cw, dw, dh, g->h, g->v, x, y))
                                              : jl_grey(lum);
            uint8_t *dst = bgra + (long long)y * pitch + 4LL * x;
            dst[0] = (uint8_t)px; dst[1] = (uint8_t)(px >> 8); dst[2] = (uint8_t)(px >> 16); dst[3] = (uint8_t)(px >> 24);
        }
    return FFHIP_OK;
}

/* ---- the items call ---- */
bool jpeg_libjpeg_item_ok(const ffhip_jpeg_geom *g, int width, int height, const uint8_t *d_bgra, int64_t pitch)
{
    if (!g || !picture_ok(g, width, height)) return false;
    const long long yw = 8LL * g->h * g->mcu_cols, yh = 8LL * g->v * g->mcu_rows;
    if (!d_bgra || ((uintptr_t)d_bgra & 15) || pitch < 4 * yw || (pitch & 15)) return false;
    /* the kernels' 32-bit indices: units of 8 pixels and blocks of a picture; byte offsets are 64-bit */
    return yw <= (1 << 24) && yh <= (1 << 24) && yw / 8 * yh <= 0x7fffffffLL;
}

int jpeg_recon_items_libjpeg_impl(const ffhip_jpeg_item *items, const ffhip_size *display, int n, void *stream, int slot)
{
    if (n < 0 || (n > 0 && (!items || !display)) || slot < 0 || slot >= FFHIP_HUFF_PARTS) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* every check first; the records with their workgroup ranges and their planes' offsets in the scratch */
    std::vector<JpegLibjpegDesc> desc((size_t)n);
    std::vector<size_t> plane_at((size_t)n);
    unsigned long long total_idct = 0, total_color = 0;
    size_t plane_bytes = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_item &it = items[i];
        const ffhip_jpeg_geom &g = it.geom;
        if (!jpeg_libjpeg_item_ok(&g, display[i].width, display[i].height, it.d_bgra, it.pitch)) return FFHIP_EINVAL;
        if (!it.d_coef_y || !it.d_quant || (g.ncomp == 3 && (!it.d_coef_u || !it.d_coef_v))) return FFHIP_EINVAL;
        if (((uintptr_t)it.d_coef_y & 15) || ((uintptr_t)it.d_coef_u & 15) || ((uintptr_t)it.d_coef_v & 15) || ((uintptr_t)it.d_quant & 15)) return FFHIP_EINVAL;
        JpegLibjpegDesc &d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.coef_y = it.d_coef_y; d.coef_u = it.d_coef_u; d.coef_v = it.d_coef_v;
        d.quant = it.d_quant; d.bgra = it.d_bgra; d.pitch = it.pitch;
        d.mcu_cols = g.mcu_cols; d.mcu_rows = g.mcu_rows;
        d.h_log2 = log2_of(g.h); d.v_log2 = log2_of(g.v);
        d.ncomp = g.ncomp; d.qt_y = g.qt_id[0]; d.qt_u = g.ncomp == 3 ? g.qt_id[1] : 0; d.qt_v = g.ncomp == 3 ? g.qt_id[2] : 0;
        d.dw_c = jl_grid_len(display[i].width, g.h); d.dh_c = jl_grid_len(display[i].height, g.v);
        const unsigned long long mcus = (unsigned long long)g.mcu_cols * g.mcu_rows, yblocks = mcus * g.h * g.v;
        const u32 wy = (u32)((yblocks + LJ_WG_THREADS - 1) / LJ_WG_THREADS), wc = g.ncomp == 3 ? (u32)((mcus + LJ_WG_THREADS - 1) / LJ_WG_THREADS) : 0u;
        d.idct_first_wg = (u32)total_idct; d.idct_n_wgs = wy + 2 * wc; d.wg_u = wy; d.wg_v = wy + wc;
        d.color_first_wg = (u32)total_color; d.color_n_wgs = (u32)((yblocks * 4 + LJ_WG_THREADS - 1) / LJ_WG_THREADS); /* a thread: 8 pixels of two rows */
        total_idct += d.idct_n_wgs; total_color += d.color_n_wgs;
        plane_at[(size_t)i] = plane_bytes; /* multiples of 64 bytes */
        plane_bytes += (size_t)(yblocks + (g.ncomp == 3 ? 2 * mcus : 0)) * 64;
    }
    if (total_idct > 0xffffffffULL || total_color > 0xffffffffULL) return FFHIP_EINVAL; /* the tables' entries are 32-bit workgroup indices */
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    /* device scratch: the records, the two per-workgroup tables, the planes (256-byte aligned); pinned staging for the records.  Both per (stream, slot) */
    const size_t desc_bytes = (size_t)n * sizeof(JpegLibjpegDesc);
    const size_t table_words = (size_t)total_idct + (size_t)total_color;
    const size_t planes_off = (desc_bytes + table_words * 4 + 255) & ~(size_t)255;
    uint8_t *dev = nullptr;
    const int rc = ffhip_items_stage(SCRATCH_JPEG_LIBJPEG + slot, stream, desc.data(), desc_bytes, table_words,
                                     planes_off + plane_bytes - desc_bytes - table_words * 4, &dev, [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            JpegLibjpegDesc &d = desc[(size_t)i];
            const size_t mcus = (size_t)d.mcu_cols * d.mcu_rows;
            d.plane_y = base + planes_off + plane_at[(size_t)i];
            d.plane_u = d.ncomp == 3 ? d.plane_y + ((mcus * 64) << (d.h_log2 + d.v_log2)) : nullptr;
            d.plane_v = d.ncomp == 3 ? d.plane_u + mcus * 64 : nullptr;
        }
    });
    if (rc) return rc;
    const JpegLibjpegDesc *d_desc = (const JpegLibjpegDesc *)dev;
    u32 *d_idct = (u32 *)(dev + desc_bytes), *d_color = d_idct + total_idct;
    hipLaunchKernelGGL(k_jpeg_libjpeg_table, dim3((unsigned)n), dim3(256), 0, st, d_desc, d_idct, d_color);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    for (int pass = 0; pass < 2; pass++) {
        const int lrc = ffhip_items_launch(0, pass ? total_color : total_idct, [&](unsigned grid_x, u32 wg_base) {
            JpegLibjpegArgs a;
            a.desc = d_desc; a.wg_item = pass ? d_color : d_idct; a.wg_base = wg_base;
            if (pass) hipLaunchKernelGGL(k_jpeg_upsample_color, dim3(grid_x), dim3(LJ_WG_THREADS), 0, st, a);
            else hipLaunchKernelGGL(k_jpeg_idct_islow, dim3(grid_x), dim3(LJ_WG_THREADS), 0, st, a);
        });
        if (lrc) return lrc;
    }
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_recon_items_libjpeg(const ffhip_jpeg_item *items, const ffhip_size *display, int n, void *stream)
{
    return jpeg_recon_items_libjpeg_impl(items, display, n, stream, 0);
}
