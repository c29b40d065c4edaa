/*
 * ffhip_jpeg_scaled.hip -- JPEG reconstruction at 1/2, 1/4 and 1/8 size straight from the coefficients: an N-point
 * inverse DCT (N = 8 / denominator) over the N x N leading coefficients of every block gives the picture at N/8 size, as libjpeg's
 * scale_num / 8 and PIL's draft() do.  The block rule is ffhip_jpeg_scaled_body.h's; the colour conversion is the full-size path's
 * (utils/colorspace.c:148-164: chroma replicated h x v, the literal fp64 expressions of ffhip_colorterms.h).
 *
 * ONE kernel, templated on N only; h, v and the component count come from the item's record, so the seven fused layout classes of the
 * full-size path (4:2:0, 4:4:4, 4:2:2, 4:4:0, 4:1:1, its transpose, grey) are one code path.  A wave takes one picture row of one chunk of
 * 64 luma blocks: lane l the N pixels of row y of block l, so that the wave's stores are ONE contiguous run of 64 x 4 N bytes of that row
 * (16-, 8- or 4-byte stores).  A lane loads the N leading int16 of the N leading rows of its luma block and of the chroma blocks above it
 * (8, 4 or 2 bytes a row), runs the column pass for its own row only and the row pass: nothing is shared between lanes, there is no LDS
 * and no barrier.  The N lanes of the N rows of a block read the same N x N corner; they sit in the four waves of one workgroup and meet
 * in the cache.
 *
 * Items of any sizes, layouts, pitches and outputs go in one launch per denominator present, through a per-workgroup item table as in
 * ffhip_jpeg_recon_items.  Denominator 1 is not this file's: it is routed to ffhip_jpeg_recon_items and is byte-identical to it.
 *
 * This file must be compiled with -ffp-contract=off.
 */
#include "ffhip_colorterms.h"
#include "ffhip_items.h"
#include "ffhip_jpeg_scaled_body.h"

#include <string.h>

#define SCALED_WG_THREADS 256
#define SCALED_WAVES (SCALED_WG_THREADS / 64)
static_assert(FFHIP_JPEG_SCALED_WG_BLOCKS == 64, "a wave is one chunk wide");

namespace {

struct JpegScaledArgs {
    const JpegScaledDesc *desc;
    const u32 *wg_item; /* per workgroup of the call: its item */
    u32 wg_base;        /* the launch's first workgroup */
};

/* the N leading int16 of row v of a block, as one load of 2 N bytes */
template <int N> __device__ __forceinline__ void load_corner_row(const int16_t *blk, int v, int16_t (&out)[N])
{
    if constexpr (N == 4) {
        const u32x2 w = *(const u32x2 *)(blk + 8 * v);
        out[0] = (int16_t)(w[0] & 0xffffu); out[1] = (int16_t)(w[0] >> 16);
        out[2] = (int16_t)(w[1] & 0xffffu); out[3] = (int16_t)(w[1] >> 16);
    } else if constexpr (N == 2) {
        const u32 w = *(const u32 *)(blk + 8 * v);
        out[0] = (int16_t)(w & 0xffffu); out[1] = (int16_t)(w >> 16);
    } else {
        out[0] = blk[8 * v];
    }
}

/* row y of the N x N samples of block `blk` */
template <int N> __device__ __forceinline__ void block_row(const int16_t *blk, const uint16_t *quant, int y, int (&s)[N])
{
    int F[N][N], c[N];
#pragma unroll
    for (int v = 0; v < N; v++) {
        int16_t cf[N], qf[N];
        load_corner_row<N>(blk, v, cf);
        load_corner_row<N>((const int16_t *)quant, v, qf);
#pragma unroll
        for (int u = 0; u < N; u++) F[v][u] = jpeg_scaled_dequant(cf[u], (uint16_t)qf[u]);
    }
    jpeg_scaled_columns<N>(F, y, c);
    jpeg_scaled_row<N>(c, s);
}

template <int N> __global__ __launch_bounds__(SCALED_WG_THREADS) void k_jpeg_recon_scaled(JpegScaledArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JpegScaledDesc &d = a.desc[item];
    const u32 lane = threadIdx.x & 63;
    const u32 w = __builtin_amdgcn_readfirstlane((wg - d.first_wg) * SCALED_WAVES + (threadIdx.x >> 6)); /* the wave's unit: (chunk, row), row fastest */
    if (w >= d.n_waves) return;
    const u32 rows = d.rows, chunk = w / rows, row = w - chunk * rows;
    const int hs = d.h_log2, vs = d.v_log2, h = 1 << hs;
    const u32 bx = chunk * FFHIP_JPEG_SCALED_WG_BLOCKS + lane; /* the lane's luma block column */
    if (bx >= ((u32)d.mcu_cols << hs)) return;                 /* nothing is loaded or stored beyond the coded width */
    /* row -> MCU row, luma block row inside it, sample row inside the block; the chroma sample row above it */
    const u32 mcu_h = (u32)N << vs; /* rows of an MCU row */
    const u32 my = row / mcu_h, py = row - my * mcu_h;
    const u32 vi = py / N, y = py - vi * N, cy = py >> vs;
    const u32 mx = bx >> hs, hi = bx & (u32)(h - 1);
    const long long mcu = (long long)my * d.mcu_cols + mx;
    int sy[N];
    block_row<N>(d.coef_y + ((mcu << (hs + vs)) + (vi << hs) + hi) * 64, d.quant + d.qt_y * 64, (int)y, sy);
    int su[N], sv[N];
    if (d.ncomp == 3) {
        block_row<N>(d.coef_u + mcu * 64, d.quant + d.qt_u * 64, (int)cy, su);
        block_row<N>(d.coef_v + mcu * 64, d.quant + d.qt_v * 64, (int)cy, sv);
    } else { /* grey: U = V = 0 planes (format/jpg.c:501, 552-554), as the full-size path has them */
#pragma unroll
        for (int i = 0; i < N; i++) su[i] = sv[i] = 0;
    }
    u32 px[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        const u32 cx = (hi * N + (u32)i) >> hs; /* pixel x of the MCU -> its chroma sample (colorspace.c:148-150) */
        int uu = su[0], vv = sv[0];
#pragma unroll
        for (int k = 1; k < N; k++) { uu = cx == (u32)k ? su[k] : uu; vv = cx == (u32)k ? sv[k] : vv; }
        px[i] = ff_bgra_fp64(sy[i], (int16_t)(uu - 128), (int16_t)(vv - 128));
    }
    uint8_t *dst = d.bgra + (long long)row * d.pitch + (long long)bx * (4 * N);
    if constexpr (N == 4) *(u32x4 *)dst = (u32x4){px[0], px[1], px[2], px[3]};
    else if constexpr (N == 2) *(u32x2 *)dst = (u32x2){px[0], px[1]};
    else *(u32 *)dst = px[0];
}

int log2_of(int x) { return x == 1 ? 0 : (x == 2 ? 1 : 2); }

/* chunks of 64 luma blocks across a picture */
long long scaled_chunks(const ffhip_jpeg_geom &g)
{
    return ((long long)g.h * g.mcu_cols + FFHIP_JPEG_SCALED_WG_BLOCKS - 1) / FFHIP_JPEG_SCALED_WG_BLOCKS;
}

} // namespace

int jpeg_scaled_item_class(const ffhip_jpeg_geom *g, int denom, const uint8_t *d_bgra, int64_t pitch)
{
    if (denom != 2 && denom != 4 && denom != 8) return -1;
    const int c = jpeg_geom_class(g); /* the two-pass layouts are not part of the mixed path */
    if (c < 0) return -1;
    const int N = 8 / denom;
    const long long blocks_x = (long long)g->h * g->mcu_cols, width = N * blocks_x, rows = (long long)N * g->v * g->mcu_rows;
    if (!d_bgra || ((uintptr_t)d_bgra & 15) || pitch < 4 * width || (pitch & 15)) return -1;
    /* the kernel's 32-bit indices: block columns, rows, waves; byte offsets are 64-bit */
    if (blocks_x > 0x7fffffffLL / 8 || rows > 0x7fffffffLL / 8 || rows * scaled_chunks(*g) > 0x7fffffffLL) return -1;
    return c;
}

namespace {

/* an item at denominator d (2, 4, 8) the kernel takes; fills its record (first_wg aside) */
bool scaled_item_desc(const ffhip_jpeg_item &it, int d, JpegScaledDesc *out)
{
    const ffhip_jpeg_geom &g = it.geom;
    if (jpeg_scaled_item_class(&g, d, it.d_bgra, it.pitch) < 0) return false;
    if (!it.d_coef_y || !it.d_quant || (g.ncomp == 3 && (!it.d_coef_u || !it.d_coef_v))) return false;
    if (((uintptr_t)it.d_coef_y & 15) || ((uintptr_t)it.d_coef_u & 15) || ((uintptr_t)it.d_coef_v & 15) || ((uintptr_t)it.d_quant & 15)) return false;
    const long long rows = (long long)(8 / d) * g.v * g.mcu_rows, chunks = scaled_chunks(g);
    memset(out, 0, sizeof(*out));
    out->coef_y = it.d_coef_y; out->coef_u = it.d_coef_u; out->coef_v = it.d_coef_v;
    out->quant = it.d_quant; out->bgra = it.d_bgra; out->pitch = it.pitch;
    out->mcu_cols = g.mcu_cols; out->mcu_rows = g.mcu_rows;
    out->h_log2 = log2_of(g.h); out->v_log2 = log2_of(g.v);
    out->ncomp = g.ncomp; out->qt_y = g.qt_id[0]; out->qt_u = g.ncomp == 3 ? g.qt_id[1] : 0; out->qt_v = g.ncomp == 3 ? g.qt_id[2] : 0;
    out->rows = (uint32_t)rows;
    out->n_waves = (uint32_t)(rows * chunks);
    out->n_wgs = (uint32_t)((rows * chunks + SCALED_WAVES - 1) / SCALED_WAVES);
    return true;
}

template <int N> void block_host(const int16_t *coef, const uint16_t *quant, int16_t *out)
{
    for (int y = 0; y < N; y++) {
        int s[N];
        jpeg_scaled_block_row<N>(coef, quant, y, s);
        for (int x = 0; x < N; x++) out[y * N + x] = (int16_t)s[x];
    }
}

} // namespace

/* ---- host only ---- */
extern "C" int ffhip_jpeg_scaled_block(const int16_t *coef, const uint16_t *quant, int denom, int16_t *out)
{
    if (!coef || !quant || !out || !jpeg_denom_ok(denom)) return FFHIP_EINVAL;
    if (denom == 8) block_host<1>(coef, quant, out);
    else if (denom == 4) block_host<2>(coef, quant, out);
    else if (denom == 2) block_host<4>(coef, quant, out);
    else { /* the full-size rule is the 8 x 8 kernels' and the accelerator seam's: not restated here */
        return FFHIP_EINVAL;
    }
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_scaled_size(int width, int height, int denom, int *w, int *h)
{
    if (width < 1 || height < 1 || !jpeg_denom_ok(denom) || !w || !h) return FFHIP_EINVAL;
    *w = jpeg_scaled_len(width, denom);
    *h = jpeg_scaled_len(height, denom);
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_scaled_rect(int width, int height, int denom, const ffhip_rect *roi, ffhip_rect *out)
{
    if (width < 1 || height < 1 || !jpeg_denom_ok(denom) || !roi || !out) return FFHIP_EINVAL;
    if (roi->x0 < 0 || roi->y0 < 0 || roi->width < 1 || roi->height < 1 || (long long)roi->x0 + roi->width > width || (long long)roi->y0 + roi->height > height)
        return FFHIP_EINVAL;
    *out = jpeg_scaled_rect_of(width, height, denom, *roi);
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_scale_choose(int rect_w, int rect_h, int out_w, int out_h)
{
    if (rect_w < 1 || rect_h < 1 || out_w < 1 || out_h < 1) return FFHIP_EINVAL;
    for (int d = 8; d > 1; d >>= 1)
        if (jpeg_scaled_len(rect_w, d) >= out_w && jpeg_scaled_len(rect_h, d) >= out_h) return d;
    return 1;
}

extern "C" int ffhip_jpeg_scaled_wg_blocks(void) { return FFHIP_JPEG_SCALED_WG_BLOCKS; }

/* ---- the items call ---- */
int jpeg_recon_items_scaled_impl(const ffhip_jpeg_item *items, const int *denom, int n, void *stream, int slot)
{
    if (n < 0 || (n > 0 && (!items || !denom)) || slot < 0 || slot >= FFHIP_HUFF_PARTS) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* every check of the reduced items first: records in the order of the denominators 2, 4, 8, every item's workgroups behind those of
     * the items before it */
    std::vector<JpegScaledDesc> desc;
    std::vector<ffhip_jpeg_item> full;
    int count[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        if (!jpeg_denom_ok(denom[i])) return FFHIP_EINVAL;
        if (denom[i] == 1) full.push_back(items[i]);
        else count[denom[i] == 2 ? 0 : (denom[i] == 4 ? 1 : 2)]++;
    }
    const size_t n_scaled = (size_t)count[0] + count[1] + count[2];
    desc.resize(n_scaled);
    size_t at[3] = {0, (size_t)count[0], (size_t)count[0] + count[1]};
    for (int i = 0; i < n; i++) {
        if (denom[i] == 1) continue;
        const int k = denom[i] == 2 ? 0 : (denom[i] == 4 ? 1 : 2);
        if (!scaled_item_desc(items[i], denom[i], &desc[at[k]++])) return FFHIP_EINVAL;
    }
    unsigned long long total = 0, wg_first[4];
    for (size_t k = 0, c = 0; c < 3; c++) {
        wg_first[c] = total;
        for (int j = 0; j < count[c]; j++, k++) {
            desc[k].first_wg = (u32)total;
            total += desc[k].n_wgs;
        }
    }
    wg_first[3] = total;
    if (total > 0xffffffffULL) return FFHIP_EINVAL; /* the table's entries are 32-bit workgroup indices */
    /* denominator 1 is the full-size call's, byte for byte: it makes its own checks before it enqueues anything */
    if (!full.empty()) {
        const int rc = jpeg_recon_items_impl(full.data(), (int)full.size(), stream, slot);
        if (rc) return rc;
    }
    if (!n_scaled) return FFHIP_OK;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    const JpegScaledDesc *d_desc = nullptr;
    u32 *d_table = nullptr;
    const int rc = ffhip_items_upload(SCRATCH_JPEG_SCALED + slot, stream, desc, total, &d_desc, &d_table);
    if (rc) return rc;
    for (int c = 0; c < 3; c++) {
        const int lrc = ffhip_items_launch(wg_first[c], wg_first[c + 1], [&](unsigned grid_x, u32 wg_base) {
            JpegScaledArgs a;
            a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
            if (c == 0) hipLaunchKernelGGL(k_jpeg_recon_scaled<4>, dim3(grid_x), dim3(SCALED_WG_THREADS), 0, st, a);
            else if (c == 1) hipLaunchKernelGGL(k_jpeg_recon_scaled<2>, dim3(grid_x), dim3(SCALED_WG_THREADS), 0, st, a);
            else hipLaunchKernelGGL(k_jpeg_recon_scaled<1>, dim3(grid_x), dim3(SCALED_WG_THREADS), 0, st, a);
        });
        if (lrc) return lrc;
    }
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_recon_items_scaled(const ffhip_jpeg_item *items, const int *denom, int n, void *stream)
{
    return jpeg_recon_items_scaled_impl(items, denom, n, stream, 0);
}
