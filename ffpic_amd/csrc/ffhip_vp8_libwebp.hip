/*
 * ffhip_vp8_libwebp.hip -- the two stages of WEBP_RULE_LIBWEBP that are kernels of their own (include/ffpic_hip.h, "the second pixel rule";
 * DESIGN.md 4.21), on either side of k_vp8_frames_items' libwebp instances (ffhip_vp8_frame.hip).  The arithmetic of both is
 * ffhip_vp8_libwebp_body.h, which the host entries at the end of this file compile as well.
 *
 * k_vp8_residual_items_libwebp: dequantisation, inverse WHT and IDCT by RFC 6386 for the macroblocks of all items of a call end to end.  32 lanes
 * own a macroblock, lane b < 24 its block b: 32 bytes of levels in, 32 bytes of residual out per lane, the Y2 block read by the sixteen luma lanes
 * (each derives its own DC from it: a hundred integer operations, no LDS, no hand-off).  The stage also leaves the one bit the loop filter of
 * RFC 6386 needs per macroblock -- some block has a non-zero dequantised coefficient -- in byte [19] of the macroblock's mode record, which the
 * frame kernel fetches anyway.  A skipped macroblock's levels are zero, so its residual is zero and its bit clear without a look at the skip flag.
 *
 * k_vp8_upsample_color: the filtered planes to BGRA over the DISPLAY rectangle with libwebp's fancy upsampler and colour step.  It cannot be the
 * tail of the frame kernel: the upsampler of an odd picture row reads the chroma row BELOW it, and that row is final only after the next
 * macroblock row has been filtered.  1.5 bytes in, 4 out per pixel.  A wave takes a PAIR of picture rows 2p - 1 and 2p over 128
 * pixels: both rows read the chroma rows p - 1 and p (one as its nearer row, the other as its further one), so the pair shares its two chroma rows,
 * in the L1 of its CU.  Lanes 0..31 have the upper row, 32..63 the lower; a lane has four pixels: one dword of luma and two aligned dwords of each
 * chroma row of each plane in, 16 bytes out in one store.
 * A workgroup of four waves is four row pairs; one launch for a mixed batch through the items launcher (ffhip_items.h).
 */
#include "ffhip_items.h"
#include "ffhip_vp8_libwebp_body.h"

#include <string.h>
#include <vector>

/* ---- residual ---- */
__global__ __launch_bounds__(256) void k_vp8_residual_items_libwebp(const Vp8LwResItem *items, int n_items, long long n_mb_all)
{
    const int t = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long long gmb = (long long)blockIdx.x * 8 + slot;
    if (gmb >= n_mb_all) return; /* whole 32-lane slots */
    /* the slot's item: the last one whose first macroblock is not behind gmb (items[n_items].first is the total) */
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first <= gmb) lo = mid;
        else hi = mid - 1;
    }
    const Vp8LwResItem &d = items[lo];
    const long long mb = gmb - d.first;
    const uint8_t *info = d.info + mb * 32;
    const int has_y2 = info[25] != 0, seg = info[26] & 3;
    const uint16_t *q = d.quant + seg * 8;
    const int16_t *lv = d.levels + mb * 400;
    int nz = 0;
    if (t < 24) {
        int dc = 0;
        const int use_dc = has_y2 && t < 16;
        if (use_dc) dc = lw_y2_dc(lv + 384, q[2], q[3], t);
        int16_t res[16];
        nz = lw_block(lv + t * 16, lw_block_qdc(q, t), lw_block_qac(q, t), use_dc, dc, res);
        u32x4 o0, o1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            o0[k] = (u32)(uint16_t)res[2 * k] | (u32)(uint16_t)res[2 * k + 1] << 16;
            o1[k] = (u32)(uint16_t)res[8 + 2 * k] | (u32)(uint16_t)res[8 + 2 * k + 1] << 16;
        }
        u32x4 *dst = (u32x4 *)(d.out + mb * 384 + t * 16);
        dst[0] = o0;
        dst[1] = o1;
    }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(nz != 0);
    const u32 mine = (u32)(b >> (32 * (threadIdx.x >> 5 & 1)));
    if (t == 0) d.modes[mb * 20 + 19] = (uint8_t)(mine != 0u);
}

int vp8_libwebp_residual_items_enqueue(const Vp8LwResItem *d_items, int n, long long n_mb, void *stream)
{
    hipLaunchKernelGGL(k_vp8_residual_items_libwebp, dim3((unsigned)((n_mb + 7) / 8)), dim3(256), 0, (hipStream_t)stream, d_items, n, n_mb);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

/* ---- colour ---- */
namespace {

#define LW_TILE_W 128   /* pixels a wave's half covers: 32 lanes of four */
#define LW_WG_PAIRS 4   /* row pairs per workgroup: one per wave */

struct LwColorDesc {
    const uint8_t *y, *u, *v;
    uint8_t *bgra;
    long long pitch;
    int ys, uvs, width, height;
    u32 first_wg, n_wgs, tiles_x, pad_;
};

struct LwColorArgs {
    const LwColorDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
};

__global__ __launch_bounds__(64 * LW_WG_PAIRS) void k_vp8_upsample_color(LwColorArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const LwColorDesc d = a.desc[item];
    const u32 local = wg - d.first_wg, ty = local / d.tiles_x, tx = local - ty * d.tiles_x;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int pair = (int)ty * LW_WG_PAIRS + wave;    /* picture rows 2 * pair - 1 and 2 * pair */
    const int r = 2 * pair - 1 + (lane >> 5);
    const int x0 = (int)tx * LW_TILE_W + 4 * (lane & 31);
    if (r < 0 || r >= d.height || x0 >= d.width) return;
    const int ch = (d.height + 1) >> 1;
    const long long near = (long long)(r >> 1) * d.uvs, far = (long long)lw_far_row(r, ch) * d.uvs;
    const uint8_t *yrow = d.y + (long long)r * d.ys;
    uint8_t *dst = d.bgra + (long long)r * d.pitch + 4LL * x0;
    uint32_t px[4];
    if (x0 + 4 <= d.width) { /* the planes are 4-byte aligned with strides that are multiples of 4 */
        const u32 y4 = *(const u32 *)(yrow + x0);
        /* the chroma samples x0 / 2 - 1 .. x0 / 2 + 2 of a row start at an odd offset: the two aligned dwords round them, shifted.  (Sixteen
         * byte loads in their place held the kernel at a quarter of the planar colour kernel's rate.)  A dword left of the row or right of its
         * stride is replaced by a neighbour: its bytes stand for samples lw_upsample4 never looks at */
        const int c1 = (x0 >> 1) - 1, at = c1 & ~3, sh = 8 * (c1 - at);
        const int lo = at < 0 ? 0 : at, hi = at + 4 > d.uvs - 4 ? d.uvs - 4 : at + 4;
        auto window = [&](const uint8_t *row) {
            const unsigned long long w2 = (unsigned long long)*(const u32 *)(row + lo) | (unsigned long long)*(const u32 *)(row + hi) << 32;
            return (u32)(w2 >> sh);
        };
        lw_color_run4(y4, window(d.u + near), window(d.u + far), window(d.v + near), window(d.v + far), x0, d.width, px);
        *(u32x4 *)dst = u32x4{px[0], px[1], px[2], px[3]};
    } else { /* the last lane of a row whose width is no multiple of four */
        const int count = d.width - x0;
        lw_color_run(yrow + x0, d.u + near, d.u + far, d.v + near, d.v + far, x0, count, d.width, px);
        for (int k = 0; k < count; k++) ((u32 *)dst)[k] = px[k];
    }
}

bool lw_color_desc(const Vp8LwColorItem &it, LwColorDesc *out)
{
    if (it.width < 1 || it.height < 1 || it.width > 16384 || it.height > 16384) return false;
    if (!it.y || !it.u || !it.v || (((uintptr_t)it.y | (uintptr_t)it.u | (uintptr_t)it.v) & 3)) return false;
    if ((it.ys & 3) || (it.uvs & 3) || it.ys < ((it.width + 3) & ~3) || it.uvs < (it.width + 1) / 2) return false;
    if (!it.bgra || ((uintptr_t)it.bgra & 15) || (it.pitch & 15) || it.pitch < 4LL * it.width || it.pitch > 0x7fffffffLL) return false;
    memset(out, 0, sizeof(*out));
    out->y = it.y; out->u = it.u; out->v = it.v; out->bgra = it.bgra; out->pitch = it.pitch;
    out->ys = it.ys; out->uvs = it.uvs; out->width = it.width; out->height = it.height;
    out->tiles_x = (u32)((it.width + LW_TILE_W - 1) / LW_TILE_W);
    const int pairs = it.height / 2 + 1; /* rows -1|0, 1|2, ..: the last pair holds row height - 1 */
    out->n_wgs = out->tiles_x * (u32)((pairs + LW_WG_PAIRS - 1) / LW_WG_PAIRS);
    return true;
}

} // namespace

int vp8_libwebp_color_items(const Vp8LwColorItem *items, int n, void *stream)
{
    if (n < 0 || (n > 0 && !items)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    std::vector<LwColorDesc> desc((size_t)n);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (!lw_color_desc(items[i], &desc[(size_t)i])) return FFHIP_EINVAL;
        desc[(size_t)i].first_wg = (u32)total;
        total += desc[(size_t)i].n_wgs;
    }
    if (total > 0xffffffffULL) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    const LwColorDesc *d_desc = nullptr;
    u32 *d_table = nullptr;
    const int rc = ffhip_items_upload(SCRATCH_VP8_LIBWEBP, stream, desc, total, &d_desc, &d_table);
    if (rc) return rc;
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        LwColorArgs a;
        a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_vp8_upsample_color, dim3(grid_x), dim3(64 * LW_WG_PAIRS), 0, st, a);
    });
}

extern "C" int ffhip_debug_vp8_upsample_color(const uint8_t *d_y, const uint8_t *d_u, const uint8_t *d_v, int ys, int uvs, int width, int height,
                                              int n_images, int64_t plane_stride_y, int64_t plane_stride_uv, uint8_t *d_bgra, int64_t pitch,
                                              int64_t image_stride, void *stream)
{
    if (n_images < 0 || n_images > (1 << 20)) return FFHIP_EINVAL;
    std::vector<Vp8LwColorItem> items((size_t)n_images);
    for (int i = 0; i < n_images; i++)
        items[(size_t)i] = {d_y ? d_y + i * plane_stride_y : nullptr, d_u ? d_u + i * plane_stride_uv : nullptr, d_v ? d_v + i * plane_stride_uv : nullptr,
                            ys, uvs, width, height, d_bgra ? d_bgra + i * image_stride : nullptr, (long long)pitch};
    return vp8_libwebp_color_items(items.data(), n_images, stream);
}

/* ---- the host entries: the same bodies, no device ---- */
extern "C" int ffhip_vp8_libwebp_residual_mb(const int16_t *levels, int has_y2, const uint16_t *factors, int16_t *residual, int *any_nz)
{
    if (!levels || !factors || !residual || !any_nz) return FFHIP_EINVAL;
    int any = 0;
    for (int b = 0; b < 24; b++) {
        const int use_dc = has_y2 && b < 16;
        const int dc = use_dc ? lw_y2_dc(levels + 384, factors[2], factors[3], b) : 0;
        any |= lw_block(levels + 16 * b, lw_block_qdc(factors, b), lw_block_qac(factors, b), use_dc, dc, residual + 16 * b);
    }
    *any_nz = any;
    return FFHIP_OK;
}

extern "C" int ffhip_webp_libwebp_color(const uint8_t *y, int64_t ys, const uint8_t *u, const uint8_t *v, int64_t uvs, int width, int height,
                                        uint8_t *bgra, int64_t pitch)
{
    if (!y || !u || !v || !bgra || width < 1 || height < 1 || width > 16384 || height > 16384) return FFHIP_EINVAL;
    if (ys < width || uvs < (width + 1) / 2 || pitch < 4LL * width) return FFHIP_EINVAL;
    const int ch = (height + 1) >> 1;
    for (int r = 0; r < height; r++) {
        const int64_t near = (int64_t)(r >> 1) * uvs, far = (int64_t)lw_far_row(r, ch) * uvs;
        uint8_t *dst = bgra + (int64_t)r * pitch;
        for (int x0 = 0; x0 < width; x0 += 4) {
            uint32_t px[4];
            const int count = width - x0 < 4 ? width - x0 : 4, cw = (width + 1) / 2;
            const uint8_t *yr = y + (int64_t)r * ys + x0;
            if (count == 4) /* as the kernel's whole lanes */
                lw_color_run4((uint32_t)yr[0] | (uint32_t)yr[1] << 8 | (uint32_t)yr[2] << 16 | (uint32_t)yr[3] << 24, lw_window(u + near, x0, cw),
                              lw_window(u + far, x0, cw), lw_window(v + near, x0, cw), lw_window(v + far, x0, cw), x0, width, px);
            else lw_color_run(yr, u + near, u + far, v + near, v + far, x0, count, width, px);
            memcpy(dst + 4 * x0, px, 4 * (size_t)count);
        }
    }
    return FFHIP_OK;
}
