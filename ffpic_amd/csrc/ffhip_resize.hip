/*
 * ffhip_resize.hip -- BGRA rectangles of any sizes resized to BGRA pictures of any sizes in one call (ffhip_bgra_resize_items), by the
 * integer rule of include/ffpic_hip.h ("decoded pictures resized on the device").  The rule itself is in
 * ffhip_resize_body.h, shared with the host entry ffhip_resize_axis_taps.
 *
 * Two launches per call.  k_resize_tables writes, per item and axis, the run (first, count) and the 12-bit weights of every output index
 * and the per-workgroup item table.  k_bgra_resize then has one workgroup per (item, output row, tile of 256 output columns): for every
 * source row of the output row's vertical run it stages the tile's horizontal footprint through LDS (dword loads of consecutive lanes, in
 * chunks of FFHIP_RESIZE_LDS_PIXELS), every lane reduces the taps of its own output column per channel (at most 255 x 4096), and the row's
 * sum goes into the lane's four accumulators times the row's weight: sum_y qy (sum_x qx v) is the rule's double sum exactly, below 2^32.
 * No intermediate picture goes to memory; a source row is read once per output row whose run holds it (about twice when shrinking).
 */
#include "ffhip_items.h"
#include "ffhip_alpha_body.h"
#include "ffhip_resize_body.h"

#include <string.h>

#define FFHIP_RESIZE_LDS_PIXELS 4096 /* 16 KiB: a 3840-wide row in one piece, and 8 workgroups on a CU */
/* the pictures' pointers come out of a record: said to be global here, they get global loads and stores instead of flat ones */
#define RESIZE_GLOBAL __attribute__((address_space(1)))

namespace {

struct ResizeArgs {
    const ResizeItemDesc *desc;
    const uint8_t *tables; /* the scratch the records' table offsets count from */
    const u32 *wg_item;    /* per workgroup of the call: its item */
    u32 wg_base;           /* the launch's first workgroup */
};

/* workgroup 2 i + a: the tables of axis a (0: x, 1: y) of item i, one output index per thread and pass; the x one also the item's range
 * of the per-workgroup table */
__global__ __launch_bounds__(256) void k_resize_tables(const ResizeItemDesc *desc, uint8_t *tables, u32 *wg_item, int filter)
{
    const u32 item = blockIdx.x >> 1, axis = blockIdx.x & 1;
    const ResizeItemDesc d = desc[item];
    const u32 n_in = (u32)(axis ? d.height : d.width), n_out = (u32)(axis ? d.out_height : d.out_width);
    u32 *fc = (u32 *)(tables + (axis ? d.fcy : d.fcx));
    uint16_t *q = (uint16_t *)(tables + (axis ? d.qy : d.qx));
    for (u32 o = threadIdx.x; o < n_out; o += 256) {
        const ResizeRun t = resize_axis_run(n_in, n_out, filter, o);
        fc[o] = t.first | t.count << 16;
        resize_axis_weights(t, n_out, [&](u32 j, u32 w) { q[j * n_out + o] = (uint16_t)w; });
    }
    if (axis == 0)
        for (u32 k = threadIdx.x; k < d.n_wgs; k += 256) wg_item[d.first_wg + k] = item;
}

/* PREMUL: every pixel is premultiplied as it is staged (once per staged pixel, not per tap): the filter runs over premultiplied bytes and
 * the output is premultiplied BGRA (ffhip_bgra_resize_items_premultiplied) */
template <bool PREMUL> __device__ __forceinline__ void bgra_resize_wg(ResizeArgs a)
{
    __shared__ u32 row[FFHIP_RESIZE_LDS_PIXELS];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const ResizeItemDesc d = a.desc[item];
    const u32 local = wg - d.first_wg, oy = local / d.tiles_x, tile = local - oy * d.tiles_x;
    const u32 out_w = (u32)d.out_width, out_h = (u32)d.out_height;
    const u32 *fcx = (const u32 *)(a.tables + d.fcx), *fcy = (const u32 *)(a.tables + d.fcy);
    const uint16_t *qx = (const uint16_t *)(a.tables + d.qx), *qy = (const uint16_t *)(a.tables + d.qy);
    /* the tile's columns ox0 .. ox1 and their footprint seg0 .. seg1 - 1 of the source row: first and first + count both grow with the column */
    const u32 ox0 = tile * FFHIP_RESIZE_WG_THREADS, ox1 = (ox0 + FFHIP_RESIZE_WG_THREADS < out_w ? ox0 + FFHIP_RESIZE_WG_THREADS : out_w) - 1u;
    const u32 lo = fcx[ox0], hi = fcx[ox1], run_y = fcy[oy];
    const u32 seg0 = lo & 0xffffu, seg1 = (hi & 0xffffu) + (hi >> 16);
    const u32 fy = run_y & 0xffffu, cy = run_y >> 16;
    const u32 ox = ox0 + threadIdx.x;
    const bool active = ox <= ox1;
    u32 fx = seg0, cx = 0;
    if (active) { const u32 v = fcx[ox]; fx = v & 0xffffu; cx = v >> 16; }
    u32 acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    for (u32 ty = 0; ty < cy; ty++) {
        const u32 wy = qy[ty * out_h + oy];
        const RESIZE_GLOBAL u32 *src = (const RESIZE_GLOBAL u32 *)(d.src + (long long)(fy + ty) * d.src_pitch);
        u32 h0 = 0, h1 = 0, h2 = 0, h3 = 0;
        for (u32 c0 = seg0; c0 < seg1; c0 += FFHIP_RESIZE_LDS_PIXELS) {
            const u32 len = seg1 - c0 < FFHIP_RESIZE_LDS_PIXELS ? seg1 - c0 : FFHIP_RESIZE_LDS_PIXELS;
            for (u32 i = threadIdx.x; i < len; i += FFHIP_RESIZE_WG_THREADS) row[i] = resize_staged<PREMUL>(src[c0 + i]);
            __syncthreads();
            /* the lane's taps that lie in this chunk: pixels max(fx, c0) .. min(fx + cx, c0 + len) - 1 */
            const u32 j_lo = c0 > fx ? c0 - fx : 0u;
            const u32 j_hi = c0 + len > fx ? (c0 + len - fx < cx ? c0 + len - fx : cx) : 0u;
            for (u32 j = j_lo; j < j_hi; j++) {
                const u32 w = qx[j * out_w + ox];
                const u32 v = row[fx + j - c0];
                h0 += w * (v & 0xffu);
                h1 += w * ((v >> 8) & 0xffu);
                h2 += w * ((v >> 16) & 0xffu);
                h3 += w * (v >> 24);
            }
            __syncthreads();
        }
        acc0 += wy * h0; acc1 += wy * h1; acc2 += wy * h2; acc3 += wy * h3;
    }
    if (active) {
        const u32 px = ((acc0 + (1u << 23)) >> 24) | ((acc1 + (1u << 23)) >> 24) << 8 | ((acc2 + (1u << 23)) >> 24) << 16 | ((acc3 + (1u << 23)) >> 24) << 24;
        *(RESIZE_GLOBAL u32 *)(d.dst + (long long)oy * d.dst_pitch + 4ll * ox) = px;
    }
}

__global__ __launch_bounds__(FFHIP_RESIZE_WG_THREADS) void k_bgra_resize(ResizeArgs a)
{
    bgra_resize_wg<false>(a);
}

__global__ __launch_bounds__(FFHIP_RESIZE_WG_THREADS) void k_bgra_resize_premultiplied(ResizeArgs a)
{
    bgra_resize_wg<true>(a);
}

bool side_ok(long long v) { return v >= 1 && v <= FFHIP_RESIZE_MAX_SIDE; }

/* an item the call takes; fills its record (first_wg and the table offsets aside) */
bool resize_item_desc(const ffhip_resize_item &it, ResizeItemDesc *out)
{
    if (!side_ok(it.width) || !side_ok(it.height) || !side_ok(it.out_width) || !side_ok(it.out_height) || it.x0 < 0 || it.y0 < 0) return false;
    if (!it.d_src || ((uintptr_t)it.d_src & 3) || it.src_pitch < 4 || (it.src_pitch & 3)) return false;
    /* as ffhip_tensor_item: the rectangle within the pitch, source offsets within 31 bits */
    if (4LL * ((long long)it.x0 + it.width) > it.src_pitch || ((long long)it.y0 + it.height) * it.src_pitch > 0x7fffffffLL) return false;
    if (!it.d_dst || ((uintptr_t)it.d_dst & 3) || (it.dst_pitch & 3) || it.dst_pitch < 4LL * it.out_width) return false;
    if (it.dst_pitch > ((long long)1 << 40)) return false; /* row offsets are 64-bit in the kernel: 2^14 rows stay far inside */
    memset(out, 0, sizeof(*out));
    out->src = it.d_src + (long long)it.y0 * it.src_pitch + 4LL * it.x0;
    out->dst = it.d_dst;
    out->src_pitch = it.src_pitch;
    out->dst_pitch = it.dst_pitch;
    out->width = it.width; out->height = it.height;
    out->out_width = it.out_width; out->out_height = it.out_height;
    out->tiles_x = (u32)((it.out_width + FFHIP_RESIZE_WG_THREADS - 1) / FFHIP_RESIZE_WG_THREADS);
    out->n_wgs = out->tiles_x * (u32)it.out_height;
    return true;
}

} // namespace

extern "C" int ffhip_resize_axis_taps(int n_in, int n_out, int filter, int o, int *first, uint16_t *q, int cap)
{
    if (!side_ok(n_in) || !side_ok(n_out) || (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS)) return FFHIP_EINVAL;
    if (o < 0 || o >= n_out || !first || cap < 0 || (cap > 0 && !q)) return FFHIP_EINVAL;
    const ResizeRun t = resize_axis_run((u32)n_in, (u32)n_out, filter, (u32)o);
    *first = (int)t.first;
    resize_axis_weights(t, (u32)n_out, [&](u32 j, u32 w) { if (j < (u32)cap) q[j] = (uint16_t)w; });
    return (int)t.count;
}

namespace {

int resize_items(const ffhip_resize_item *items, int n, int filter, bool premultiply, void *stream)
{
    if (n < 0 || n > 0x3fffffff || (n > 0 && !items) || (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* the records: every item's workgroups behind those of the items before it, its four tables behind theirs */
    std::vector<ResizeItemDesc> desc((size_t)n);
    const size_t desc_bytes = (size_t)n * sizeof(ResizeItemDesc);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (!resize_item_desc(items[i], &desc[(size_t)i])) return FFHIP_EINVAL;
        desc[(size_t)i].first_wg = (u32)total;
        total += desc[(size_t)i].n_wgs;
    }
    if (total > 0xffffffffULL) return FFHIP_EINVAL; /* the table's entries are 32-bit workgroup indices */
    size_t at = (desc_bytes + 4 * (size_t)total + 15) & ~(size_t)15;
    for (int i = 0; i < n; i++) {
        ResizeItemDesc &d = desc[(size_t)i];
        const size_t taps_x = resize_axis_max_taps((u32)d.width, (u32)d.out_width, filter), taps_y = resize_axis_max_taps((u32)d.height, (u32)d.out_height, filter);
        d.fcx = (long long)at; at += 4 * (size_t)d.out_width;
        d.fcy = (long long)at; at += 4 * (size_t)d.out_height;
        d.qx = (long long)at; at += (2 * taps_x * (size_t)d.out_width + 3) & ~(size_t)3;
        d.qy = (long long)at; at += (2 * taps_y * (size_t)d.out_height + 3) & ~(size_t)3;
    }
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    /* device scratch: the records, the per-workgroup table, the tap tables; pinned staging for the records.  Both per stream */
    uint8_t *dev = nullptr;
    const int rc = ffhip_items_stage(SCRATCH_RESIZE_ITEMS, stream, desc.data(), desc_bytes, (size_t)total, at - desc_bytes - 4 * (size_t)total, &dev);
    if (rc) return rc;
    const ResizeItemDesc *d_desc = (const ResizeItemDesc *)dev;
    u32 *d_table = (u32 *)(dev + desc_bytes);
    hipLaunchKernelGGL(k_resize_tables, dim3(2u * (unsigned)n), dim3(256), 0, st, d_desc, dev, d_table, filter);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        ResizeArgs a;
        a.desc = d_desc; a.tables = dev; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(premultiply ? k_bgra_resize_premultiplied : k_bgra_resize, dim3(grid_x), dim3(FFHIP_RESIZE_WG_THREADS), 0, st, a);
    });
}

} // namespace

extern "C" int ffhip_bgra_resize_items(const ffhip_resize_item *items, int n, int filter, void *stream)
{
    return resize_items(items, n, filter, false, stream);
}

extern "C" int ffhip_bgra_resize_items_premultiplied(const ffhip_resize_item *items, int n, int filter, void *stream)
{
    return resize_items(items, n, filter, true, stream);
}
