/*
 * ffhip_orient.hip -- BGRA rectangles of any sizes turned upright by their EXIF orientations in one call (ffhip_bgra_orient_items;
 * include/ffpic_hip.h, "EXIF orientation").  Pure pixel movement, one dword per pixel.  The coordinate map, the layout of
 * the work and the LDS bank arithmetic are in ffhip_orient_body.h.
 *
 * Two launches per call: k_items_table (ffhip_items.h) writes the per-workgroup item table, k_bgra_orient has one workgroup of 256 threads per
 * 64 x 64 tile of an item's stored rectangle.  The orientation comes out of the item's record, so the branch on it is uniform over the
 * workgroup (the barrier of the transposing branch included), and so is the one on "the whole tile lies inside".  Every lane loads its 16
 * pixels before it stores the first: the loads of a wave are all in flight together, whatever the compiler may assume about source and
 * destination; in a whole tile no branch stands between the stores either.
 */
#include "ffhip_items.h"
#include "ffhip_orient_body.h"

#include <string.h>

namespace {

struct OrientArgs {
    const OrientItemDesc *desc;
    const u32 *wg_item; /* per workgroup of the call: its item */
    u32 wg_base;        /* the launch's first workgroup */
};

/* One tile.  FULL: all 64 x 64 pixels of it lie inside the rectangle, and nothing is predicated: 16 loads, then 16 stores, no branch
 * between them.  Otherwise (the tiles along the right and the lower edge) every load and store has its lane's condition */
template <bool FULL> __device__ __forceinline__ void orient_move_tile(const OrientItemDesc &d, const OrientTile &t, u32 *tile, int wave, int lane)
{
    constexpr int WAVES = FFHIP_ORIENT_WG_THREADS / 64;
    u32 v[FFHIP_ORIENT_ROWS_PER_WAVE];
    if (!FFHIP_ORIENT_TRANSPOSE(d.orientation)) {
#pragma unroll
        for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++) {
            int c, r;
            const bool in = orient_straight_source(d, t, lane, k * WAVES + wave, &c, &r);
            v[k] = FULL || in ? orient_load(d, t, c, r) : 0u;
        }
#pragma unroll
        for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++)
            if (FULL || (lane < t.uw && k * WAVES + wave < t.uh)) orient_store(d, t, lane, k * WAVES + wave, v[k]);
        return;
    }
#pragma unroll
    for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++) {
        const int row = k * WAVES + wave;
        v[k] = FULL || (lane < t.tw && row < t.th) ? orient_load(d, t, lane, row) : 0u;
    }
#pragma unroll
    for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++) tile[(k * WAVES + wave) * FFHIP_ORIENT_LDS_PITCH + lane] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++) {
        int at;
        const bool in = orient_transposed_source(d, t, lane, k * WAVES + wave, &at);
        v[k] = FULL || in ? tile[at] : 0u;
    }
#pragma unroll
    for (int k = 0; k < FFHIP_ORIENT_ROWS_PER_WAVE; k++)
        if (FULL || (lane < t.uw && k * WAVES + wave < t.uh)) orient_store(d, t, lane, k * WAVES + wave, v[k]);
}

__global__ __launch_bounds__(FFHIP_ORIENT_WG_THREADS) void k_bgra_orient(OrientArgs a)
{
    __shared__ u32 tile[FFHIP_ORIENT_TILE * FFHIP_ORIENT_LDS_PITCH];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const OrientItemDesc d = a.desc[item];
    const u32 local = wg - d.first_wg, ty = local / d.tiles_x, tx = local - ty * d.tiles_x;
    const OrientTile t = orient_tile(d, tx, ty);
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (t.tw == FFHIP_ORIENT_TILE && t.th == FFHIP_ORIENT_TILE) orient_move_tile<true>(d, t, tile, wave, lane);
    else orient_move_tile<false>(d, t, tile, wave, lane);
}

/* an item the call takes; fills its record (first_wg aside) */
bool orient_item_desc(const ffhip_orient_item &it, OrientItemDesc *out)
{
    if (it.orientation < 1 || it.orientation > 8) return false;
    if (it.width < 1 || it.height < 1 || it.x0 < 0 || it.y0 < 0) return false;
    if (!it.d_src || ((uintptr_t)it.d_src & 3) || it.src_pitch < 4 || (it.src_pitch & 3)) return false;
    /* as ffhip_tensor_item: the rectangle within the pitch, source offsets within 31 bits */
    if (4LL * ((long long)it.x0 + it.width) > it.src_pitch || ((long long)it.y0 + it.height) * it.src_pitch > 0x7fffffffLL) return false;
    const int uw = FFHIP_ORIENT_TRANSPOSE(it.orientation) ? it.height : it.width;
    if (!it.d_dst || ((uintptr_t)it.d_dst & 3) || (it.dst_pitch & 3) || it.dst_pitch < 4LL * uw) return false;
    if (it.dst_pitch > ((long long)1 << 32)) return false; /* row offsets are 64-bit in the kernel: below 2^29 rows (the source's bound) stay inside */
    memset(out, 0, sizeof(*out));
    out->src = it.d_src + (long long)it.y0 * it.src_pitch + 4LL * it.x0;
    out->dst = it.d_dst;
    out->src_pitch = it.src_pitch;
    out->dst_pitch = it.dst_pitch;
    out->ws = it.width; out->hs = it.height;
    out->orientation = it.orientation;
    out->tiles_x = (u32)((it.width + FFHIP_ORIENT_TILE - 1) / FFHIP_ORIENT_TILE);
    out->n_wgs = out->tiles_x * (u32)((it.height + FFHIP_ORIENT_TILE - 1) / FFHIP_ORIENT_TILE); /* width x height < 2^29: far below 2^32 tiles */
    return true;
}

} // namespace

extern "C" int ffhip_bgra_orient_items(const ffhip_orient_item *items, int n, void *stream)
{
    if (n < 0 || (n > 0 && !items)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* the records, every item's workgroups behind those of the items before it */
    std::vector<OrientItemDesc> desc((size_t)n);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (!orient_item_desc(items[i], &desc[(size_t)i])) return FFHIP_EINVAL;
        desc[(size_t)i].first_wg = (u32)total;
        total += desc[(size_t)i].n_wgs;
    }
    if (total > 0xffffffffULL) return FFHIP_EINVAL; /* the table's entries are 32-bit workgroup indices */
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    /* device scratch: the records, then the per-workgroup table; pinned staging for the records.  Both per stream */
    const OrientItemDesc *d_desc = nullptr;
    u32 *d_table = nullptr;
    const int rc = ffhip_items_upload(SCRATCH_ORIENT_ITEMS, stream, desc, total, &d_desc, &d_table);
    if (rc) return rc;
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        OrientArgs a;
        a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_bgra_orient, dim3(grid_x), dim3(FFHIP_ORIENT_WG_THREADS), 0, st, a);
    });
}
