/*
 * ffhip_vp8_enc_gpu.hip -- the lossy WebP encoder on the device (include/ffpic_hip.h "Lossy WebP encoding").  The rule is
 * ffhip_vp8_enc_body.h's, shared with the host functions of ffhip_vp8_enc.c.
 *   k_items_tables2   (ffhip_items.h, twice) a workgroup per picture: its index over its ranges of the four per-workgroup tables
 *   k_vp8_enc_color   a thread per 2 x 2 cell of the macroblock grid: four luma samples, one U, one V into the padded source planes
 *   k_vp8_enc_mb      a wave per macroblock, one launch per anti-diagonal x + y = d of the part's largest grid: a picture has min(cols, rows)
 *                     workgroups in every launch, those beyond its diagonal's length leave at once.  v8e_mb with (lane, 64): the eight sums
 *                     of squared differences by a wave reduction, a block a lane for the 24 forward and the 24 inverse DCTs, the WHT pair on
 *                     lane 0 between them; levels, modes, the non-zero mask and the reconstruction go to scratch
 *   k_vp8_enc_parts   a lane per partition of a picture, the first partition included, V8_CODER_LANES lanes a workgroup: the lane tokenises
 *                     as it codes (v8e_first_partition, v8e_token_partition) into its partition's room in scratch
 *   k_vp8_enc_scan    a thread per picture: the sizes into the head and the size table, the file's length, the verdict
 *   k_vp8_enc_copy    a workgroup per 16 Ki pixels of the grid: its share of the file into the caller's buffer, every byte under cap
 * No kernel waits for another workgroup.  The host side is the encoders' common one: ffhip_parts_run, ffhip_items_run,
 * ffhip_lengths_read.
 */
#include "ffhip_items.h"
#include "ffhip_parts.h"
#include "ffhip_vp8_enc_internal.h"

#include <string.h>

#define V8_WG 256
#define V8_PART_ITEMS 4096  /* pictures of a part at most */
#define V8_CODER_LANES 1    /* of a workgroup of k_vp8_enc_parts: the coder's branches follow the data, lanes of one wave would wait for each other */
#define V8_COPY_PIXELS 16384
#define V8_SCRATCH_PER_PIXEL 32

namespace {

struct V8Desc {
    ffhip_jpeg_source src;
    v8e_pic pic;
    uint8_t *d_out, *parts_base; /* parts_base: the first partition, then the token partitions, v8e_part_at apart */
    unsigned long long cap;
    int32_t qi, filter, parts, pad;
    u32 color_first, color_n; /* workgroups of k_vp8_enc_color */
    u32 mb_first, mb_n;       /* of a launch of k_vp8_enc_mb: min(cols, rows) */
    u32 lane_first, lane_n;   /* lanes of k_vp8_enc_parts: parts + 1 */
    u32 copy_first, copy_n;
};
struct V8Args {
    const V8Desc *desc;
    const u32 *wg_item;
    v8e_file *file;
    u32 wg_base;
};

__global__ __launch_bounds__(V8_WG) void k_vp8_enc_color(V8Args a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const V8Desc &d = a.desc[item];
    const u32 cw = 8u * (u32)d.pic.cols, ch = 8u * (u32)d.pic.rows;
    const unsigned long long idx = (unsigned long long)(wg - d.color_first) * V8_WG + threadIdx.x;
    if (idx >= (unsigned long long)cw * ch) return; /* nothing is stored beyond the planes */
    const int cy = (int)(idx / cw), cx = (int)(idx - (unsigned long long)cy * cw);
    const ffhip_jpeg_source s = d.src;
    int u, v;
    v8e_chroma(&s, cx, cy, &u, &v);
    uint8_t *su = (uint8_t *)d.pic.su, *sv = (uint8_t *)d.pic.sv, *sy = (uint8_t *)d.pic.sy;
    su[(size_t)cy * cw + cx] = (uint8_t)u;
    sv[(size_t)cy * cw + cx] = (uint8_t)v;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = 2 * cx + (k & 1), y = 2 * cy + (k >> 1);
        sy[(size_t)y * 2 * cw + x] = (uint8_t)v8e_luma(&s, x, y);
    }
}

__global__ __launch_bounds__(64) void k_vp8_enc_mb(V8Args a, int diag)
{
    __shared__ v8e_mb_store m;
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const V8Desc &d = a.desc[item];
    const int cols = d.pic.cols, rows = d.pic.rows;
    if (diag >= cols + rows - 1) return;
    const int x_lo = diag - (rows - 1) > 0 ? diag - (rows - 1) : 0, x_hi = diag < cols - 1 ? diag : cols - 1;
    const int x = x_lo + (int)(wg - d.mb_first);
    if (x > x_hi) return; /* uniform over the workgroup: nobody waits at a barrier */
    const v8e_pic pic = d.pic;
    v8e_mb(&pic, &m, x, diag - x, (int)threadIdx.x, 64);
}

__global__ __launch_bounds__(V8_CODER_LANES) void k_vp8_enc_parts(V8Args a, unsigned long long lanes)
{
    const unsigned long long t = ((unsigned long long)a.wg_base + blockIdx.x) * V8_CODER_LANES + threadIdx.x;
    if (t >= lanes) return;
    const u32 item = a.wg_item[t];
    const V8Desc &d = a.desc[item];
    const int k = (int)((u32)t - d.lane_first);
    v8e_file &f = a.file[item];
    if (k == 0)
        f.p0 = (u32)v8e_first_partition(&d.pic, d.qi, d.filter, d.parts_base);
    else
        f.part[k - 1] = (u32)v8e_token_partition(&d.pic, k - 1, d.parts, d.parts_base + v8e_part_at(k - 1, d.pic.cols, d.pic.rows, d.parts));
}

__global__ __launch_bounds__(64) void k_vp8_enc_scan(V8Args a, int n)
{
    const int item = (int)(blockIdx.x * 64 + threadIdx.x);
    if (item >= n) return;
    const V8Desc &d = a.desc[item];
    v8e_file &f = a.file[item];
    f.parts = d.parts;
    v8e_file_plan(&f, d.src.width, d.src.height);
    if (f.status != FFHIP_OK) f.file_len = 0;
    else if (f.file_len > d.cap) f.status = FFHIP_EVP8_NOSPACE;
}

__global__ __launch_bounds__(V8_WG) void k_vp8_enc_copy(V8Args a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const V8Desc &d = a.desc[item];
    const v8e_file &f = a.file[item];
    const unsigned long long end = f.file_len < d.cap ? f.file_len : d.cap; /* 0 for a picture without a file */
    const unsigned long long share = (end + d.copy_n - 1) / d.copy_n, from = (unsigned long long)(wg - d.copy_first) * share;
    const unsigned long long to = from + share < end ? from + share : end;
    if (from < to) v8e_file_copy(&f, d.parts_base, d.pic.cols, d.pic.rows, d.d_out, from, to, (int)threadIdx.x, V8_WG);
}

bool item_ok(const ffhip_vp8_encode_item &it)
{
    return ffhip_vp8enc_source_ok(&it.src) && ffhip_vp8enc_params_ok(it.quality, it.filter) && !(it.cap && !it.d_out);
}

size_t grid_pixels(const ffhip_vp8_encode_item &it) { return (size_t)256 * (size_t)v8e_mb_cols(it.src.width) * (size_t)v8e_mb_cols(it.src.height); }

/* the pictures of one part: one synchronisation */
int encode_part(const ffhip_vp8_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<V8Desc> desc((size_t)n);
    std::vector<size_t> mb_at((size_t)n), parts_at((size_t)n);
    unsigned long long t_color = 0, t_mb = 0, t_lane = 0, t_copy = 0;
    size_t n_mbs = 0, parts_bytes = 0;
    int diags = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_vp8_encode_item &it = items[i];
        V8Desc &d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        const int cols = v8e_mb_cols(it.src.width), rows = v8e_mb_cols(it.src.height);
        const size_t mbs = (size_t)cols * rows;
        d.src = it.src; d.d_out = it.d_out; d.cap = it.cap;
        d.pic.cols = cols; d.pic.rows = rows;
        d.qi = ffhip_vp8_encode_quality_index(it.quality);
        d.filter = it.filter < 0 ? v8e_auto_filter(d.qi) : it.filter;
        d.parts = 1 << v8e_log2_parts(rows);
        ffhip_vp8enc_steps(d.qi, d.pic.q);
        d.color_first = (u32)t_color; d.color_n = (u32)((mbs * 64 + V8_WG - 1) / V8_WG);
        d.mb_first = (u32)t_mb; d.mb_n = (u32)(cols < rows ? cols : rows);
        d.lane_first = (u32)t_lane; d.lane_n = (u32)d.parts + 1;
        d.copy_first = (u32)t_copy; d.copy_n = (u32)((mbs * 256 + V8_COPY_PIXELS - 1) / V8_COPY_PIXELS);
        t_color += d.color_n; t_mb += d.mb_n; t_lane += d.lane_n; t_copy += d.copy_n;
        mb_at[(size_t)i] = n_mbs; n_mbs += mbs;
        parts_at[(size_t)i] = parts_bytes; parts_bytes += (size_t)v8e_part_at(d.parts, cols, rows, d.parts);
        if (cols + rows - 1 > diags) diags = cols + rows - 1;
    }
    if (t_color > 0xffffffffULL) return FFHIP_EINVAL;
    /* the scratch: the picture records (uploaded), the four tables, the files' records, the masks, the levels, the modes, the source planes
     * and the reconstruction, the partitions.  Every byte a kernel reads was written by a kernel of this call before it */
    const size_t up_bytes = (size_t)n * sizeof(V8Desc), table_words = (size_t)(t_color + t_mb + t_lane + t_copy);
    const size_t file_off = ffhip_up(up_bytes + table_words * 4, 8), mask_off = file_off + (size_t)n * sizeof(v8e_file);
    const size_t level_off = ffhip_up(mask_off + n_mbs * 4, 16), mode_off = level_off + n_mbs * 800, plane_off = ffhip_up(mode_off + n_mbs * 2, 16);
    const size_t parts_off = plane_off + n_mbs * 768, end = parts_off + parts_bytes;
    std::vector<uint8_t> upl(up_bytes);
    uint8_t *dev = nullptr;
    int rc = ffhip_items_stage(SCRATCH_VP8_ENC, stream, upl.data(), up_bytes, table_words, end - up_bytes - table_words * 4, &dev, [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            V8Desc &d = desc[(size_t)i];
            const size_t at = mb_at[(size_t)i], mbs = (size_t)d.pic.cols * d.pic.rows;
            uint8_t *planes = base + plane_off + at * 768;
            d.pic.mask = (uint32_t *)(base + mask_off) + at;
            d.pic.levels = (int16_t *)(base + level_off) + at * 400;
            d.pic.ymode = base + mode_off + at * 2; d.pic.uvmode = d.pic.ymode + mbs;
            d.pic.sy = planes; d.pic.su = planes + mbs * 256; d.pic.sv = planes + mbs * 320;
            d.pic.ry = planes + mbs * 384; d.pic.ru = planes + mbs * 640; d.pic.rv = planes + mbs * 704;
            d.parts_base = base + parts_off + parts_at[(size_t)i];
        }
        memcpy(upl.data(), desc.data(), up_bytes);
    });
    if (rc) return rc;
    V8Args a;
    a.desc = (const V8Desc *)dev; a.file = (v8e_file *)(dev + file_off); a.wg_base = 0;
    u32 *d_color = (u32 *)(dev + up_bytes), *d_mb = d_color + t_color, *d_lane = d_mb + t_mb, *d_copy = d_lane + t_lane;
    hipLaunchKernelGGL((k_items_tables2<V8Desc, V8Desc, &V8Desc::color_first, &V8Desc::color_n, &V8Desc::mb_first, &V8Desc::mb_n>), dim3((unsigned)n),
                       dim3(256), 0, st, a.desc, a.desc, d_color, d_mb);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    hipLaunchKernelGGL((k_items_tables2<V8Desc, V8Desc, &V8Desc::lane_first, &V8Desc::lane_n, &V8Desc::copy_first, &V8Desc::copy_n>), dim3((unsigned)n),
                       dim3(256), 0, st, a.desc, a.desc, d_lane, d_copy);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    a.wg_item = d_color;
    rc = ffhip_items_run(k_vp8_enc_color, t_color, V8_WG, stream, a);
    if (rc) return rc;
    a.wg_item = d_mb;
    for (int diag = 0; diag < diags; diag++) {
        rc = ffhip_items_run(k_vp8_enc_mb, t_mb, 64, stream, a, diag);
        if (rc) return rc;
    }
    a.wg_item = d_lane;
    rc = ffhip_items_run(k_vp8_enc_parts, (t_lane + V8_CODER_LANES - 1) / V8_CODER_LANES, V8_CODER_LANES, stream, a, t_lane);
    if (rc) return rc;
    a.wg_base = 0;
    hipLaunchKernelGGL(k_vp8_enc_scan, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a, n);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    a.wg_item = d_copy;
    rc = ffhip_items_run(k_vp8_enc_copy, t_copy, V8_WG, stream, a);
    if (rc) return rc;
    return ffhip_lengths_read(SCRATCH_VP8_ENC + 1, stream, a.file, n, len_out, status);
}

} // namespace

extern "C" int ffhip_vp8_encode_items(const ffhip_vp8_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!items || !len_out || !status))) return FFHIP_EINVAL;
    for (int i = 0; i < n; i++)
        if (!item_ok(items[i])) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(nullptr) / V8_SCRATCH_PER_PIXEL; /* a pixel of the macroblock grid takes 32 bytes of scratch at most */
    return ffhip_parts_run(n, budget, V8_PART_ITEMS, [&](int i) { return grid_pixels(items[i]); },
                           [&](int first, int cnt) { return encode_part(items + first, cnt, len_out + first, status + first, stream); });
}
