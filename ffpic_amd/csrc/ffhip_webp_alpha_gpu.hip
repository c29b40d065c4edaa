/* ffhip_webp_alpha_gpu.hip -- the alpha plane of lossy WebP files into byte 3 of their pictures (include/ffpic_hip.h, "lossy WebP, the alpha
 * plane").  The stage runs behind the libwebp rule's back half of ffhip_webp_decode_files_device_ex, over the files with an
 * OK status and a plane, in parts of its own, driven through ffhip_staged.h: host threads copy a raw plane, or decode a lossless plane's
 * prefix codes (ffhip_vp8l.c), into pinned staging; one upload; the lossless planes go through k_vp8l_predict and k_vp8l_finish, unchanged,
 * into scratch BGRA pictures, where alpha is byte 1 of a pixel; k_webp_alpha_unfilter undoes the filter into a byte plane;
 * k_webp_alpha_merge writes byte 3 of the pictures.  Neither kernel has an error path: what a file is refused for is seen on the host.
 *
 * k_webp_alpha_unfilter, in the form of k_png_unfilter.  A file is cut into bands of 64 rows; a wave takes one band, lane r its row r.  A
 * row is walked in CHUNKS of 16 samples and the lanes are skewed by one chunk: at step t lane r reconstructs chunk t - r.  The chunk above
 * is what lane r - 1 produced one step earlier: four DPP wave_shr:1 moves; the left and the above-left of a chunk's first sample are
 * registers kept from the step before.  Lane 0 reads the chunk above from the band above's last row of the OUTPUT plane, which the launch
 * before has written: level l of every file is one launch, over records sorted by band count.  No spin-waits, counters or LDS.
 *   The chunk size, by the argument of ffhip_png_gpu.hip: at one byte a sample the widest single load and store is 16 samples, and with
 * every row of source and output padded to the chunk there is no partial chunk at all.  The skew costs 63 steps a band whatever the chunk,
 * so a larger chunk shortens a row's n_chunks steps and lengthens the share of the skew: a 1920-sample row is 120 steps + 63 at 16 samples
 * (34 % skew), 480 + 63 at four (12 %), 30 + 63 at 64.  A step's cost is the serial chain through `left` -- 16 dependent additions in the
 * horizontal arm, 16 clamped sums in the gradient arm -- plus one load and one store; the chain is the same per sample whatever the chunk,
 * the load and store are per chunk.  16 it is: the widest access the hardware has, 183 steps instead of 543 for that row, four registers
 * handed down.  A 64-sample chunk would need four loads, 16 moves and 64 samples' worth of live registers a step to save 90 of 183 steps.
 *   The filter is per file and so wave-uniform: one branch picks the horizontal, vertical or gradient arm.  Row 0 of a file takes the
 * horizontal arm under every filter -- lane 0 of band 0 alone leaves the wave's arm there.  The first sample of every later row predicts
 * from above, which the arms get from their starting registers (ffhip_webp_alpha_body.h).  The source is per record a byte plane (raw:
 * step 1) or a byte of a word picture (lossless: step 4), both with rows padded to whole chunks and 16-byte aligned; the output is a
 * byte plane whose pitch is a multiple of 16.  Files with filter 0 have no record.
 *
 * k_webp_alpha_merge.  Streaming: a lane owns four pixels of a row, loads their 16 bytes of BGRA and their four alpha samples -- from the
 * unfiltered plane, or for filter 0 straight from the source by the same pointer, pitch and step -- replaces byte 3 of each and makes one
 * 16-byte store.  A row's last partial group stores its alpha bytes one by one; nothing beside the width x height pixels is written. */
#include "ffhip_staged.h"
#include "ffhip_webp_alpha_internal.h"

#include <chrono>

namespace {

constexpr int ALPHA_BAND = 64;
constexpr int ALPHA_CHUNK = 16;
constexpr int ALPHA_MERGE_THREADS = FFHIP_GATHER_THREADS;

/* one file's stored plane: sample (x, y) is src[y * src_pitch + x * src_step] */
struct AlphaUnfDesc {
    const uint8_t *src;
    uint8_t *out; /* rows of out_pitch bytes */
    u32 src_pitch, src_step, out_pitch, width, rows, filter, n_bands;
};
struct AlphaUnfArgs {
    const AlphaUnfDesc *desc; /* sorted by n_bands, largest first: the items with a band `level` are the first of them */
    u32 level, wg_base;
};

/* one file's picture and its finished alpha samples */
struct AlphaMergeDesc {
    const uint8_t *src;
    uint8_t *dst;
    int64_t pitch;
    u32 src_pitch, src_step, width, height, groups_x;
    u32 first_wg, n_wgs;
};
struct AlphaMergeArgs {
    const AlphaMergeDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
};

/* four samples at p, one a byte: step 1 a dword of a byte plane (p 4-byte aligned), step 4 one byte of each of four words (the words 16-byte aligned) */
__device__ __forceinline__ u32 alpha_load4(const uint8_t *p, u32 step)
{
    if (step == 1) return *(const u32 *)p;
    const unsigned long long at = (unsigned long long)p;
    const u32 sh = 8u * (u32)(at & 3);
    const u32x4 v = *(const u32x4 *)(at & ~3ull);
    return ((v.x >> sh) & 255u) | ((v.y >> sh) & 255u) << 8 | ((v.z >> sh) & 255u) << 16 | ((v.w >> sh) & 255u) << 24;
}

/* a chunk: 16 samples */
__device__ __forceinline__ void alpha_load16(const uint8_t *p, u32 step, u32 (&w)[4])
{
    if (step == 1) {
        const u32x4 v = *(const u32x4 *)p;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = alpha_load4(p + 16 * k, step);
}

/* one chunk by arm MODE: a, c the left and above left of its first sample */
template <int MODE> __device__ __forceinline__ void alpha_chunk(const u32 (&raw)[4], const u32 (&up)[4], int a, int c, u32 (&out)[4])
{
    int o[ALPHA_CHUNK];
#pragma unroll
    for (int i = 0; i < ALPHA_CHUNK; i++) {
        const int b = byte_of(up, i);
        o[i] = ffhip_webp_alpha_sample(MODE, byte_of(raw, i), a, b, c);
        a = o[i];
        c = b;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = (u32)o[4 * k] | (u32)o[4 * k + 1] << 8 | (u32)o[4 * k + 2] << 16 | (u32)o[4 * k + 3] << 24;
}

/* One band.  Every lane runs every step, whatever its row: the cross-lane moves want the whole wave */
__global__ __launch_bounds__(ALPHA_BAND) void k_webp_alpha_unfilter(AlphaUnfArgs args)
{
    const AlphaUnfDesc d = args.desc[args.wg_base + blockIdx.x];
    const int lane = (int)threadIdx.x;
    const u32 band = args.level;
    const u32 row = band * ALPHA_BAND + (u32)lane;
    const bool live = row < d.rows;
    const uint8_t *in = d.src + (unsigned long long)(live ? row : 0) * d.src_pitch;
    uint8_t *cur = d.out + (unsigned long long)(live ? row : 0) * d.out_pitch;
    const uint8_t *above = band ? d.out + ((unsigned long long)band * ALPHA_BAND - 1) * d.out_pitch : nullptr; /* lane 0's row above */
    const u32 n_chunks = (d.width + ALPHA_CHUNK - 1) / ALPHA_CHUNK;
    const int mode = row ? (int)d.filter : FFHIP_WEBP_ALPHA_HORIZONTAL;
    u32 out[4] = {0, 0, 0, 0}; /* the lane's last chunk */
    int corner = 0;            /* the last sample of the chunk above it */
    for (u32 t = 0; t < n_chunks + ALPHA_BAND - 1; t++) {
        u32 up[4];
#pragma unroll
        for (int k = 0; k < 4; k++) up[k] = wave_shr1(out[k]);
        const u32 q = t - (u32)lane;
        if (!live || t < (u32)lane || q >= n_chunks) continue;
        if (lane == 0 && above) alpha_load16(above + (unsigned long long)q * ALPHA_CHUNK, 1, up);
        u32 raw[4];
        alpha_load16(in + (unsigned long long)q * ALPHA_CHUNK * d.src_step, d.src_step, raw);
        /* a row's first sample: 0 to its left in row 0, else the sample above on both sides */
        const int a = q ? (int)(out[3] >> 24) : row ? (int)(up[0] & 255u) : 0;
        const int c = q ? corner : a;
        corner = (int)(up[3] >> 24);
        if (mode == FFHIP_WEBP_ALPHA_HORIZONTAL) alpha_chunk<FFHIP_WEBP_ALPHA_HORIZONTAL>(raw, up, a, c, out);
        else if (mode == FFHIP_WEBP_ALPHA_VERTICAL) alpha_chunk<FFHIP_WEBP_ALPHA_VERTICAL>(raw, up, a, c, out);
        else alpha_chunk<FFHIP_WEBP_ALPHA_GRADIENT>(raw, up, a, c, out);
        *(u32x4 *)(cur + (unsigned long long)q * ALPHA_CHUNK) = u32x4{out[0], out[1], out[2], out[3]};
    }
}

__global__ __launch_bounds__(ALPHA_MERGE_THREADS) void k_webp_alpha_merge(AlphaMergeArgs args)
{
    const u32 wg = args.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(args.wg_item[wg]);
    const AlphaMergeDesc *d = args.desc + item;
    const u32 width = d->width, gx = d->groups_x;
    const u32 g = (wg - d->first_wg) * ALPHA_MERGE_THREADS + threadIdx.x; /* groups_x x height < 2^28 */
    if (g >= gx * d->height) return;
    const u32 y = g / gx, x0 = 4 * (g - y * gx);
    const u32 n = min(4u, width - x0);
    const u32 al = alpha_load4(d->src + (unsigned long long)y * d->src_pitch + (unsigned long long)x0 * d->src_step, d->src_step);
    uint8_t *out = d->dst + (long long)y * d->pitch + 4ll * x0;
    if (n == 4) {
        const u32x4 px = *(const u32x4 *)out;
        *(u32x4 *)out = u32x4{(px.x & 0xffffffu) | (al << 24), (px.y & 0xffffffu) | ((al >> 8) << 24), (px.z & 0xffffffu) | ((al >> 16) << 24),
                              (px.w & 0xffffffu) | ((al >> 24) << 24)};
    } else {
        for (u32 j = 0; j < n; j++) out[4 * j + 3] = (uint8_t)(al >> (8 * j));
    }
}

thread_local int t_alpha_last[4];     /* ffhip_debug_webp_alpha_last */
thread_local double t_alpha_times[4]; /* ffhip_debug_webp_alpha_times */

/* a file of the call with a plane */
struct AlphaFile {
    int i; /* its index in the call */
    ffhip_webp_alpha_head head;
};
/* its place in a part: a raw plane in the staging behind the lossless files' bytes, a lossless one as file `v` of the part's VP8L files;
 * in the part's work area its scratch picture (lossless) and its unfiltered plane (a filter) */
struct AlphaPartFile { int j, v; size_t raw_off, pic_off, out_off; };

size_t alpha_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
size_t alpha_plane_pitch(const ffhip_webp_alpha_head &h) { return alpha_up(h.width, ALPHA_CHUNK); }
size_t alpha_picture_pitch(const ffhip_webp_alpha_head &h) { return 4 * alpha_up(h.width, ALPHA_CHUNK); } /* a chunk of its samples is 64 bytes */

/* One part: `vbytes` of VP8L staging, the raw planes behind them, `work_bytes` of pictures and planes that stay on the device.  The clock
 * (FFHIP_WEBP_ALPHA_TIMES) stands around the upload with the lossless planes' two kernels, the unfilter launches and the merge launch */
int alpha_run_part(const std::vector<AlphaPartFile> &part, const std::vector<Vp8lPartFile> &vpart, size_t vbytes, size_t raw_bytes, size_t work_bytes,
                   const std::vector<AlphaFile> &af, const std::vector<ffhip_vp8l_file> &pf, std::vector<int> &st_a, std::vector<uint8_t *> &d_pic,
                   std::vector<int64_t> &pic_pitch, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch, void *stream, StageClock &clock)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = vbytes + raw_bytes;
    clock.mark_from(0, st);
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_WEBP_ALPHA, stream, bytes + 64);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_WEBP_ALPHA, stream, bytes / 4 + 16);
    uint8_t *work = (uint8_t *)ffhip_scratch(SCRATCH_WEBP_ALPHA + 3, stream, work_bytes / 4 + 16);
    if (!pin || !dev || !work) return FFHIP_ENOMEM;
    const auto t0 = std::chrono::steady_clock::now();
    ffhip_parallel_for((int)part.size(), n_threads, [&](int k) {
        const AlphaPartFile &p = part[(size_t)k];
        const ffhip_webp_alpha_head &h = af[(size_t)p.j].head;
        if (h.compression == 1) {
            st_a[(size_t)p.j] = vp8l_stage_file(pf[(size_t)p.j], vpart[(size_t)p.v], pin);
            return;
        }
        uint8_t *to = pin + vbytes + p.raw_off;
        const size_t pp = alpha_plane_pitch(h);
        for (u32 y = 0; y < h.height; y++) memcpy(to + y * pp, h.data + (size_t)y * h.width, h.width);
    });
    t_alpha_times[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    clock.mark_from(0, st);
    FFHIP_CHECK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
    clock.mark_from(1, st);
    int rc = FFHIP_OK;
    if (!vpart.empty()) {
        for (const AlphaPartFile &p : part) {
            if (p.v < 0) continue;
            d_pic[(size_t)p.j] = work + p.pic_off;
            pic_pitch[(size_t)p.j] = (int64_t)alpha_picture_pitch(af[(size_t)p.j].head);
        }
        int counts[2] = {0, 0}; /* not reported: t_alpha_last[1] counts the lossless planes */
        rc = vp8l_enqueue_part(vpart, dev, pf.data(), d_pic.data(), pic_pitch.data(), st_a.data(), stream, SCRATCH_WEBP_ALPHA, counts, nullptr);
        if (rc) return rc;
        clock.mark_from(1, st);
    }
    std::vector<AlphaUnfDesc> unf;
    std::vector<AlphaMergeDesc> mer;
    unsigned long long total = 0;
    for (const AlphaPartFile &p : part) {
        if (st_a[(size_t)p.j]) continue;
        const AlphaFile &f = af[(size_t)p.j];
        const ffhip_webp_alpha_head &h = f.head;
        AlphaMergeDesc m;
        memset(&m, 0, sizeof(m));
        if (h.compression == 1) {
            m.src = work + p.pic_off + 1; /* the green byte */
            m.src_pitch = (u32)alpha_picture_pitch(h);
            m.src_step = 4;
        } else {
            m.src = dev + vbytes + p.raw_off;
            m.src_pitch = (u32)alpha_plane_pitch(h);
            m.src_step = 1;
        }
        if (h.filter) {
            AlphaUnfDesc u;
            memset(&u, 0, sizeof(u));
            u.src = m.src; u.src_pitch = m.src_pitch; u.src_step = m.src_step;
            u.out = work + p.out_off;
            u.out_pitch = (u32)alpha_plane_pitch(h);
            u.width = h.width; u.rows = h.height; u.filter = (u32)h.filter;
            u.n_bands = (u.rows + ALPHA_BAND - 1) / ALPHA_BAND;
            unf.push_back(u);
            m.src = u.out; m.src_pitch = u.out_pitch; m.src_step = 1;
        }
        m.dst = d_bgra[f.i];
        m.pitch = pitch[f.i];
        m.width = h.width;
        m.height = h.height;
        ffhip_gather_place(m, &total); /* n_wgs < 2^20: both sides below 2^14 */
        mer.push_back(m);
    }
    if (mer.empty()) return FFHIP_OK;
    rc = ffhip_banded_launches(SCRATCH_WEBP_ALPHA + 4, stream, unf, &t_alpha_last[2], [&](u32 level, const AlphaUnfDesc *d_unf, unsigned grid_x, u32 wg_base) {
        AlphaUnfArgs a;
        a.desc = d_unf; a.level = level; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_webp_alpha_unfilter, dim3(grid_x), dim3(ALPHA_BAND), 0, st, a);
    });
    if (rc) return rc;
    clock.mark_from(2, st);
    rc = ffhip_gather_launch(SCRATCH_WEBP_ALPHA + 5, stream, mer, total, [&](const AlphaMergeDesc *d_mer, const u32 *d_table, unsigned grid_x, u32 wg_base) {
        AlphaMergeArgs a;
        a.desc = d_mer; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_webp_alpha_merge, dim3(grid_x), dim3(ALPHA_MERGE_THREADS), 0, st, a);
    });
    clock.mark_from(3, st);
    return rc;
}

} // namespace

int webp_alpha_stage(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch, int *status,
                     void *stream)
{
    n_threads = ffhip_host_threads(n_threads);
    for (int &v : t_alpha_last) v = 0;
    for (double &t : t_alpha_times) t = 0;
    const auto t_open = std::chrono::steady_clock::now();
    /* the chunk walk and the header byte of every delivered file; the lossless planes' transform lists */
    std::vector<ffhip_webp_alpha_head> heads((size_t)n);
    ffhip_parallel_for(n, n_threads, [&](int i) {
        memset(&heads[(size_t)i], 0, sizeof(heads[0]));
        if (status[i]) return;
        const int rc = ffhip_webp_alpha_find(files[i], lens[i], &heads[(size_t)i]);
        if (rc) { status[i] = FFHIP_EINVAL; heads[(size_t)i].has_alpha = 0; }
    });
    std::vector<AlphaFile> af;
    for (int i = 0; i < n; i++)
        if (heads[(size_t)i].has_alpha) af.push_back({i, heads[(size_t)i]});
    if (af.empty()) return FFHIP_OK;
    const size_t m = af.size();
    Vp8lFiles opened(m);
    std::vector<ffhip_vp8l_file> &pf = opened.v;
    std::vector<int> st_a(m, 0);
    ffhip_parallel_for((int)m, n_threads, [&](int j) {
        const ffhip_webp_alpha_head &h = af[(size_t)j].head;
        memset(&pf[(size_t)j], 0, sizeof(pf[0]));
        if (h.compression == 1) st_a[(size_t)j] = ffhip_vp8l_open_stream(h.data, h.data_len, (int32_t)h.width, (int32_t)h.height, 0, 1, &pf[(size_t)j]);
    });
    t_alpha_times[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_open).count();
    std::vector<uint8_t *> d_pic(m, nullptr);
    std::vector<int64_t> pic_pitch(m, 0);
    StageClock clock(FFHIP_ENV("FFHIP_WEBP_ALPHA_TIMES"), t_alpha_times);
    const size_t budget = ffhip_part_budget(FFHIP_ENV("FFHIP_WEBP_ALPHA_PART_BYTES"));
    int rc = FFHIP_OK;
    for (size_t j = 0; j < m && rc == FFHIP_OK;) {
        std::vector<AlphaPartFile> part;
        std::vector<Vp8lPartFile> vpart;
        size_t res = 0, side = 0, raw = 0, work = 0;
        for (; j < m; j++) {
            if (st_a[j]) continue;
            const ffhip_webp_alpha_head &h = af[j].head;
            const size_t plane = alpha_plane_pitch(h) * h.height, picture = h.compression == 1 ? alpha_picture_pitch(h) * h.height : 0;
            if (!part.empty() && res + side + raw + work + plane + picture > budget) break;
            AlphaPartFile p{(int)j, -1, raw, work, work + picture};
            if (h.compression == 1) {
                p.v = (int)vpart.size();
                vp8l_part_add(vpart, pf[j], (int)j, &res, &side);
            } else {
                raw += plane;
            }
            work += picture + (h.filter ? plane : 0);
            part.push_back(p);
        }
        if (part.empty()) break;
        vp8l_part_seal(vpart, res);
        t_alpha_last[3]++;
        rc = ffhip_part_end(alpha_run_part(part, vpart, res + side, raw, work, af, pf, st_a, d_pic, pic_pitch, n_threads, d_bgra, pitch, stream, clock), stream, clock);
    }
    for (size_t j = 0; j < m; j++) {
        if (st_a[j]) status[af[j].i] = st_a[j] == FFHIP_ENOMEM ? FFHIP_ENOMEM : FFHIP_EINVAL;
        t_alpha_last[0] += st_a[j] == 0;
        t_alpha_last[1] += st_a[j] == 0 && af[j].head.compression == 1;
    }
    return rc;
}

extern "C" int ffhip_debug_webp_alpha_last(int out[4]) { return ffhip_copy_out(out, t_alpha_last); }

extern "C" int ffhip_debug_webp_alpha_times(double out[4]) { return ffhip_copy_out(out, t_alpha_times); }
