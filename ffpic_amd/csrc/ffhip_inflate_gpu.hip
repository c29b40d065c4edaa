/* ffhip_inflate_gpu.hip -- zlib streams inflated on the device, a wave per stream (include/ffpic_hip.h, "PNG, inflate on the device";
 * DESIGN.md 4.30): k_inflate and ffhip_inflate_streams_device.  The algorithm is ffhip_inflate_body.h, which the host model
 * (ffhip_inflate_model.c) compiles too.
 *
 * k_inflate.  One 64-thread workgroup, one wave, per stream record; the records are sorted by compressed length, longest first, so a
 * workgroup's record is its index and the tail of a launch is the short streams.  The serial part of the body is wave-uniform: every
 * lane runs it on the same bytes, with the tables, the code lengths and the batch's steps in LDS (every lane stores the same value at
 * the same address).  A step of the writer part is one load and one store per lane.  The window is the output itself, in global
 * memory: in front of a match's first step stands a workgroup-scope fence, so that the stores of the steps before it are visible to
 * its loads; the loads of a step never read what a store of the same step, or of the same match, writes.  Adler-32 is summed by the wave
 * over the finished output, and a record with the PNG tail has every row's filter byte checked, lanes over rows.
 *   No error path other than the record's status word; no unbounded loop and no spin-wait: every loop that consumes input counts its
 * turns against 8 x len + 64 (ffhip_inflate_body.h), the others run to bounds known at their entry. */
#include "ffhip_inflate_gpu.h"
#include "ffhip_items.h"
#include "ffhip_inflate_body.h"

#include <algorithm>

namespace {

__device__ __forceinline__ u32 wave_sum(u32 v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (u32)__shfl_xor((int)v, o, 64);
    return v;
}

__global__ __launch_bounds__(FFHIP_INF_LANES) void k_inflate(FfhipInflateRec *rec, u32 wg_base)
{
    __shared__ ffhip_inf_store store;
    FfhipInflateRec *r = rec + wg_base + blockIdx.x;
    const int lane = (int)threadIdx.x;
    const uint8_t *src = r->src;
    uint8_t *dst = r->dst;
    ffhip_inf_state st;
    int rc = ffhip_inf_begin(&st, src, r->len, r->cap, (int)r->partial);
    bool dirty = false; /* stores since the last fence */
    while (!rc && !st.done) { /* a batch that does not end the stream has counted at least one turn */
        const int n = ffhip_inf_batch(&st, &store);
        if (n < 0) { rc = n; break; }
        for (int k = 0; k < n; k++) {
            const ffhip_inf_step *s = &store.step[k];
            if (dirty && ffhip_inf_step_reads_output(s)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                dirty = false;
            }
            uint8_t v;
            if (ffhip_inf_step_load(s, &store, src, dst, lane, &v)) ffhip_inf_step_store(s, dst, lane, v);
            dirty = true;
        }
    }
    const unsigned long long out_len = st.out_len;
    if (dirty) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (!rc && !st.full) { /* the condition of ffhip_inflate_upto: ended by its last block, not stopped by a full output */
        u32 a = 1, b = 0;
        for (unsigned long long at = 0; at < out_len; at += FFHIP_INF_ADLER_BLOCK) {
            const u32 m = out_len - at < FFHIP_INF_ADLER_BLOCK ? (u32)(out_len - at) : FFHIP_INF_ADLER_BLOCK;
            u32 s1, s2;
            ffhip_inf_adler_lane(dst + at, m, lane, &s1, &s2);
            ffhip_inf_adler_fold(&a, &b, m, wave_sum(s1), wave_sum(s2));
        }
        if (st.want != (b << 16 | a)) rc = FFHIP_EINVAL;
    }
    if (!rc && r->png) { /* ffhip_png_read_filtered's: the whole filtered picture, every filter byte one of the five */
        if (out_len != r->cap) rc = FFHIP_EINVAL;
        unsigned long long sub = 0;
        int bad = 0;
        for (int p = 0; p < 7 && !rc; p++) {
            const u32 rows = r->rows[p];
            const unsigned long long pitch = r->pitch[p];
            for (u32 y = (u32)lane; y < rows; y += FFHIP_INF_LANES) bad |= dst[sub + y * pitch] > 4;
            sub += pitch * rows;
        }
        if (__any(bad)) rc = FFHIP_EINVAL;
    }
    if (lane == 0) {
        r->status = rc;
        r->out_len = out_len;
    }
}

} // namespace

void ffhip_inflate_sort(std::vector<FfhipInflateRec> &rec)
{
    std::stable_sort(rec.begin(), rec.end(), [](const FfhipInflateRec &x, const FfhipInflateRec &y) { return x.len > y.len; });
}

int ffhip_inflate_launch(FfhipInflateRec *d_rec, size_t n, void *stream)
{
    return ffhip_items_launch(0, n, [&](unsigned grid_x, u32 wg_base) {
        hipLaunchKernelGGL(k_inflate, dim3(grid_x), dim3(FFHIP_INF_LANES), 0, (hipStream_t)stream, d_rec, wg_base);
    });
}

extern "C" int ffhip_inflate_streams_device(const uint8_t *const *src, const size_t *len, int n, uint8_t *const *d_dst, const size_t *cap,
                                            size_t *out_len, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!src || !len || !d_dst || !cap || !out_len || !status))) return FFHIP_EINVAL;
    for (int i = 0; i < n; i++)
        if ((!src[i] && len[i]) || (!d_dst[i] && cap[i])) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    /* the staging, pinned and device alike: the streams, each at a multiple of 8, then the records */
    std::vector<FfhipInflateRec> rec((size_t)n);
    size_t bytes = 0;
    for (int i = 0; i < n; i++) {
        FfhipInflateRec &r = rec[(size_t)i];
        memset(&r, 0, sizeof(r));
        r.src = (const uint8_t *)bytes; /* an offset until the staging is known */
        r.dst = d_dst[i];
        r.len = len[i];
        r.cap = cap[i];
        r.index = (u32)i;
        bytes += (len[i] + 7) & ~(size_t)7;
    }
    const size_t rec_bytes = rec.size() * sizeof(FfhipInflateRec);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_PNG, stream, bytes + rec_bytes);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_PNG, stream, (bytes + rec_bytes) / 4 + 16);
    if (!pin || !dev) return FFHIP_ENOMEM;
    for (FfhipInflateRec &r : rec) {
        const size_t off = (size_t)r.src;
        if (r.len) memcpy(pin + off, src[r.index], (size_t)r.len);
        r.src = dev + off;
    }
    ffhip_inflate_sort(rec);
    memcpy(pin + bytes, rec.data(), rec_bytes);
    FFHIP_CHECK(hipMemcpyAsync(dev, pin, bytes + rec_bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
    const int rc = ffhip_inflate_launch((FfhipInflateRec *)(dev + bytes), rec.size(), stream);
    if (rc) return rc;
    FFHIP_CHECK(hipMemcpyAsync(pin + bytes, dev + bytes, rec_bytes, hipMemcpyDeviceToHost, st), FFHIP_EIO);
    FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO);
    const FfhipInflateRec *back = (const FfhipInflateRec *)(pin + bytes);
    for (int k = 0; k < n; k++) {
        status[back[k].index] = back[k].status;
        out_len[back[k].index] = (size_t)back[k].out_len;
    }
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}
