/* ffhip_items.h -- what the items calls share (ffhip_jpeg_recon_items and its _scaled and _libjpeg forms, ffhip_bgra_resize_items,
 * ffhip_bgra_orient_items, ffhip_bgra_to_tensor_items, and the encoders: ffhip_jpeg_encode_items, ffhip_deflate_streams_device,
 * ffhip_png_encode_items, ffhip_vp8l_encode_items): the per-workgroup item table(s), the upload of the records and the launches over a
 * range of workgroups.  A call lays its items' workgroups end to end (first_wg: a prefix sum of n_wgs, the total within 32 bits), uploads
 * the records, has a table kernel write every item's index over its range, and launches its kernels over the range.  The encoders answer
 * with a length and a status per item: ffhip_lengths_read is their read-back of the device's verdicts.
 *
 * The calls only enqueue.  Their contract with the stream -- a second call may refill the pinned records while the first call's copy out of
 * them has not run -- rests on the ffhip_pinned_staging / ffhip_pinned_staged pair, and ffhip_items_stage is the one place that keeps it. */
#ifndef FFHIP_ITEMS_H
#define FFHIP_ITEMS_H

#include "ffhip_internal.h"

#include <string.h>

/* one workgroup per item: the item's index over its range of the per-workgroup table */
template <class Desc> __global__ __launch_bounds__(256) void k_items_table(const Desc *desc, u32 *wg_item)
{
    const u32 item = blockIdx.x, first = desc[item].first_wg, n = desc[item].n_wgs;
    for (u32 k = threadIdx.x; k < n; k += 256) wg_item[first + k] = item;
}

/* two tables in one launch: item i over [FA, FA + NA) of a[i] in a_item and over [FB, FB + NB) of b[i] in b_item (a and b may be one array) */
template <class A, class B, u32 A::*FA, u32 A::*NA, u32 B::*FB, u32 B::*NB>
__global__ __launch_bounds__(256) void k_items_tables2(const A *a, const B *b, u32 *a_item, u32 *b_item)
{
    const u32 item = blockIdx.x;
    const u32 f0 = a[item].*FA, n0 = a[item].*NA, f1 = b[item].*FB, n1 = b[item].*NB;
    for (u32 k = threadIdx.x; k < n0; k += 256) a_item[f0 + k] = item;
    for (u32 k = threadIdx.x; k < n1; k += 256) b_item[f1 + k] = item;
}

/* v up to a multiple of a, a power of two */
inline size_t ffhip_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

/* The scratch of (kind, stream): the records, then `table_words` words of per-workgroup table(s), then `tail_bytes` of the call's own (its
 * padding included).  Enqueues the records' upload through the kind's pinned staging; *dev is the scratch.  ready(dev) runs before the
 * records are copied: records that point into the scratch get their addresses there. */
template <class Ready>
int ffhip_items_stage(int kind, void *stream, const void *records, size_t record_bytes, size_t table_words, size_t tail_bytes, uint8_t **dev, Ready ready)
{
    *dev = (uint8_t *)ffhip_scratch(kind, stream, (record_bytes + 4 * table_words + tail_bytes) / 4 + 16);
    if (!*dev) return FFHIP_ENOMEM;
    uint8_t *pin = ffhip_pinned_staging(kind, stream, record_bytes);
    if (!pin) return FFHIP_ENOMEM;
    ready(*dev);
    memcpy(pin, records, record_bytes);
    FFHIP_CHECK(hipMemcpyAsync(*dev, pin, record_bytes, hipMemcpyHostToDevice, (hipStream_t)stream), FFHIP_EIO);
    return ffhip_pinned_staged(kind, stream) != FFHIP_OK ? FFHIP_EIO : FFHIP_OK;
}
inline int ffhip_items_stage(int kind, void *stream, const void *records, size_t record_bytes, size_t table_words, size_t tail_bytes, uint8_t **dev)
{
    return ffhip_items_stage(kind, stream, records, record_bytes, table_words, tail_bytes, dev, [](uint8_t *) {});
}

/* the common form: records of one type with first_wg / n_wgs, one table of `total` workgroups behind them, written by k_items_table */
template <class Desc> int ffhip_items_upload(int kind, void *stream, const std::vector<Desc> &desc, unsigned long long total, const Desc **d_desc, u32 **d_table)
{
    uint8_t *dev = nullptr;
    const size_t bytes = desc.size() * sizeof(Desc);
    const int rc = ffhip_items_stage(kind, stream, desc.data(), bytes, (size_t)total, 0, &dev);
    if (rc) return rc;
    *d_desc = (const Desc *)dev;
    *d_table = (u32 *)(dev + bytes);
    hipLaunchKernelGGL(k_items_table<Desc>, dim3((unsigned)desc.size()), dim3(256), 0, (hipStream_t)stream, *d_desc, *d_table);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

/* launch(grid_x, wg_base) over the workgroups [first, last): a launch stays below 2^31 workgroups, a range may not */
template <class Launch> int ffhip_items_launch(unsigned long long first, unsigned long long last, Launch launch)
{
    for (unsigned long long b = first; b < last; b += 0x7fffffffULL) {
        const unsigned long long left = last - b;
        launch((unsigned)(left < 0x7fffffffULL ? left : 0x7fffffffULL), (u32)b);
        FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    }
    return FFHIP_OK;
}

/* kernel(args, rest...) with `threads` threads over the workgroups [0, total), args.wg_base set per launch */
template <class Kernel, class Args, class... Rest>
int ffhip_items_run(Kernel kernel, unsigned long long total, unsigned threads, void *stream, Args &args, const Rest &...rest)
{
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        args.wg_base = wg_base;
        hipLaunchKernelGGL(kernel, dim3(grid_x), dim3(threads), 0, (hipStream_t)stream, args, rest...);
    });
}

/* n records of the device into pinned scratch `kind`, and the wait for them: a synchronisation of the stream */
template <class V> int ffhip_records_fetch(int kind, void *stream, const V *d_records, int n, const V **host)
{
    V *h = (V *)ffhip_pinned_scratch(kind, stream, (size_t)n * sizeof(V));
    if (!h) return FFHIP_ENOMEM;
    FFHIP_CHECK(hipMemcpyAsync(h, d_records, (size_t)n * sizeof(V), hipMemcpyDeviceToHost, (hipStream_t)stream), FFHIP_EIO);
    FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO);
    *host = h;
    return FFHIP_OK;
}

/* an encoder's last step: the verdicts (file_len, status) fetched, into len_out[] and status[]; the first status that is not FFHIP_OK */
template <class V> int ffhip_lengths_read(int kind, void *stream, const V *d_verdicts, int n, size_t *len_out, int *status)
{
    const V *h = nullptr;
    const int rc = ffhip_records_fetch(kind, stream, d_verdicts, n, &h);
    if (rc) return rc;
    int first = FFHIP_OK;
    for (int i = 0; i < n; i++) {
        len_out[i] = (size_t)h[i].file_len;
        status[i] = h[i].status;
        if (first == FFHIP_OK && status[i] != FFHIP_OK) first = status[i];
    }
    return first;
}

#endif
