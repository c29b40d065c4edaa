/* ffhip_items.h -- what the items calls share (ffhip_jpeg_recon_items and its _scaled and _libjpeg forms, ffhip_bgra_resize_items,
 * ffhip_bgra_orient_items, ffhip_bgra_to_tensor_items): the per-workgroup item table, the upload of the records and the launches over a
 * range of workgroups.  A call lays its items' workgroups end to end (first_wg: a prefix sum of n_wgs, the total within 32 bits), uploads
 * the records, has a table kernel write every item's index over its range, and launches its pixel kernel over the range.
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

#endif
