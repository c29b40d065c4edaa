/* ffhip_planes.h -- the layout arithmetic of the JPEG file calls (ffhip_pipeline.hip): how a batch's planes and tables
 * share one block, and how the rows of a chunk are split over the host threads that copy them out.  Plain C++ with no HIP in it, so that
 * tests/tools/check_slots.cpp runs it on the CPU. */
#ifndef FFHIP_PLANES_H
#define FFHIP_PLANES_H

#include <stddef.h>
#include <stdint.h>

/* Y | U | V | quantiser tables of a batch in one block, device or pinned: yb and cb are the int16 elements of the luma plane and of each chroma
 * plane (cb 0: grey, no chroma planes), the n pictures' tables lie on a 16-byte boundary behind the planes */
struct Planes { int16_t *y, *u, *v; uint16_t *q; };
struct PlaneBlock {
    size_t yb, cb, q_off, bytes;
    PlaneBlock(size_t yb_, size_t cb_, size_t n) : yb(yb_), cb(cb_), q_off(((yb_ + 2 * cb_) * 2 + 15) & ~(size_t)15), bytes(q_off + n * 512) {}
    Planes at(uint8_t *base) const { int16_t *y = (int16_t *)base; return {y, cb ? y + yb : nullptr, cb ? y + yb + cb : nullptr, (uint16_t *)(base + q_off)}; }
};

/* copy_out: the host threads that copy `rows` rows -- 16 at most, one below 64 rows -- and the rows [lo, hi) thread t of nt takes: contiguous,
 * in order, every row of [0, rows) once */
inline int ffhip_copy_threads(long long rows, int n_threads) { return rows < 64 || n_threads < 1 ? 1 : n_threads > 16 ? 16 : n_threads; }
struct FfhipRows { long long lo, hi; };
inline FfhipRows ffhip_copy_rows(long long rows, int t, int nt) { return {rows * t / nt, rows * (t + 1) / nt}; }

#endif
