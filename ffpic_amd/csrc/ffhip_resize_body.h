/* ffhip_resize_body.h -- the resize rule for one output index of one axis (include/ffpic_hip.h, "decoded pictures resized on the
 * device") and the record of an item of ffhip_bgra_resize_items (ffhip_resize.hip).  Plain C++ without builtins, __host__
 * too: ffhip_resize_axis_taps on the host and the table kernel on the device run the same function, and a CPU program can hold it against
 * the rule written another way.
 *
 * Everything fits unsigned 32-bit for sides up to 16384: (2 k + 1) n_out and c < 2^30, S <= 2^15, r <= 2^15, 4096 r + R / 2 < 2^28 + 2^29
 * (R <= count * S <= 2^14 * 2^15). */
#ifndef FFHIP_RESIZE_BODY_H
#define FFHIP_RESIZE_BODY_H

#include <stdint.h>

#include "ffpic_hip.h"
#include "ffhip_alpha_body.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define FFHIP_RESIZE_WG_THREADS 256 /* of the resize kernel: one output column each */

/* the most taps an output index of the axis can have: the samples (2 k + 1) n_out of an open interval of length 2 S lie 2 n_out apart */
__host__ __device__ inline uint32_t resize_axis_max_taps(uint32_t n_in, uint32_t n_out, int filter)
{
    const uint32_t S = 2u * (filter == FFHIP_RESIZE_ANTIALIAS && n_in > n_out ? n_in : n_out);
    const uint32_t m = (S + n_out - 1u) / n_out;
    return m < n_in ? m : n_in;
}

struct ResizeRun { uint32_t first, count, S, c, R, best; }; /* best: the tap (index into the run) that takes the residual */

__host__ __device__ inline uint32_t resize_raw_weight(const ResizeRun &t, uint32_t n_out, uint32_t k)
{
    const uint32_t p = (2u * k + 1u) * n_out;
    return t.S - (p > t.c ? p - t.c : t.c - p);
}

/* the run of taps of output `o`: arguments already checked (1 <= n_in, n_out <= 16384, o < n_out) */
__host__ __device__ inline ResizeRun resize_axis_run(uint32_t n_in, uint32_t n_out, int filter, uint32_t o)
{
    ResizeRun t;
    t.S = 2u * (filter == FFHIP_RESIZE_ANTIALIAS && n_in > n_out ? n_in : n_out);
    t.c = (2u * o + 1u) * n_in;
    /* the lowest k with (2 k + 1) n_out > c - S, i.e. 2 k + 1 >= floor((c - S) / n_out) + 1 where c > S */
    uint32_t k = 0;
    if (t.c > t.S) {
        const uint32_t m = (t.c - t.S) / n_out + 1u; /* 2 k + 1 >= m */
        k = m / 2u;                                  /* m odd: (m - 1) / 2; m even: m / 2 */
    }
    t.first = k;
    t.count = 0; t.R = 0; t.best = 0;
    uint32_t best_r = 0;
    for (; k < n_in && (2u * k + 1u) * n_out < t.c + t.S; k++) {
        const uint32_t r = resize_raw_weight(t, n_out, k);
        if (r > best_r) { best_r = r; t.best = t.count; } /* the lowest k on a tie */
        t.R += r;
        t.count++;
    }
    return t;
}

/* weight j (< t.count) of the run, the residual aside */
__host__ __device__ inline uint32_t resize_weight(const ResizeRun &t, uint32_t n_out, uint32_t j)
{
    return (resize_raw_weight(t, n_out, t.first + j) * 4096u + t.R / 2u) / t.R;
}

/* Every weight of the run through store(j, q_j), in no particular order; a tap's LAST store is its weight.  Step 4: the residual 4096 - sum goes to tap `best`.  Step 5
 * (every q >= 0) is kept where a long run rounds up more often than its largest weight can pay for (ANTIALIAS 1080 -> 1: 41 too many
 * against a largest weight of 7): the largest tap goes to 0 and what is still owed is taken from the taps that follow it in the order of
 * step 4 -- falling r, the lowest k on a tie -- each down to 0 at most.  The run's r rises to `best` and falls behind it, so that order
 * is a walk outwards from `best`. */
template <class Store> __host__ __device__ inline void resize_axis_weights(const ResizeRun &t, uint32_t n_out, Store store)
{
    uint32_t sum = 0, at_best = 0;
    for (uint32_t j = 0; j < t.count; j++) {
        const uint32_t w = resize_weight(t, n_out, j);
        sum += w;
        if (j == t.best) at_best = w;
        else store(j, w);
    }
    if (at_best + 4096u >= sum) { store(t.best, at_best + 4096u - sum); return; }
    uint32_t owed = sum - 4096u - at_best; /* < the sum of the other weights: they sum to 4096 + owed */
    store(t.best, 0u);
    uint32_t lo = t.best, hi = t.best + 1u; /* the next taps below and above: lo - 1 and hi */
    while (owed && (lo > 0u || hi < t.count)) {
        const uint32_t r_lo = lo > 0u ? resize_raw_weight(t, n_out, t.first + lo - 1u) : 0u;
        const uint32_t r_hi = hi < t.count ? resize_raw_weight(t, n_out, t.first + hi) : 0u;
        const uint32_t j = lo > 0u && (hi >= t.count || r_lo >= r_hi) ? --lo : hi++;
        const uint32_t w = resize_weight(t, n_out, j), take = w < owed ? w : owed;
        store(j, w - take);
        owed -= take;
    }
}

/* A source pixel as the resize kernel stages it into its row: as it is, or premultiplied (ffhip_bgra_resize_items_premultiplied) */
template <bool PREMUL> __host__ __device__ inline uint32_t resize_staged(uint32_t px) { return PREMUL ? alpha_premultiply_pixel(px) : px; }

/* One item of a call, as the kernels read it.  The tap tables of an axis: fc[o] = first | count << 16 (first <= 16383, count <= 16384), and the
 * weights TAP-MAJOR, q[j * n_out + o] for tap j of output o, so that the lanes of a
 * wave, one output column each, load a tap's weights from consecutive addresses. */
struct ResizeItemDesc { /* 96 bytes */
    const uint8_t *src; /* pixel (x0, y0) */
    uint8_t *dst;
    long long src_pitch, dst_pitch;
    int width, height, out_width, out_height;
    uint32_t first_wg, n_wgs; /* its workgroups: out_height x tiles_x */
    uint32_t tiles_x;         /* column tiles of FFHIP_RESIZE_WG_THREADS outputs */
    uint32_t pad_;
    long long fcx, fcy;       /* byte offsets of the tables in the call's scratch */
    long long qx, qy;
};

#endif
