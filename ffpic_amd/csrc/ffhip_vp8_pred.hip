/*
 * ffhip_vp8_pred.hip -- VP8 (WebP lossy) intra prediction + residual add for batches of key
 * frames, bit-exact with
 *   pred_luma / pred_chrome        format/predict.c:426-645
 *   the 18 predictors              format/predict.c:34-355
 *   add_residue_subblock           format/predict.c:378-389
 * looped like vp8_decode (format/webp.c:1833-1851), including the reference's own edge
 * rules (129/127 defaults, 127 top-right inside a macroblock, 16x16 V/H predictors that
 * copy raw memory -- predict.c:338-353 -- for which bytes before the plane read as 0).
 *
 * This stage is dependency-bound, not bandwidth-bound: a macroblock needs its left, above, above-left and above-right neighbours
 * reconstructed.  The file holds two forms of it:
 *   - the ROW form, the default (k_vp8_predict_rows): one launch per batch, a wave owns a macroblock row of one image, rows are handed
 *     out by ticket and follow the row above through per-row progress counters; no host-side scheduling.  It is also the prediction half
 *     of the side-by-side call (ffhip_vp8_lf.hip) and the small-batch form of ffhip_vp8_decode_frames (ffhip_vp8_frame.hip).
 *   - the LEVELS form (k_vp8_predict): the host assigns every macroblock a wavefront level (x + 2y, plus one extra edge for the
 *     reference's wrapped H_PRED read at x = 0) and there is one launch per level over all images of the batch, a wave per macroblock.
 *     The fallback for what the row form does not take (unaligned mode records, a plane of 2^23 macroblocks) and the A/B form
 *     (FFHIP_VP8_PRED_MODE=levels).  Also here: the device check of mode records and what both stages' host entries share.
 */
#include "ffhip_vp8_device.h"

#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

struct Vp8PredArgs {
    const uint8_t *modes;    /* [n_images][n_mb][20]                      */
    const int16_t *residual; /* [n_images][res_rows][384]                 */
    const int32_t *resmap;   /* [n_images][n_mb] or NULL                  */
    const uint32_t *work;    /* this level: (image, mb) pairs             */
    uint8_t *y, *u, *v;
    long long plane_y, plane_uv, res_stride;
    int mbcols, mbrows, count;
    /* row form only */
    int pshift;     /* a row's progress counter is word (image * mbrows + row) << pshift behind the header (FFHIP_VP8_PROGRESS_SHIFT) */
    uint32_t *ctrl; /* [0] next luma row ticket, [FFHIP_VP8_CTRL_TICKET_C] next chroma row ticket, [FFHIP_VP8_CTRL_ABORT] abort; from ctrl + FFHIP_VP8_CTRL_HDR: luma macroblocks finished per (image, row), then the chroma ones */
    int *async_err; /* pinned host word (ffhip_async_err_word) */
    int n_images;
    int split; /* 1: luma rows and chroma rows are separate rows (other waves); 0: one wave walks both parts of a row */
    int slack; /* a row that has to BLOCK on the row above waits until that row is this many macroblocks further than needed (throughput regime: see the host side) */
    unsigned long long *trace; /* diagnostics (ffhip_debug_vp8_trace): per (image, row) EIGHT words: the 100 MHz clock at ticket, first macroblock, middle, last store; then the row's time (same clock) summed per phase: fetch wait + consume, poll + next fetch's issue, luma, chroma */
};

__device__ __forceinline__ int px_or0(const uint8_t *plane, long long off) { return off < 0 ? 0 : plane[off]; }

#define TS 24 /* tile row stride: 1 left + 16 + 4 top-right, padded */

/* DC / TM / VE / HE value of an NxN block pixel from edge arrays with the reference's rules */
template <int N>
__device__ __forceinline__ int pred_nxn(int mode, int r, int c, const int *top /* -1..N-1 via top[k+1] */,
                                        const int *left, int x, int y)
{
    constexpr int SH = N == 16 ? 4 : 3;
    if (mode == 0) {
        int dc = 0;
        if (x > 0) for (int i = 0; i < N; i++) dc += left[i];
        if (y > 0) for (int i = 0; i < N; i++) dc += top[i + 1];
        if (x == 0 && y == 0) dc = 0x80;
        else if (x == 0 || y == 0) dc = (dc + (1 << (SH - 1))) >> SH;
        else dc = (dc + (1 << SH)) >> (SH + 1);
        return dc & 0xff;
    }
    if (mode == 1) return clamp255(left[r] + top[c + 1] - top[0]);
    if (mode == 2) return top[c + 1];
    return left[r];
}

__global__ __launch_bounds__(256) void k_vp8_predict(Vp8PredArgs a)
{
    __shared__ uint8_t tiles[4][17 * TS];
    __shared__ short resl[4][384];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + w;
    if (item >= a.count) return;
    const int img = (int)a.work[2 * item], mb = (int)a.work[2 * item + 1];
    const int n_mb = a.mbcols * a.mbrows;
    const int x = mb % a.mbcols, y = mb / a.mbcols;
    const uint8_t *m = a.modes + ((long long)img * n_mb + mb) * 20;
    const int ymode = m[0], uvmode = m[1];
    const long long rrow = a.resmap ? a.resmap[(long long)img * n_mb + mb] : mb;
    const int16_t *coff = a.residual + (long long)img * a.res_stride + rrow * 384;
    uint8_t *T = tiles[w];
    short *R = resl[w];

    /* residual -> LDS (768 B = 64 lanes x 12 B) */
    {
        const u32 *src = (const u32 *)coff;
        u32 *dst = (u32 *)R;
#pragma unroll
        for (int i = 0; i < 3; i++) dst[lane * 3 + i] = src[lane * 3 + i];
    }
    /* ---- luma ---- */
    const int ys = 16 * a.mbcols;
    uint8_t *Y = a.y + (long long)img * a.plane_y;
    const long long org = (long long)y * 16 * ys + x * 16;
    /* borders as raw memory: tile row 0 = the row above (cols -1..19), tile col 0 = dst[-1] of each row */
    if (lane < 21) T[lane] = (uint8_t)px_or0(Y, org - ys + (lane - 1));
    if (lane >= 32 && lane < 48) T[(lane - 32 + 1) * TS] = (uint8_t)px_or0(Y, org + (long long)(lane - 32) * ys - 1);
    wave_sync();

    if (ymode == 4) { /* B_PRED: 16 dependent 4x4 steps, 16 lanes each */
        const int r = (lane >> 2) & 3, c = lane & 3;
        for (int n = 0; n < 16; n++) {
            const int xs = n & 3, ysb = n >> 2;
            if (lane < 16) {
                const uint8_t *S = T + (ysb * 4 + 1) * TS + xs * 4 + 1; /* sub-block origin in the tile */
                int e[13];
#pragma unroll
                for (int k = 0; k < 4; k++) e[3 - k] = (x > 0 || xs > 0) ? S[k * TS - 1] : 129;
                if (y == 0 && ysb == 0) {
#pragma unroll
                    for (int k = 4; k < 13; k++) e[k] = 127;
                } else if (ysb == 0) {
#pragma unroll
                    for (int k = 0; k < 8; k++) e[5 + k] = S[-TS + k];
                    e[4] = (xs > 0 || x > 0) ? S[-TS - 1] : 129;
                    if (x == a.mbcols - 1 && xs == 3) { e[9] = e[10] = e[11] = e[12] = 127; }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) e[5 + k] = S[-TS + k];
#pragma unroll
                    for (int k = 4; k < 8; k++) e[5 + k] = xs == 3 ? 127 : S[-TS + k];
                    e[4] = (xs == 0 && x == 0) ? 129 : S[-TS - 1];
                }
                const int mode = m[2 + n];
                int p;
                if (mode == 0) {
                    int dc = 4;
#pragma unroll
                    for (int k = 0; k < 4; k++) dc += e[5 + k] + e[k];
                    p = dc >> 3;
                } else if (mode == 1) {
                    /* e[3-r] = left[r]; dynamic index resolved by selects */
                    const int lf = r == 0 ? e[3] : (r == 1 ? e[2] : (r == 2 ? e[1] : e[0]));
                    const int tp = c == 0 ? e[5] : (c == 1 ? e[6] : (c == 2 ? e[7] : e[8]));
                    p = clamp255(lf + tp - e[4]);
                } else {
                    const unsigned t = kVp8Taps[mode - 2][lane];
                    int va = 0, vb = 0, vc = 0;
#pragma unroll
                    for (int k = 0; k < 13; k++) { /* register array, compile-time indices only */
                        va = (int)(t & 15) == k ? e[k] : va;
                        vb = (int)((t >> 4) & 15) == k ? e[k] : vb;
                        vc = (int)(t >> 8) == k ? e[k] : vc;
                    }
                    p = (va + 2 * vb + vc + 2) >> 2;
                }
                ((uint8_t *)S)[r * TS + c] = (uint8_t)clamp255(p + R[16 * n + lane]);
            }
            wave_sync();
        }
    } else {
        int top[17], left[16];
#pragma unroll
        for (int k = 0; k < 17; k++) top[k] = 127;
#pragma unroll
        for (int k = 0; k < 16; k++) left[k] = 129;
        if (x > 0) {
#pragma unroll
            for (int k = 0; k < 16; k++) left[k] = T[(k + 1) * TS];
        }
        if (y > 0) {
#pragma unroll
            for (int k = 0; k < 16; k++) top[k + 1] = T[k + 1];
            top[0] = x > 0 ? T[0] : 129;
        }
        const int r = lane >> 2, c0 = (lane & 3) * 4;
        int dcv = 0;
        if (ymode == 0) dcv = pred_nxn<16>(0, 0, 0, top, left, x, y);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = c0 + k;
            int p;
            if (ymode == 0) p = dcv;
            else if (ymode == 2) p = T[c + 1];                  /* raw row above (predict.c:338-344) */
            else if (ymode == 3) p = T[(r + 1) * TS];           /* raw dst[-1]   (predict.c:346-353) */
            else {
                int lf = 0, tp = 0;
#pragma unroll
                for (int q = 0; q < 16; q++) { lf = q == r ? left[q] : lf; tp = q == c ? top[q + 1] : tp; }
                p = clamp255(lf + tp - top[0]);
            }
            const int ri = 16 * (4 * (r >> 2) + (c >> 2)) + 4 * (r & 3) + (c & 3);
            T[(r + 1) * TS + c + 1] = (uint8_t)clamp255(p + R[ri]);
        }
        wave_sync();
    }
    /* luma tile -> plane: one dword (4 px) per lane */
    {
        const int r = lane >> 2, c0 = (lane & 3) * 4;
        const uint8_t *s = T + (r + 1) * TS + c0 + 1;
        const u32 v = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
        *(u32 *)(Y + org + (long long)r * ys + c0) = v;
    }

    /* ---- chroma: one pixel of U and one of V per lane ---- */
    const int us = 8 * a.mbcols;
    const long long corg = (long long)y * 8 * us + x * 8;
    const int r = lane >> 3, c = lane & 7;
#pragma unroll
    for (int pl = 0; pl < 2; pl++) {
        uint8_t *P = (pl ? a.v : a.u) + (long long)img * a.plane_uv;
        int top[9], left[8];
#pragma unroll
        for (int k = 0; k < 9; k++) top[k] = 127;
#pragma unroll
        for (int k = 0; k < 8; k++) left[k] = 129;
        if (x > 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) left[k] = P[corg + (long long)k * us - 1];
        }
        if (y > 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) top[k + 1] = P[corg - us + k];
            top[0] = x > 0 ? P[corg - us - 1] : 129;
        }
        int p;
        if (uvmode == 0) p = pred_nxn<8>(0, 0, 0, top, left, x, y);
        else {
            int lf = 0, tp = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) { lf = q == r ? left[q] : lf; tp = q == c ? top[q + 1] : tp; }
            p = uvmode == 1 ? clamp255(lf + tp - top[0]) : (uvmode == 2 ? tp : lf);
        }
        const int ri = 256 + 64 * pl + 16 * (2 * (r >> 2) + (c >> 2)) + 4 * (r & 3) + (c & 3);
        const int outv = clamp255(p + R[ri]);
        /* all border reads of this wave are done before any of its stores land in the same rows:
         * the stores below only touch the macroblock's own pixels */
        P[corg + (long long)r * us + c] = (uint8_t)outv;
    }
}

/* Row form: ONE launch per batch.  A wave owns one macroblock row of one image and walks it left
 * to right, so the left neighbour never leaves LDS; what it needs from the row above it reads
 * with agent-scope loads once that row's progress counter says macroblock x + 1 is out (the
 * whole row for the reference's wrapped H_PRED at x = 0).  Rows are handed out by ticket, row
 * index major, so the row a wave waits for always has a smaller ticket and is running or done.
 * The next macroblock's residual, modes and upper border are fetched while the current one is
 * predicted.  Stores are agent-scope; the row counter moves three macroblocks late, when the
 * in-order completion of the wave's vector-memory operations proves them done without a drain.
 *
 * The macroblock lives in an LDS tile whose borders are first rewritten to what the reference's
 * edge rules say (129 left of the picture, 127 above it and right of it, predict.c:433-437,
 * 492-517) unless the 16x16 mode is V_PRED/H_PRED, which copy raw memory (predict.c:338-353);
 * after that every predictor is a handful of plain tile reads. */
#define VP8_SPIN_LIMIT (1 << 21)
struct Vp8Fetch {
    u32 res[3]; /* the part's share of the residual: 12 B per lane (whole macroblock), 8 B (luma) or 4 B (chroma) */
    u32 mo;    /* lanes 0..4: one dword of the 20 mode bytes */
    int a, b, c; /* one border byte per lane, by the lane's role: luma top (lanes 0..20: columns -1..19 of the row above), U top
                    (21..29), V top (32..40), raw luma left at x = 0 (48..63) -- one load per plane, a lane without a role in
                    that plane reads 0; OR-ed when the fetch is CONSUMED (combined at the loads, the OR would wait for them there) */
};

/* what a lane does, by its number: constants of the launch */
struct Vp8Lane {
    int offY, offU, offV; /* offsets of its border byte from the macroblock's first luma / chroma pixel (no role in that plane: far outside it) */
    int dst1, dst2;       /* where the byte goes in the tile array; chroma left columns */
    int carry_src;        /* the previous macroblock's right column, for the lanes that carry it over */
    int lumaY_lane, chroma_lane;
    int ys, us, n_mb;
};

/* ONE ROW of one image: all of it (PART 0), its luma (PART 1) or its chroma (PART 2).  The two are separate dependency chains -- luma reads luma, chroma
 * reads chroma, both read the modes and their own third of the residual -- and until round 3 one wave walked both: a macroblock
 * cost 1.72 us of which the chroma was 0.33 and its share of the fetch another 0.1 (profiles/r3_vp8_batch_waves_16.json), all of it
 * on the chain a frame's 68 rows hang on.  As rows of their own the chroma runs on other waves, ahead of the luma (it is three
 * times cheaper and needs no above-right neighbour), with progress counters of its own that the side-by-side filter also looks at.
 * TRACE: the diagnostics instantiation stamps clocks (ffhip_debug_vp8_trace; luma rows).  As a run-time `if (a.trace)` the five
 * stamps per macroblock -- branches that are never taken -- cost the shipped kernel 8 % on 16 frames of random modes (3.41 -> 3.13
 * ms): they end basic blocks in the middle of the macroblock loop.  Returns false when the call has been given up. */
template <bool TRACE, int PART>
__device__ __forceinline__ bool vp8_row(const Vp8PredArgs &a, const Vp8Lane &L, const int lane, const int y, const int img, uint8_t *BT, short *R, const u32 *TT)
{
    uint8_t *const T = BT;
    uint8_t *const C0 = BT + BT_C0, *const C1 = BT + BT_C1;
    const int ys = L.ys, us = L.us, n_mb = L.n_mb;
    uint32_t *const progress = a.ctrl + FFHIP_VP8_CTRL_HDR + ((PART == 2 ? (long long)a.n_images * a.mbrows : 0LL) << a.pshift);
    unsigned long long *const tr = TRACE && (PART == 0 || (PART == 2) == ((a.slack & 0x1000) != 0)) && a.trace ? /* (diagnostics: slack bit 12 = trace the chroma rows of a split launch instead of the luma rows) */ a.trace + 8 * ((long long)img * a.mbrows + y) : nullptr;
    unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0, tp = 0;
    if (tr && lane == 0) tr[0] = wall_clock64();
    uint8_t *Y = a.y + (long long)img * a.plane_y;
    uint8_t *U = a.u + (long long)img * a.plane_uv, *V = a.v + (long long)img * a.plane_uv;
    const uint8_t *mrow = a.modes + ((long long)img * n_mb + (long long)y * a.mbcols) * 20;
    const int32_t *maprow = a.resmap ? a.resmap + (long long)img * n_mb + (long long)y * a.mbcols : nullptr;
    const uint32_t *prog_up = progress + (((long long)img * a.mbrows + y - 1) << a.pshift);
    uint32_t *prog_me = progress + (((long long)img * a.mbrows + y) << a.pshift);
    unsigned seen = y == 0 ? 0x7fffffffu : 0u; /* macroblocks of the row above known to be finished */
    const __amdgpu_buffer_rsrc_t rY = ffhip_rsrc(Y, 256u * (unsigned)n_mb), rU = ffhip_rsrc(U, 64u * (unsigned)n_mb),
                                 rV = ffhip_rsrc(V, 64u * (unsigned)n_mb);
    const __amdgpu_buffer_rsrc_t rRes = ffhip_rsrc(a.residual + (long long)img * a.res_stride,
                                                   (unsigned)(a.res_stride * 2 > 0xffffffffLL ? 0xffffffffLL : a.res_stride * 2));
    const __amdgpu_buffer_rsrc_t rMo = ffhip_rsrc(mrow, 20u * (unsigned)a.mbcols);
    const int row_org = y * 16 * ys, row_corg = y * 8 * us;

    /* issue everything macroblock x1 needs -- no lane conditions; blocks only while the row above is not far enough */
    /* A poll of the row above is a trip to memory, and a row that follows the row above in lock-step needs a fresh value for
     * EVERY macroblock: waiting for it made the step t + L instead of t (so every row fell further behind the one above
     * until its polls became rare: the lag between rows grew to ~ sqrt(2 (L / t) x) macroblocks, which is most of a
     * frame's time).  So one poll is always in flight: issued behind this fetch, read in front of the next one, when it has
     * had a whole macroblock to come back.  Its value is a macroblock old -- never too new -- and if it does not suffice the
     * blocking poll below takes over. */
    u32 poll_v = 0;
    bool poll_out = false;
    auto fetch = [&](int x1, long long rrow, unsigned need, Vp8Fetch &f) -> bool {
        int spins = 0;
        if (poll_out && seen < need) {
            const unsigned got = (unsigned)__builtin_amdgcn_readfirstlane((int)poll_v);
            seen = got > seen ? got : seen;
        }
        poll_out = false;
        /* blocked: resume only when the row above is `slack` macroblocks further than needed (never more than its end) */
        const unsigned slack = (unsigned)a.slack & 0xfffu;
        const unsigned want = seen < need ? ((need + slack) < (unsigned)a.mbcols ? need + slack : (unsigned)a.mbcols) : need;
        while (seen < want) {
            seen = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(prog_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (seen >= want) break;
            /* every exit of this loop is taken by the WHOLE wave: the abort word is read through readfirstlane like the progress
             * counter, so `ok` at the call sites is uniform by construction, not by the loads of 64 lanes happening to agree */
            if ((spins & 15) == 15 && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&a.ctrl[FFHIP_VP8_CTRL_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return false; /* given up elsewhere: whoever did has said why */
            if (++spins > VP8_SPIN_LIMIT) {
                if (lane == 0) {
                    __hip_atomic_store(&a.ctrl[FFHIP_VP8_CTRL_ABORT], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.async_err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                return false;
            }
            if (spins < 16) __builtin_amdgcn_s_sleep(1);
            else __builtin_amdgcn_s_sleep(16);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); /* ordering only */
        /* the part's share of the macroblock's 768 residual bytes: 8 per lane of the first 512 (luma), 4 per lane of the last 256 */
        if (PART == 0) {
            const u32x3 r3 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(rRes, lane * 12, (int)(rrow * 768), 0));
            f.res[0] = r3[0]; f.res[1] = r3[1]; f.res[2] = r3[2];
        } else if (PART == 1) {
            const u32x2 r2 = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rRes, lane * 8, (int)(rrow * 768), 0));
            f.res[0] = r2[0]; f.res[1] = r2[1];
        } else {
            f.res[0] = (u32)__builtin_amdgcn_raw_buffer_load_b32(rRes, 512 + lane * 4, (int)(rrow * 768), 0);
        }
        f.mo = (u32)__builtin_amdgcn_raw_buffer_load_b32(rMo, (lane < 5 ? lane : 4) * 4, x1 * 20, 0);
        /* borders: device-coherent loads (the row above is another wave's output); offsets outside the
         * plane -- "bytes before the plane" included -- read as 0 by the buffer range check */
        const int org = row_org + x1 * 16, corg = row_corg + x1 * 8;
        if (PART != 2) {
            /* the raw left column (lanes 48-63) is read from memory at x = 0 only -- everywhere else it is the previous macroblock's
             * right column, carried over in LDS: pointed outside the plane the sixteen lanes cost no memory request (they were sixteen
             * device-coherent 64-byte requests per macroblock, four fifths of the kernel's uncached reads) */
            f.a = ffhip_load_u8_sc1(rY, lane_select_vmask(x1 != 0 ? M_LEFT : 0ull, L.offY + org, (int)0x80000000u));
        }
        if (PART != 1) {
            f.b = ffhip_load_u8_sc1(rU, L.offU + corg);
            f.c = ffhip_load_u8_sc1(rV, L.offV + corg);
        }
        if (seen < (unsigned)a.mbcols) { /* the row above is not known to be finished: next macroblock's poll, not waited for */
            poll_v = __hip_atomic_load(prog_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            poll_out = true;
        }
        return true;
    };

    /* prologue: macroblock 0 -- its y mode decides how much of the row above the luma needs.
     * Fetches run ONE macroblock ahead, into the registers the consumed fetch has just left: the loads are issued right
     * behind the consume step and have the whole prediction of the macroblock to arrive.  (The first form ran two ahead
     * through three register sets rotated by copies at the end of the iteration -- and a copy of a register with a load
     * in flight waits for the load: every macroblock paid a trip to memory.) */
    /* the residual row of macroblock x1: with a map, its entry was loaded when x1 - 1 was fetched (loaded where it is used it
     * would be a dependent load in front of the residual's -- and, worse, the compiler then guards the map-less path with a
     * wait for ALL outstanding memory operations, i.e. for the stores of the macroblock just finished) */
    /* (round 3) ... and as a vector load its register was carried round the loop: in one of the three forms of this function the
     * compiler rotated it with a copy at the loop's end -- a copy of a register with a load in flight waits for ALL outstanding
     * memory operations, i.e. the chroma rows paid a trip to memory per macroblock (0.7 us where their work is 0.3).  The entry is
     * wave-uniform input data: a SCALAR load, issued and waited for in one statement (the compiler may copy the result register
     * the moment the statement ends), a macroblock before its entry is needed: ~0.1 us per macroblock, for callers with a map only. */
    auto map_load = [&](int x1) {
        int v;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(maprow + x1) : "memory");
        return v;
    };
    int map_next = 0;
    if (maprow) map_next = map_load(0);
    auto res_row = [&](int x1) {
        long long r = (long long)y * a.mbcols + x1;
        if (maprow) {
            r = (long long)map_next;
            if (x1 + 1 < a.mbcols) map_next = map_load(x1 + 1);
        }
        return r;
    };
    /* luma reads above-right: macroblock x + 1 of the row above; chroma its own column and the corner only: macroblock x */
    auto need_of = [&](int x1) { return y == 0 ? 0u : (unsigned)(x1 + (PART != 2 ? 2 : 1) < a.mbcols ? x1 + (PART != 2 ? 2 : 1) : a.mbcols); };
    const int ymode0 = __builtin_amdgcn_readfirstlane((int)mrow[0]);
    Vp8Fetch f;
    if (!fetch(0, res_row(0), (PART != 2 && y > 0 && ymode0 == 3) ? (unsigned)a.mbcols : need_of(0), f)) return false;
    if (tr && lane == 0) tr[1] = wall_clock64();
    /* The fetch of macroblock x + 1 is CONSUMED at the end of macroblock x -- when x's samples are in registers, in front of x's
     * stores -- not at the top of x + 1.  At the loop's top the wait for the fetched registers was a wait for everything: the
     * compiler takes the minimum over the ways into the loop head, the prologue has nothing in flight behind its fetch, so every
     * macroblock waited for the stores it had issued a moment ago to COMPLETE (device-coherent write-through: the better part of a
     * microsecond).  Here the only operation behind the fetch is its poll, and the stores have a whole macroblock to land before
     * anything waits on this wave's memory counter again.  The row counter's proof stands: the fetch consumed at the end of x - 1
     * was issued behind the stores of x - 2 (vector-memory operations of a wave complete in issue order). */
    u32 mo[5] = {0, 0, 0, 0, 0}; /* the 20 mode bytes of the macroblock at hand as five scalars */
    auto consume = [&](const int x) {
#pragma unroll
        for (int i = 0; i < 5; i++) mo[i] = (u32)__builtin_amdgcn_readlane((int)f.mo, i);
        const int ymode = (int)(mo[0] & 0xff);
        const bool raw = ymode == 2 || ymode == 3;
        /* ---- consume the fetch: residual and borders -> LDS, borders already in their final form (129 left of the
         * picture, 127 above it and right of it, predict.c:433-437, 492-517; raw memory for V_PRED / H_PRED) ---- */
        {
            const int carry = (int)BT[L.carry_src]; /* the previous macroblock's right column */
            const unsigned long long none = 0ull;
            if (PART == 0) {
                *(u32x3 *)((char *)R + lane * 12) = u32x3{f.res[0], f.res[1], f.res[2]};
                const unsigned long long m127 = (y == 0 ? (M_UTOP | M_VTOP | (raw ? none : M_LUMATOP)) : none) |
                                                ((!raw && x == a.mbcols - 1) ? M_TOPRIGHT : none);
                const unsigned long long m129 = (x == 0 ? (M_FIRST_CHROMA | (raw ? none : (M_FIRST_LUMA | M_LEFT))) : none) & ~m127;
                int v = f.a | f.b | f.c;
                v = lane_select_vmask(x != 0 ? M_LEFT : none, v, carry);
                v = lane_select_vmask(m127, v, 127);
                v = lane_select_vmask(m129, v, 129);
                BT[L.dst1] = (uint8_t)v;
                BT[L.dst2] = (uint8_t)(x == 0 ? 129 : carry); /* chroma left columns */
            } else if (PART == 1) {
                *(u32x2 *)((char *)R + lane * 8) = u32x2{f.res[0], f.res[1]};
                const unsigned long long m127 = (y == 0 && !raw ? M_LUMATOP : none) | ((!raw && x == a.mbcols - 1) ? M_TOPRIGHT : none);
                const unsigned long long m129 = (x == 0 && !raw ? (M_FIRST_LUMA | M_LEFT) : none) & ~m127;
                int v = f.a;
                v = lane_select_vmask(x != 0 ? M_LEFT : none, v, carry);
                v = lane_select_vmask(m127, v, 127);
                v = lane_select_vmask(m129, v, 129);
                BT[L.dst1] = (uint8_t)v; /* (lanes with a chroma role write into the chroma tiles nobody reads here) */
            } else {
                *(u32 *)((char *)R + 512 + lane * 4) = f.res[0];
                const unsigned long long m127 = y == 0 ? (M_UTOP | M_VTOP) : none;
                const unsigned long long m129 = (x == 0 ? M_FIRST_CHROMA : none) & ~m127;
                int v = f.b | f.c;
                v = lane_select_vmask(m127, v, 127);
                v = lane_select_vmask(m129, v, 129);
                BT[L.dst1] = (uint8_t)v;
                BT[L.dst2] = (uint8_t)(x == 0 ? 129 : carry); /* chroma left columns */
            }
        }
        wave_sync();
    };
    consume(0);
    for (int x = 0; x < a.mbcols; x++) {
        if (tr && lane == 0 && x == a.mbcols / 2) tr[2] = wall_clock64();
        if (tr) tp = wall_clock64();
        const int ymode = (int)(mo[0] & 0xff), uvmode = (int)((mo[0] >> 8) & 0xff);
        /* ---- move the row counter.  Vector-memory operations of a wave complete in issue order and
         * share one counter, so the fetch consumed at the end of the previous iteration (issued behind the stores
         * of macroblock x - 2) having returned means those stores have completed: no drain needed ---- */
        if (lane == 0 && x >= 2) __hip_atomic_store(prog_me, (unsigned)(x - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        /* ---- start the fetch of the next macroblock ---- */
        if (x + 1 < a.mbcols && !fetch(x + 1, res_row(x + 1), need_of(x + 1), f)) return false;

        if (tr) { const unsigned long long tn = wall_clock64(); ph1 += tn - tp; tp = tn; }
        const int org = row_org + x * 16, corg = row_corg + x * 8;
        u32 lumaout = 0;
        int outc[2] = {0, 0};
        if (PART != 2) {
            /* ---- luma ---- */
            const int r16 = lane >> 2, c16 = (lane & 3) * 4; /* this lane's 4 pixels of the macroblock */
            if (ymode == 4) { /* B_PRED: the 16 sub-blocks in 10 dependent steps */
                /* What a step costs a lone wave is its instructions, its taken branches (~8 instructions each) and its LDS
                 * round trips -- so a step has NO branch and ONE round trip: every step reads the eight bytes B_DC_PRED
                 * needs, the three taps of its own mode (B_TM_PRED's from row 8 of the table) and picks the result by two
                 * selects; tap addresses and residual values are in registers before the first step.  (Before: a mode
                 * switch of three scalar branches, two of them taken, and the residual read behind the taps: 215 ns a step.)
                 * And a sub-block needs its left, above and above-right neighbours only: sub-block (xs, ys) can run at time
                 * xs + 2 ys, which puts TWO sub-blocks into six of the ten steps -- lanes 0-15 take one, lanes 16-31 the
                 * other (lanes 32-63 repeat lanes 0-31: same addresses, same values, no exec masking). */
                static constexpr int SA[10] = {0, 1, 2, 3, 6, 7, 10, 11, 14, 15}, SB[10] = {0, 1, 4, 5, 8, 9, 12, 13, 14, 15};
                const int l16 = lane & 15, r = l16 >> 2, c = l16 & 3;
                const bool second = (lane & 16) != 0;
                int ta[10], tb[10], tc[10], rv[10], md[10], so[10];
#pragma unroll
                for (int t = 0; t < 10; t++) {
                    const int nA = SA[t], nB = SB[t];
                    const int modeA = (int)((mo[(2 + nA) >> 2] >> (8 * ((2 + nA) & 3))) & 0xff), modeB = (int)((mo[(2 + nB) >> 2] >> (8 * ((2 + nB) & 3))) & 0xff);
                    const int mode = second ? modeB : modeA;
                    const u32 to = TT[(mode < 10 ? mode : 2) * 16 + l16]; /* a mode past the table: the first directional row, as before */
                    const int oA = ((nA >> 2) * 4 + 1) * PRS + 4 + (nA & 3) * 4, oB = ((nB >> 2) * 4 + 1) * PRS + 4 + (nB & 3) * 4;
                    const int sb = second ? oB : oA; /* sub-block origin in the tile */
                    ta[t] = sb - 64 + (int)(to & 0xff); tb[t] = sb - 64 + (int)((to >> 8) & 0xff); tc[t] = sb - 64 + (int)(to >> 16);
                    rv[t] = (int)R[16 * (second ? nB : nA) + l16];
                    md[t] = mode; so[t] = sb;
                }
#pragma unroll
                for (int t = 0; t < 10; t++) {
                    uint8_t *S = T + so[t];
                    const int va = T[ta[t]], vb = T[tb[t]], vc = T[tc[t]];
                    const u32 top4 = *(const u32 *)(S - PRS);
                    const int l0 = S[-1], l1 = S[PRS - 1], l2 = S[2 * PRS - 1], l3 = S[3 * PRS - 1];
                    const int dir = (va + 2 * vb + vc + 2) >> 2;
                    const int tm = clamp255(va + vb - vc);
                    const int dc = (4 + sum4(top4) + l0 + l1 + l2 + l3) >> 3;
                    int p = md[t] == 1 ? tm : dir;
                    p = md[t] == 0 ? dc : p;
                    S[r * PRS + c] = (uint8_t)clamp255(p + rv[t]);
                    wave_sync();
                }
                lumaout = *(const u32 *)(T + (r16 + 1) * PRS + 4 + c16);
            } else {
                const u32 top4 = *(const u32 *)(T + 4 + c16);
                const int lf = T[(r16 + 1) * PRS + 3], cor = T[3];
                int dcv = 0;
                if (ymode == 0) { /* DC over the edges that exist (predict.c:34-76) */
                    int dc = 0;
                    if (x > 0) {
#pragma unroll
                        for (int k = 0; k < 16; k++) dc += T[(k + 1) * PRS + 3];
                    }
                    if (y > 0) dc += sum4(*(const u32 *)(T + 4)) + sum4(*(const u32 *)(T + 8)) + sum4(*(const u32 *)(T + 12)) + sum4(*(const u32 *)(T + 16));
                    if (x == 0 && y == 0) dc = 0x80;
                    else if (x == 0 || y == 0) dc = (dc + 8) >> 4;
                    else dc = (dc + 16) >> 5;
                    dcv = dc & 0xff;
                }
                /* the residual of 4 neighbouring pixels is 4 consecutive shorts */
                const s16x4 rs = *(const s16x4 *)(R + 16 * (4 * (r16 >> 2) + (c16 >> 2)) + 4 * (r16 & 3));
                u32 o = 0;
                /* the mode as lane masks and selects: written as if / else on the (wave-uniform) mode the compiler made it a
                 * chain of scalar branches per pixel -- a dozen taken branches per macroblock, ~8 instructions each for a lone wave */
                const unsigned long long is_dc = __builtin_amdgcn_ballot_w64(ymode == 0), is_v = __builtin_amdgcn_ballot_w64(ymode == 2),
                                         is_h = __builtin_amdgcn_ballot_w64(ymode == 3);
                const int lc = lf - cor;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int tpx = (int)((top4 >> (8 * k)) & 0xff);
                    int p = clamp255(tpx + lc);                  /* TM_PRED */
                    p = lane_select_vmask(is_h, p, lf);                /* raw dst[-1]   (predict.c:346-353) */
                    p = lane_select_vmask(is_v, p, tpx);               /* raw row above (predict.c:338-344) */
                    p = lane_select_vmask(is_dc, p, dcv);
                    o |= (u32)clamp255(p + rs[k]) << (8 * k);
                }
                wave_sync(); /* every lane has read its borders */
                *(u32 *)(T + (r16 + 1) * PRS + 4 + c16) = o;
                lumaout = o;
            }
            if (tr) { const unsigned long long tn = wall_clock64(); ph2 += tn - tp; tp = tn; }
        }
        if (PART != 1) {
            /* ---- chroma: one pixel of U and one of V per lane ---- */
            const int r = lane >> 3, c = lane & 7;
#pragma unroll
            for (int pl = 0; pl < 2; pl++) {
                const uint8_t *Cp = pl ? C1 : C0;
                const int lf = Cp[(r + 1) * PCS + 3], tpx = Cp[4 + c], cor = Cp[3];
                int p;
                if (uvmode == 0) {
                    int dc = 0;
                    if (x > 0) {
#pragma unroll
                        for (int k = 0; k < 8; k++) dc += Cp[(k + 1) * PCS + 3];
                    }
                    if (y > 0) dc += sum4(*(const u32 *)(Cp + 4)) + sum4(*(const u32 *)(Cp + 8));
                    if (x == 0 && y == 0) dc = 0x80;
                    else if (x == 0 || y == 0) dc = (dc + 4) >> 3;
                    else dc = (dc + 8) >> 4;
                    p = dc & 0xff;
                } else {
                    p = lane_select_vmask(__builtin_amdgcn_ballot_w64(uvmode == 1), lf, clamp255(lf + tpx - cor));
                    p = lane_select_vmask(__builtin_amdgcn_ballot_w64(uvmode == 2), p, tpx);
                }
                const int ri = 256 + 64 * pl + 16 * (2 * (r >> 2) + (c >> 2)) + 4 * (r & 3) + (c & 3);
                outc[pl] = clamp255(p + R[ri]);
            }
            wave_sync(); /* all border reads done before the tiles change */
            C0[(r + 1) * PCS + 4 + c] = (uint8_t)outc[0];
            C1[(r + 1) * PCS + 4 + c] = (uint8_t)outc[1];
        }
        wave_sync();
        if (tr) { const unsigned long long tn = wall_clock64(); ph3 += tn - tp; tp = tn; }
        /* ---- the next macroblock's residual and borders into LDS, then this one's samples out ---- */
        if (x + 1 < a.mbcols) consume(x + 1);
        if (PART != 2) __builtin_amdgcn_raw_buffer_store_b32(lumaout, rY, L.lumaY_lane, org, FFHIP_AUX_SC1);
        if (PART != 1) {
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)outc[0], rU, L.chroma_lane, corg, FFHIP_AUX_SC1);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)outc[1], rV, L.chroma_lane, corg, FFHIP_AUX_SC1);
        }
        if (tr) ph0 += wall_clock64() - tp;
    }
    /* ---- the row is complete once its last stores are ---- */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the fence's own wait can be optimised away (MI355X_MICROARCH.md, compiler hazard) */
    if (lane == 0) __hip_atomic_store(prog_me, (unsigned)a.mbcols, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tr && lane == 0) { tr[3] = wall_clock64(); tr[4] = ph0; tr[5] = ph1; tr[6] = ph2; tr[7] = ph3; }
    return true;
}

template <bool TRACE>
__global__ __launch_bounds__(64) void k_vp8_predict_rows(Vp8PredArgs a)
{
    /* one array for the luma tile T (17 rows of PRS), the chroma tiles (9 rows of PCS each) and a dump cell, so that a lane's
     * border byte goes out with ONE store whatever its role */
    __shared__ __attribute__((aligned(16))) uint8_t BT[BT_DUMP + 16];
    __shared__ __attribute__((aligned(16))) short R[384];
    __shared__ u32 TT[10 * 16]; /* indexed by the sub-block mode itself: row 0 B_DC_PRED (no taps: any valid cell), row 1 B_TM_PRED's (left, above, corner), rows 2-9 the directional modes' */
    uint8_t *const T = BT;
    const int lane = threadIdx.x;
    Vp8Lane L;
    L.n_mb = a.mbcols * a.mbrows;
    L.ys = 16 * a.mbcols; L.us = 8 * a.mbcols;
    const int ys = L.ys, us = L.us;

    /* B_PRED taps of this lane's pixel as tile byte offsets from the sub-block origin, biased by 64:
     * edge e[k] of predict.c's L K J I X A..H sits at (3-k) rows down / one left, the corner, or k-5 along the row above */
    u32 tapoff[8];
    {
        auto off = [](int k) { return k < 4 ? (3 - k) * PRS - 1 : (k == 4 ? -PRS - 1 : -PRS + (k - 5)); };
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const unsigned t = kVp8Taps[m][lane & 15];
            tapoff[m] = (u32)(off((int)(t & 15)) + 64) | ((u32)(off((int)((t >> 4) & 15)) + 64) << 8) | ((u32)(off((int)(t >> 8)) + 64) << 16);
        }
    }
    /* above-right of the sub-blocks in column 3 below the first row: always 127 (predict.c:509-517) */
    if (lane < 12) T[(4 + 4 * (lane >> 2)) * PRS + 20 + (lane & 3)] = 127;
    /* the tap words again as a table in LDS, [directional mode][pixel]: a B_PRED macroblock looks up the words of its
     * sixteen sub-blocks at once, in front of the sixteen dependent steps -- picking them inside each step was seven
     * compares and seven selects on the chain (a lone wave pays ~8 cycles an instruction, profiles/r2_lone_wave.txt) */
    if (lane < 16) {
#pragma unroll
        for (int m = 0; m < 8; m++) TT[(m + 2) * 16 + lane] = tapoff[m];
        const int r = lane >> 2, c = lane & 3;
        TT[16 + lane] = (u32)(r * PRS - 1 + 64) | ((u32)(-PRS + c + 64) << 8) | ((u32)(-PRS - 1 + 64) << 16);
        TT[lane] = 64u | (64u << 8) | (64u << 16);
    }
    wave_sync();

    /* what a lane does with the borders, by its number (see Vp8Fetch::a): offsets of its byte from the macroblock's first
     * luma / chroma pixel in the three planes (lanes without that role: far outside any plane -- the buffer range check
     * returns 0 and the loads can simply be OR-ed), where the byte goes in the tile array, and for the lanes that
     * carry the previous macroblock's right column over as this one's left column, where they take it from */
    const int OUT = (int)0x80000000u;
    L.offY = lane <= 20 ? lane - 1 - ys : (lane >= 48 ? (lane - 48) * ys - 1 : OUT);
    L.offU = lane >= 21 && lane <= 29 ? lane - 22 - us : OUT;
    L.offV = lane >= 32 && lane <= 40 ? lane - 33 - us : OUT;
    L.dst1 = lane <= 20 ? 3 + lane : (lane <= 29 && lane >= 21 ? BT_C0 + 3 + (lane - 21) : (lane >= 32 && lane <= 40 ? BT_C1 + 3 + (lane - 32) :
             (lane >= 48 ? (lane - 47) * PRS + 3 : BT_DUMP)));
    /* chroma left columns: lanes 0..15 = plane (lane >> 3), row (lane & 7) */
    L.dst2 = lane < 16 ? (lane < 8 ? BT_C0 : BT_C1) + ((lane & 7) + 1) * PCS + 3 : BT_DUMP;
    L.carry_src = lane >= 48 ? (lane - 47) * PRS + 4 + 15 : (lane < 16 ? (lane < 8 ? BT_C0 : BT_C1) + ((lane & 7) + 1) * PCS + 4 + 7 : BT_DUMP);
    L.lumaY_lane = (lane >> 2) * ys + (lane & 3) * 4; L.chroma_lane = (lane >> 3) * us + (lane & 7);

    /* Tickets per part: (row index, image), row index major, so whatever a row waits for -- the same part of the row above -- has a
     * smaller ticket of the same counter and is running or done.  Split: two waves in five start on the chroma rows (a third of the luma rows' work, but a chroma
     * row follows the row above at one macroblock, so as many of them are in flight: with one wave in four the chroma finished 0.25 ms
     * behind the luma of 16 frames); a wave that finds its part's tickets gone takes the other part's, so any grid size finishes
     * both.  Not split (PART 0): a wave walks both parts of its row -- fewer device-coherent requests per macroblock, what a
     * chip-filling batch is bound by.  (One loop nest for the three forms, left by `break`: with a loop of its own per form, left
     * by `return`, the compiler's restructured control flow never terminated -- twice, in two different arrangements.) */
    const bool chroma_first = (0xAu >> (blockIdx.x % 5u)) & 1u; /* waves 1 and 3 of every five */
    bool alive = true;
    for (int pass = 0; pass < 2 && alive; pass++) {
        if (pass == 1 && (!a.split || chroma_first)) break; /* the waves that began on the luma rows finish what chroma is left (a grid of one wave
                                                               has no other); a chroma wave joining the luma rows late would only hold a ticket far from
                                                               its turn and poll (33 instead of 25 rows per image in flight: 16 frames 1.07 against 0.98 ms) */
        const int part = a.split ? (chroma_first != (pass == 1) ? 2 : 1) : 0;
        uint32_t *const counter = &a.ctrl[part == 2 ? FFHIP_VP8_CTRL_TICKET_C : 0];
        for (;;) {
            unsigned ticket = 0;
            if (lane == 0) ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
            if (ticket >= (unsigned)(a.n_images * a.mbrows)) break;
            const int y = (int)(ticket / (unsigned)a.n_images), img = (int)(ticket % (unsigned)a.n_images);
            bool ok;
            if (part == 0) ok = vp8_row<TRACE, 0>(a, L, lane, y, img, BT, R, TT);
            else if (part == 2) ok = vp8_row<TRACE, 2>(a, L, lane, y, img, BT, R, TT);
            else ok = vp8_row<TRACE, 1>(a, L, lane, y, img, BT, R, TT);
            if (!__builtin_amdgcn_readfirstlane((int)ok)) { alive = false; break; }
        }
    }
}

/* ------------------------------------------------------------------------ host */

/* Mode records that are not VP8's (vp8_mode_record_valid) for batches too large for a host pass: one thread per record in FRONT of the
 * kernel that reads them.  Checked inside the row kernel's macroblock loop -- one branch that is never taken -- it cost 9 % on 16 frames
 * of random modes.  Both kernels write vp8_mode_record_valid's rule out: called as the predicate it compiled to more scalar (32 -> 37) or
 * vector registers (8 -> 17) in every form tried; tests/test_vp8_items_gpu.py holds the kernels to the predicate record by record. */
/* Refuse the call through the stream: a ticket counter beyond every row (words 0 and idx_c) sends each wave of the kernel behind home at
 * once, at no cost to a valid call (a look at the abort word per row cost a 1024-frame call 4 %); the frame kernels read word idx_abort. */
__device__ __forceinline__ void vp8_refuse_call(uint32_t *ctrl, int *async_err, const uint32_t idx_c, const uint32_t idx_abort)
{
    __hip_atomic_store(&ctrl[0], 0x7fffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctrl[idx_c], 0x7fffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctrl[idx_abort], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(async_err, FFHIP_ASYNC_BAD_INPUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
/* the records of one array (20-byte records, 4-byte aligned) */
__global__ __launch_bounds__(256) void k_vp8_check_modes(const uint8_t *modes, long long n_records, uint32_t *ctrl, int *async_err, uint32_t idx_c, uint32_t idx_abort)
{
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_records; i += (long long)gridDim.x * 256) {
        const uint32_t *rec = (const uint32_t *)(modes + i * 20);
        const uint32_t m = rec[0];
        bad |= (m & 0xffu) > 4u || ((m >> 8) & 0xffu) > 3u;
        if ((m & 0xffu) == 4u) {
            auto over9 = [](uint32_t w) { return ((w | (((w & 0x0f0f0f0fu) + 0x06060606u))) & 0xf0f0f0f0u) != 0u; };
            bad |= over9(m >> 16) || over9(rec[1]) || over9(rec[2]) || over9(rec[3]) || over9(rec[4] & 0xffffu);
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) && (threadIdx.x & 63) == 0) vp8_refuse_call(ctrl, async_err, idx_c, idx_abort);
}
/* the records of ffhip_vp8_decode_items' items without a host copy, one launch for all of them: a record's item is found by a search over
 * the items' prefix (the sentinel behind the last one holds the total); the frame kernels' four-word header */
__global__ __launch_bounds__(256) void k_vp8_check_modes_items(const Vp8CheckItem *items, int n, long long n_records, uint32_t *ctrl, int *async_err)
{
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_records; i += (long long)gridDim.x * 256) {
        int lo = 0, hi = n; /* items[lo].first <= i < items[hi].first */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].first <= i) lo = mid;
            else hi = mid;
        }
        const uint32_t *rec = (const uint32_t *)(items[lo].modes + (i - items[lo].first) * 20);
        const uint32_t m = rec[0];
        bad |= (m & 0xffu) > 4u || ((m >> 8) & 0xffu) > 3u;
        if ((m & 0xffu) == 4u) {
            auto over9 = [](uint32_t w) { return ((w | (((w & 0x0f0f0f0fu) + 0x06060606u))) & 0xf0f0f0f0u) != 0u; };
            bad |= over9(m >> 16) || over9(rec[1]) || over9(rec[2]) || over9(rec[3]) || over9(rec[4] & 0xffffu);
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) && (threadIdx.x & 63) == 0) vp8_refuse_call(ctrl, async_err, 2u, 1u);
}
static unsigned check_modes_grid(long long n_records) { return (unsigned)std::min<long long>((n_records + 255) / 256, 4096); }
/* for the frame kernel of ffhip_vp8_frame.hip, whose header is four words (0 and 2 unused, 1 the abort word: nobody polls it) */
extern "C" int ffhip_vp8_check_modes_enqueue(const uint8_t *d_modes, long long n_records, uint32_t *ctrl, int *async_err, void *stream)
{
    hipLaunchKernelGGL(k_vp8_check_modes, dim3(check_modes_grid(n_records)), dim3(256), 0, (hipStream_t)stream, d_modes, n_records, ctrl, async_err, 2u, 1u);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}
int vp8_check_modes_items_enqueue(const Vp8CheckItem *d_items, int n, long long n_records, uint32_t *ctrl, int *async_err, void *stream)
{
    hipLaunchKernelGGL(k_vp8_check_modes_items, dim3(check_modes_grid(n_records)), dim3(256), 0, (hipStream_t)stream, d_items, n, n_records, ctrl, async_err);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}
extern "C" int ffhip_vp8_modes_ok_host(const uint8_t *h_modes, long long n_records)
{
    for (long long i = 0; i < n_records; i++)
        if (!vp8_mode_record_valid(h_modes + i * 20)) return 0;
    return 1;
}

static unsigned long long *g_vp8_trace = nullptr;
/* diagnostics: a device buffer of 8 x n_images x mbrows u64 the row kernel stamps (tests/tools/diag_vp8_row_trace.py); NULL = off */
extern "C" void ffhip_debug_vp8_trace(void *d_buf) { g_vp8_trace = (unsigned long long *)d_buf; }

Vp8RowSwitches vp8_row_switches(const char *mode, const Vp8SideBySide *sbs)
{
    Vp8RowSwitches sw;
    sw.async_err = (mode && !strcmp(mode, "levels")) ? nullptr : ffhip_async_err_word();
    if (sw.async_err && sbs && sbs->err_word) sw.async_err = sbs->err_word; /* the side-by-side call's own word (ffhip_vp8_lf.hip) */
    const char *ps = FFHIP_ENV("FFHIP_VP8_PROGRESS_SHIFT"), *sl = FFHIP_ENV("FFHIP_VP8_SLACK");
    sw.pshift = ps ? std::min(5, std::max(0, atoi(ps))) : 5;
    sw.slack = sl ? std::max(0, atoi(sl)) : 0;
    return sw;
}
int vp8_levels_upload_and_launch(int scratch_kind, void *stream, const std::vector<std::vector<uint32_t>> &lists,
                                 const std::function<void(const uint32_t *work, int count)> &launch)
{
    size_t total = 0;
    for (auto &l : lists) total += l.size();
    uint32_t *g_work = ffhip_scratch(scratch_kind, stream, total);
    if (!g_work) return FFHIP_ENOMEM;
    std::vector<uint32_t> flat;
    flat.reserve(total);
    for (auto &l : lists) flat.insert(flat.end(), l.begin(), l.end());
    FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO); /* the work buffer may still be in use by an earlier call */
    FFHIP_CHECK(hipMemcpy(g_work, flat.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice), FFHIP_EIO);
    size_t off = 0;
    for (auto &l : lists) {
        if (!l.empty()) launch(g_work + off, (int)(l.size() / 2));
        off += l.size();
    }
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

/* row form (default): no host-side scheduling at all, one launch.  `a`: the common fields */
static int pred_rows_enqueue(Vp8PredArgs a, int n_images, const uint8_t *h_modes, const Vp8RowSwitches &sw, void *stream, Vp8SideBySide *sbs)
{
    hipStream_t st = (hipStream_t)stream;
    const int mbcols = a.mbcols, mbrows = a.mbrows;
    const long long recs = (long long)mbcols * mbrows * n_images;
    /* mode bytes out of range: refused here, synchronously, for batches of up to 2^17 macroblocks; beyond that the
     * host pass would cost more than the launch it guards (8 M records for 1024 frames), and a kernel in front of the row
     * kernel refuses the call through the stream (k_vp8_check_modes: nothing is written, ffhip_stream_sync returns FFHIP_EINVAL) */
    const bool host_checked = recs <= (1LL << 17);
    if (host_checked && !ffhip_vp8_modes_ok_host(h_modes, recs)) return FFHIP_EINVAL;
    const size_t words = FFHIP_VP8_CTRL_HDR + ((2 * (size_t)n_images * (size_t)mbrows) << sw.pshift); /* tickets, abort; the rows' luma counters, then their chroma counters */
    uint32_t *g_work = ffhip_scratch(SCRATCH_VP8_PRED, stream, words);
    if (!g_work) return FFHIP_ENOMEM;
    FFHIP_CHECK(hipMemsetAsync(g_work, 0, words * sizeof(uint32_t), st), FFHIP_EIO);
    if (!host_checked) { /* IN FRONT of the fork: enqueued behind it, the side-by-side filter kernel became resident a kernel ahead of the
                            prediction it waits for, and a 1024-frame call took a third longer (12.1 -> 16.6 ms for the two stages) */
        hipLaunchKernelGGL(k_vp8_check_modes, dim3(check_modes_grid(recs)), dim3(256), 0, st, a.modes, recs, g_work, sw.async_err, (uint32_t)FFHIP_VP8_CTRL_TICKET_C, (uint32_t)FFHIP_VP8_CTRL_ABORT);
    }
    if (sbs) { /* the loop filter of the same call starts behind this point, on its own stream */
        FFHIP_CHECK(hipEventRecord(sbs->fork, st), FFHIP_EIO);
        sbs->pred_progress = g_work + FFHIP_VP8_CTRL_HDR;
        sbs->pshift = sw.pshift;
    }
    a.ctrl = g_work; a.async_err = sw.async_err; a.n_images = n_images; a.pshift = sw.pshift; a.slack = sw.slack;
    a.trace = g_vp8_trace;
    /* How many waves: as many as can be RESIDENT (occupancy x CUs; half of that next to the loop-filter kernel of the same
     * call, so that the two always fit side by side whichever the hardware starts first), but never more rows per image
     * than its wavefront is wide -- a row trails the row above by four macroblocks, so mbcols / 4 + 2 rows of an image can
     * be at work at once; a wave beyond that holds a ticket far from its turn and only polls (16 x 1080p: 2048 waves
     * 5.62 / 2.10 ms, 256 waves 5.48 / 1.96 -- tests/tools/bench_stages.py).  One wave per SIMD issues an instruction every
     * 5-8 cycles (profiles/r2_lone_wave.txt); the co-resident waves of OTHER images fill those slots, which is where the
     * throughput of a large batch comes from (tests/tools/bench_vp8_batch_sweep.py). */
    const char *wv = FFHIP_ENV("FFHIP_VP8_PRED_WAVES");
    /* measured (256 x 1080p, tests/tools/diag_vp8_batch_waves.py, diag_vp8_batch_grid.py): the kernel gains up to three waves per
     * SIMD and loses beyond (2048 / 3072 / 4096 waves: 2.56 / 2.45 / 2.56 ms); next to the loop filter three quarters of the
     * residency are the prediction's -- it is the longer chain -- and a quarter of its own the filter's: together they still fit */
    long long resident = ffhip_resident_waves((const void *)k_vp8_predict_rows<false>, 64);
    resident = std::max<long long>(1, resident - resident / 4);
    const long long rows_wide = (long long)n_images * (mbcols / 5 + 1); /* measured, 16 x 1080p of the encoder's stream next to the filter: 16 / 24 / 32 rows per image 1.19 / 1.12 / 1.18 ms */
    /* Luma and chroma as rows of their own (other waves) take the chroma off the chain a frame hangs on -- one frame 0.93 -> 0.84 ms --
     * at the price of 14 device-coherent requests per macroblock instead of 10 (modes, poll and counter twice) and of as many
     * chroma rows in flight as luma rows (a chroma row follows the row above at one macroblock).  Measured, whole chain on the
     * encoder's stream, split against not: 1 frame 0.84 / 0.92 ms, 16 frames 1.16 / 1.15, 64 frames 2.55 / 1.97, 256 frames 6.7 / 5.4.
     * So: split while the launch is at its minimum size anyway (a handful of frames), not beyond. */
    const char *sp = FFHIP_ENV("FFHIP_VP8_PRED_SPLIT");
    a.split = sp ? (atoi(sp) != 0) : (rows_wide * 5 / 3 <= 256);
    const long long wide = std::max<long long>(256, a.split ? rows_wide * 5 / 3 : rows_wide);
    const long long cap = wv ? std::max(1, atoi(wv)) : std::min(resident, wide);
    const unsigned waves = (unsigned)std::min<long long>((a.split ? 2LL : 1LL) * n_images * mbrows, cap);
    if (sbs) sbs->pred_split = a.split;
    if (a.trace) hipLaunchKernelGGL(k_vp8_predict_rows<true>, dim3(waves), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k_vp8_predict_rows<false>, dim3(waves), dim3(64), 0, st, a);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

/* levels form (fallback, A/B): one launch per wavefront level */
static int pred_levels_enqueue(Vp8PredArgs a, int n_images, const uint8_t *h_modes, void *stream)
{
    const int mbcols = a.mbcols, mbrows = a.mbrows;
    const long long n_mb = (long long)mbcols * mbrows;
    /* before anything is enqueued, as the row form's host check: k_vp8_predict indexes kVp8Taps with a B_PRED sub-block mode */
    if (!ffhip_vp8_modes_ok_host(h_modes, n_mb * n_images)) return FFHIP_EINVAL;
    /* wavefront levels: left, above, above-left, above-right -- plus the reference's wrapped
     * read of H_PRED at x = 0, which sees the last pixel of the previous pixel row
     * (predict.c:346-353), i.e. the last macroblock of the row above */
    std::vector<int> level((size_t)n_mb);
    std::vector<std::vector<uint32_t>> lists;
    for (int img = 0; img < n_images; img++) {
        const uint8_t *mo = h_modes + (size_t)img * n_mb * 20;
        for (int y = 0; y < mbrows; y++)
            for (int x = 0; x < mbcols; x++) {
                int lv = 0;
                auto dep = [&](int dx, int dy) { if (dx >= 0 && dx < mbcols && dy >= 0) lv = std::max(lv, level[(size_t)dy * mbcols + dx] + 1); };
                dep(x - 1, y); dep(x, y - 1); dep(x - 1, y - 1); dep(x + 1, y - 1);
                if (x == 0 && y > 0 && mo[((size_t)y * mbcols) * 20] == 3) dep(mbcols - 1, y - 1);
                level[(size_t)y * mbcols + x] = lv;
                if ((size_t)lv >= lists.size()) lists.resize((size_t)lv + 1);
                lists[(size_t)lv].push_back((uint32_t)img);
                lists[(size_t)lv].push_back((uint32_t)(y * mbcols + x));
            }
    }
    return vp8_levels_upload_and_launch(SCRATCH_VP8_PRED, stream, lists, [&](const uint32_t *work, int count) {
        a.work = work; a.count = count;
        hipLaunchKernelGGL(k_vp8_predict, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    });
}

/* the prediction's argument check, made before the device is asked for and before anything is enqueued (ffhip_vp8_predict_loopfilter makes it
 * in front of the kernel that saves the last luma column).  n_images 0 passes whatever the pointers are: nothing to do */
int vp8_predict_args_check(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                           int64_t residual_stride, const uint8_t *d_y, const uint8_t *d_u, const uint8_t *d_v)
{
    if (mbcols <= 0 || mbrows <= 0 || n_images < 0) return FFHIP_EINVAL;
    if (n_images == 0) return FFHIP_OK;
    if (!h_modes || !d_modes || !d_residual || !d_y || !d_u || !d_v) return FFHIP_EINVAL;
    if (((uintptr_t)d_residual & 3) || ((uintptr_t)d_y & 3) || (residual_stride & 1)) return FFHIP_EINVAL;
    if ((long long)mbcols * mbrows * n_images > 0x3fffffffLL) return FFHIP_EINVAL;
    return FFHIP_OK;
}

/* sbs: next to the loop filter of the same call (ffhip_vp8_predict_loopfilter), which starts behind the counter reset */
int vp8_predict_recon_impl(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                           int64_t residual_stride, const int32_t *d_resmap, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y,
                           int64_t plane_stride_uv, void *stream, Vp8SideBySide *sbs)
{
    const int bad = vp8_predict_args_check(mbcols, mbrows, n_images, h_modes, d_modes, d_residual, residual_stride, d_y, d_u, d_v);
    if (bad || n_images == 0) return bad;
    const long long n_mb = (long long)mbcols * mbrows;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    { /* (the self-healing record of a side-by-side call is good while that call is the stream's last: ffhip_vp8_lf.hip) */
        std::lock_guard<std::mutex> l(g_ffhip_state_mu);
        ffhip_stream_state(stream)->vp8_seq++;
    }
    Vp8PredArgs a = {}; /* the fields both forms read */
    a.modes = d_modes; a.residual = d_residual; a.resmap = d_resmap;
    a.y = d_y; a.u = d_u; a.v = d_v;
    a.plane_y = plane_stride_y; a.plane_uv = plane_stride_uv; a.res_stride = residual_stride;
    a.mbcols = mbcols; a.mbrows = mbrows;
    const Vp8RowSwitches sw = vp8_row_switches(FFHIP_ENV("FFHIP_VP8_PRED_MODE"), sbs);
    if (sw.async_err && !((uintptr_t)d_modes & 3) && n_mb < (1LL << 23) /* 32-bit byte offsets into a plane */)
        return pred_rows_enqueue(a, n_images, h_modes, sw, stream, sbs);
    return pred_levels_enqueue(a, n_images, h_modes, stream);
}
extern "C" int ffhip_vp8_predict_recon(int mbcols, int mbrows, int n_images, const uint8_t *h_modes,
                                       const uint8_t *d_modes, const int16_t *d_residual, int64_t residual_stride,
                                       const int32_t *d_resmap, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                                       int64_t plane_stride_y, int64_t plane_stride_uv, void *stream)
{
    return vp8_predict_recon_impl(mbcols, mbrows, n_images, h_modes, d_modes, d_residual, residual_stride, d_resmap, d_y, d_u, d_v, plane_stride_y,
                                  plane_stride_uv, stream, nullptr);
}
