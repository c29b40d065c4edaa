/*
 * ffhip_vp8_frame.hip -- the THROUGHPUT form of the VP8 key-frame chain: the frame loop of vp8_decode
 * (format/webp.c:1833-1868) for a batch of frames as ONE kernel,
 *   vp8_prerdict_mb        -> pred_luma / pred_chrome + add_residue    format/predict.c:426-645, 378-389
 *   loopfilter             -> the four edge steps per macroblock       format/webp.c:1686-1752 (1480-1684)
 *   YUV420_to_BGRA32       -> BGRA                                     utils/colorspace.c:291-329 (webp.c:1868)
 * bit-exact with the three separate stages (ffhip_vp8_predict_recon, ffhip_vp8_loopfilter, ffhip_yuv420_to_bgra).
 *
 * The row kernels of ffhip_vp8_pred.hip / ffhip_vp8_lf.hip are latency designs: one wave per macroblock row of ANY frame,
 * rows of a frame found by ticket, every hand-off between rows through device-coherent (sc1) memory, three passes over the
 * planes (prediction writes them, the filter re-reads and re-writes them, the colour kernel re-reads them: 19.4 B per pixel).
 * With hundreds of frames in a call that form is bound by the rate of uncached requests, not by
 * arithmetic.  Frames do not depend on each other, so here
 *
 *   - ONE WORKGROUP owns a frame (then the next one of its share): its NW waves take the frame's macroblock rows round-robin,
 *     row y following row y - 1 at two to three macroblocks.  The rows of a frame always meet inside one CU: progress
 *     counters live in LDS, nothing is device-coherent, no wave ever waits for a wave that may not be resident -- there is
 *     no ticket, no bounded-wait give-up on a busy device, no side stream.
 *   - ONE WAVE does everything for its macroblock: prediction + residual, THEN the loop filter, THEN the colour conversion.
 *     The filter may not run ahead of the prediction of the neighbours (predict.c reads unfiltered samples, the filter
 *     rewrites up to three samples beyond each edge), which is why the row kernels keep the filter a row behind.  Here the wave
 *     keeps what later predictions read -- the unfiltered bottom row (for the row below) and right column (for the next
 *     macroblock: it never leaves the prediction tile in LDS) -- apart from the tile it filters.
 *   - what a row hands DOWN is two line buffers per row (global scratch, 192 B per macroblock, L2-resident, written and read
 *     by the same CU: workgroup-scope coherence, plain loads and stores): the unfiltered bottom sample row of each plane, and
 *     the bottom six luma / four chroma rows as filtered so far -- the row below applies its top-edge filter to them and
 *     emits them.  A full row of lines, not a ring: the reference's wrapped H_PRED read at x = 0 (predict.c:346-353: the
 *     sample left of a row's first pixel is the last pixel of the row above) makes a row wait for the WHOLE row above, and a
 *     producer that could block on its consumer would deadlock there.
 *   - every sample is written ONCE, as BGRA, after its last filter touch: macroblock (x, y) emits the 16 x 16 pixels at
 *     offset (-8, -6) from its own origin (columns up to x*16 + 12 and rows up to y*16 + 12 are final once (x, y) is filtered;
 *     4:2:0 pairs make it -8 / -6), with one extra column / row iteration at the right / bottom picture edge.  Residual in
 *     (3 B per pixel), BGRA out (4 B per pixel): 7 B per pixel plus the lines, where the three stages move 19.4.
 *
 * Small batches stay with the row kernels (a frame's critical path is shorter there: more rows of ONE frame in flight
 * than a workgroup has waves); the host entry ffhip_vp8_decode_frames picks by batch size (FFHIP_VP8_FRAMES forces either).
 */
#include "ffhip_colorterms.h"
#include "ffhip_vp8_filters.h"
#include "ffhip_vp8_bool.h"

#include <algorithm>
#include <queue>
#include <vector>
#include <stdlib.h>
#include <string.h>

struct Vp8FrameArgs {
    const uint8_t *modes;    /* [n_images][n_mb][20]                                          */
    const int16_t *residual; /* [n_images][res_rows][384]                                     */
    const int32_t *resmap;   /* [n_images][n_mb] or NULL                                      */
    const uint8_t *filters;  /* [4][2][3] sub_limit, inter_limit, hev_thresh (NULL: type 0)   */
    uint8_t *bgra;           /* [n_images] images of 16*mbrows rows, `pitch` bytes apart       */
    uint8_t *y, *u, *v;      /* optional: the filtered planes as well (NULL: not written)      */
    uint8_t *lines;          /* scratch: [gridDim.x][nslot][slot_bytes]                        */
    const uint32_t *ctrl;    /* [1] != 0: the mode check in front refused the call            */
    int *async_err;
    long long res_stride, image_stride, plane_y, plane_uv;
    int pitch, mbcols, mbrows, n_images, nslot;
    unsigned slot_bytes;
};

#define FR_SPIN_LIMIT (1 << 22)
/* one wave's LDS arena (tile strides, tile offsets and lane masks: ffhip_vp8_device.h; the filter tiles here have 6 rows above and 8 columns left
 * for luma, 4 and 4 for chroma) */
#define AR_BT 0      /* 784 B: prediction tiles + dump cell                         */
#define AR_R 800     /* 768 B: the macroblock's residual                            */
#define AR_TL 1568   /* 22 x 24 B: luma filter tile                                 */
#define AR_TC0 2096  /* 20 x 24 B each (12 rows in use; filter_phase's unused reads stay inside) */
#define AR_TC1 2576
#define AR_DUMP 3056 /* 64 dwords: where lanes without a role read and write        */
#define AR_BYTES 3328
#define SH_TT 0      /* 160 dwords: B_PRED tap words by sub-block mode              */
#define SH_FT 640    /* 24 B: the filter parameters                                 */
#define SH_PROG 672  /* 16 dwords: per wave, macroblocks of its current row handed down */
#define SH_ABORT 736
#define SH_BYTES 768
#define FR_OUT ((int)0x80000000u) /* a buffer offset outside everything: loads return 0, stores are dropped */

#define FR_SPEC 0 /* the row text under the reference's rule; k_vp8_frames_items_libwebp includes it once more with 1 */
#define FR_AUX_SC0 1 /* workgroup-scope loads of the lines (they hit the CU's L1 like plain loads: the producer is on this CU) */
/* a B_PRED sub-block mode as the row reads it: k_vp8_frames takes it as it is (the host's check or k_vp8_check_modes refused the call
 * in front of it); k_vp8_frames_items clamps it (an item's host copy is checked, not its device copy: TT is never indexed beyond mode 9).
 * What a valid record is: vp8_mode_record_valid, ffhip_vp8_device.h */
#define FR_SUBMODE(m) m

template <int TYPE, bool PLANES, bool MAP> /* MAP: the call has a residual map (d_resmap): its scalar load per macroblock and four scalar registers only there; loop filter of the launch: 0 none, 1 simple, 2 normal; PLANES: the filtered planes are written as well (their three buffer
                                     resources, masks and stores cost every caller two dozen scalar registers in a kernel that spills a hundred: an instance of their own) */
__global__ __launch_bounds__(1024) void k_vp8_frames(Vp8FrameArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32 *const TT = (u32 *)(smem + SH_TT);
    uint8_t *const FT = smem + SH_FT;
    u32 *const PROG = (u32 *)(smem + SH_PROG);
    u32 *const ABORT = (u32 *)(smem + SH_ABORT);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), NW = (int)(blockDim.x >> 6);
    uint8_t *const AR = smem + SH_BYTES + w * AR_BYTES;
    uint8_t *const BT = AR + AR_BT, *const T = BT, *const C0 = BT + BT_C0, *const C1 = BT + BT_C1;
    short *const R = (short *)(AR + AR_R);
    uint8_t *const TL = AR + AR_TL;
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
#define FLDS32(addr) (*(__attribute__((address_space(3))) u32 *)(unsigned long long)(addr))
#define FLDS16(addr) (*(__attribute__((address_space(3))) unsigned short *)(unsigned long long)(addr))
    const unsigned bt = (unsigned)(unsigned long long)(lds_u8 *)BT, tl = (unsigned)(unsigned long long)(lds_u8 *)TL,
                   tc0 = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_TC0), tc1 = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_TC1),
                   dump = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_DUMP) + 4u * (unsigned)lane;
    const int ys = 16 * a.mbcols, us = 8 * a.mbcols, n_mb = a.mbcols * a.mbrows;
    /* the slot of one row's lines: six filtered luma rows (rows 10..15 of the macroblock row), four filtered rows of U and of
     * V (rows 4..7), then the unfiltered bottom row of Y, U, V */
    const int off_fu = 6 * ys, off_fv = 6 * ys + 4 * us, off_ul = 6 * ys + 8 * us, off_uu = off_ul + ys, off_uv = off_uu + us;

    /* ---- once per workgroup: the tap table, the filter parameters, the counters.  (This start of the workgroup is twice in this file, and the tap table's fill a third time in
     * k_vp8_predict_rows: as one included text or one inlined helper the same values came out of other instructions, and these kernels' code
     * is pinned.) ---- */
    if (w == 0) {
        if (lane < 16) {
            auto off = [](int k) { return k < 4 ? (3 - k) * PRS - 1 : (k == 4 ? -PRS - 1 : -PRS + (k - 5)); };
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const unsigned t = kVp8Taps[m][lane];
                TT[(m + 2) * 16 + lane] = (u32)(off((int)(t & 15)) + 64) | ((u32)(off((int)((t >> 4) & 15)) + 64) << 8) | ((u32)(off((int)(t >> 8)) + 64) << 16);
            }
            const int r = lane >> 2, c = lane & 3;
            TT[16 + lane] = (u32)(r * PRS - 1 + 64) | ((u32)(-PRS + c + 64) << 8) | ((u32)(-PRS - 1 + 64) << 16);
            TT[lane] = 64u | (64u << 8) | (64u << 16);
            PROG[lane] = 0u;
        }
        if (lane < 24) FT[lane] = (TYPE != 0 && a.filters) ? a.filters[lane] : (uint8_t)0;
        if (lane == 0) *ABORT = a.ctrl[1]; /* the mode check in front of this launch refused the call: nothing is written */
    }
    /* above-right of the sub-blocks in column 3 below the first row: always 127 (predict.c:509-517) */
    if (lane < 12) T[(4 + 4 * (lane >> 2)) * PRS + 20 + (lane & 3)] = 127;
    __syncthreads();
    if (__hip_atomic_load(ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;

#include "ffhip_vp8_frame_lanes.inc"

    const __amdgpu_buffer_rsrc_t rL = ffhip_rsrc(a.lines + (long long)blockIdx.x * (long long)a.nslot * (long long)a.slot_bytes, (unsigned)a.nslot * a.slot_bytes);
    /* ---- the rows of this workgroup's frames, round-robin over its waves: global row g = (frame of the share, row of the
     * frame); a frame has mbrows + 1 rows, the last one only applies nothing and emits the bottom six pixel rows ---- */
    const int RPF = a.mbrows + 1, PSTRIDE = a.mbcols + 2;
    for (int g = w;; g += NW) { /* (32-bit: a workgroup's share is a few frames of a few hundred rows) */
        const int k = g / RPF;
        const int y = g - k * RPF;
        const long long img = (long long)blockIdx.x + (long long)k * (long long)gridDim.x;
        if (img >= a.n_images) break;
        const bool real_row = y < a.mbrows; /* not the emission-only row below the picture */
        const int wp = (w + NW - 1) % NW;   /* the wave that has the row above */
        const u32 up_base = y > 0 ? (u32)((g - 1) / NW) * (u32)PSTRIDE : 0u, my_base = (u32)(g / NW) * (u32)PSTRIDE; /* (the first row of a frame waits for nobody) */
#include "ffhip_vp8_frame_row.inc"
    }
}

/* ---- mixed batches (ffhip_vp8_decode_items): frames of any size, filter parameters, output and pitch in one launch ----
 * The body is k_vp8_frames' (the two included texts) on a batch of one built per row from the frame's descriptor, read with scalar
 * loads (constant address space, wave-uniform index: the buffer resources stay in scalar registers).  What the uniform kernel takes
 * from one geometry per launch comes from the host's schedule here:
 *   - rows <-> waves: a workgroup's share is a list of frames; g counts the rows of the whole share (a frame has mbrows + 1 of them)
 *     and wave g % NW takes row g, as there.  slot.row0 is the share's row count in front of a frame.
 *   - progress: row g publishes base(g) + x, base(g) = slot.base0 + y * (mbcols + 2) with base0 the sum of (mbrows + 1) * (mbcols + 2)
 *     over the frames in front: bases grow along the share and a row's values stay below the next row's base, so a wave's counter only
 *     grows and a consumer of row g - 1 (same frame) is released exactly by that row.
 *   - filter parameters: 24 bytes per WAVE (waves of one workgroup can be on different frames), refilled at every row.
 *   - line slots: sized by the launch's widest frame, NW + 1 per workgroup as there, and one more behind them that nothing writes
 *     (zeroed per launch): the first row's read of "its" row above at soffset = num_records finds zeros whether or not the range
 *     check counts soffset in. */
struct Vp8FrameDesc {
    const uint8_t *modes;    /* [n_mb][20] */
    const int16_t *residual; /* [rows][384] */
    const int32_t *resmap;   /* [n_mb] or NULL */
    uint8_t *bgra;
    long long res_stride;    /* elements the residual's buffer resource spans: n_mb x 384 */
    int pitch, mbcols, mbrows, pad_;
    uint8_t filters[24];     /* [4][2][3] */
    uint8_t pad2_[8];
};
struct Vp8FrameSlot { int frame, row0; u32 base0, pad_; }; /* a workgroup's frames in order, then a sentinel: frame -1, row0 = the share's rows */
struct Vp8ItemsArgs {
    const Vp8FrameDesc *frames;
    const Vp8FrameSlot *sched;
    const u32 *wg_first; /* [gridDim.x]: the workgroup's first slot */
    uint8_t *lines;      /* [gridDim.x][nslot + 1][slot_bytes] */
    const uint32_t *ctrl;
    int *async_err;
    int nslot;
    unsigned slot_bytes;
};
typedef __attribute__((address_space(4))) const Vp8FrameDesc fr_cdesc;
typedef __attribute__((address_space(4))) const Vp8FrameSlot fr_cslot;
typedef __attribute__((address_space(4))) const u32 fr_cu32;

#undef FR_SUBMODE
#define FR_SUBMODE(m) std::min(m, 9)

template <int TYPE, bool MAP>
__global__ __launch_bounds__(1024) void k_vp8_frames_items(Vp8ItemsArgs ia)
{
    constexpr bool PLANES = false;
#include "ffhip_vp8_frame_items.inc"
}

/* ---- WEBP_RULE_LIBWEBP: k_vp8_frames_items' text (ffhip_vp8_frame_items.inc) once more with FR_SPEC set.  Prediction by RFC 6386 (the 127 / 129 borders for
 * 16x16 V_PRED and H_PRED too, so no row waits for the whole row above; the macroblock's above-right samples for sub-blocks 7, 11 and 15; the
 * last sample above, four times, right of the last macroblock), the loop filter's inner edges by B_PRED or the record's byte [19], and the
 * filtered PLANES as the only output: libwebp's upsampler reads the chroma row below a pixel row, which is final only after the next macroblock
 * row has been filtered, so the colour step is k_vp8_upsample_color behind this kernel.  The planes of a frame lie behind each other at the
 * descriptor's `bgra`: Y (256 B per macroblock), U, V (64 each).  Never a residual map.  The hand-counted wait in the row text counts, behind the
 * fetch and the lines, three stores (luma, U | V) where the BGRA instances count one and k_vp8_frames' PLANES instances four. */
template <int TYPE>
__global__ __launch_bounds__(1024) void k_vp8_frames_items_libwebp(Vp8ItemsArgs ia)
{
    constexpr bool PLANES = true, MAP = false;
#undef FR_SPEC
#define FR_SPEC 1
#include "ffhip_vp8_frame_items.inc"
#undef FR_SPEC
#define FR_SPEC 0
}
#undef FR_SUBMODE

/* ------------------------------------------------------------------------ host */

extern "C" int ffhip_vp8_check_modes_enqueue(const uint8_t *d_modes, long long n_records, uint32_t *ctrl, int *async_err, void *stream); /* ffhip_vp8_pred.hip */
extern "C" int ffhip_vp8_modes_ok_host(const uint8_t *h_modes, long long n_records);                                                   /* ffhip_vp8_pred.hip */

/* The three-stage form of the same call (the latency form for small batches): prediction || loop filter as the row kernels,
 * then the planar colour conversion; needs the planes, which a caller that did not pass any gets from library scratch. */
static int decode_frames_rows(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                              int64_t residual_stride, const int32_t *d_resmap, int filter_type, const uint8_t *d_filters, uint8_t *d_bgra,
                              int pitch, int64_t image_stride, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y,
                              int64_t plane_stride_uv, void *stream)
{
    const long long n_mb = (long long)mbcols * mbrows;
    if (!d_y) {
        const size_t per = (size_t)n_mb * 384; /* 256 + 64 + 64 bytes per macroblock */
        uint8_t *p = (uint8_t *)ffhip_scratch(SCRATCH_VP8_FRAMES + 1, stream, ((size_t)n_images * per + 3) / 4);
        if (!p) return FFHIP_ENOMEM;
        d_y = p; d_u = p + (size_t)n_images * n_mb * 256; d_v = d_u + (size_t)n_images * n_mb * 64;
        plane_stride_y = n_mb * 256; plane_stride_uv = n_mb * 64;
        /* the planes' initial contents are what the reference's raw H_PRED reads at x = 0 find below a row's first pixel: fresh planes are zero */
        FFHIP_CHECK(hipMemsetAsync(p, 0, (size_t)n_images * per, (hipStream_t)stream), FFHIP_EIO);
    } else { /* the caller's planes are outputs of this call in either form: what they held must not show through those reads */
        /* one memset per plane set (packed frames), or one 2-D memset (a "row" = a frame's plane, the pitch = the frame stride): three per
         * frame were up to ~380 enqueues in front of a form chosen for its latency */
        struct { uint8_t *p; int64_t stride; size_t bytes; } pl[3] = {{d_y, plane_stride_y, (size_t)n_mb * 256}, {d_u, plane_stride_uv, (size_t)n_mb * 64}, {d_v, plane_stride_uv, (size_t)n_mb * 64}};
        for (auto &q : pl) {
            if (n_images == 1 || q.stride == (int64_t)q.bytes) FFHIP_CHECK(hipMemsetAsync(q.p, 0, q.bytes * (size_t)n_images, (hipStream_t)stream), FFHIP_EIO);
            else if (q.stride > (int64_t)q.bytes) FFHIP_CHECK(hipMemset2DAsync(q.p, (size_t)q.stride, 0, q.bytes, (size_t)n_images, (hipStream_t)stream), FFHIP_EIO);
            else
                for (int i = 0; i < n_images; i++) FFHIP_CHECK(hipMemsetAsync(q.p + (int64_t)i * q.stride, 0, q.bytes, (hipStream_t)stream), FFHIP_EIO);
        }
    }
    /* the colour conversion below belongs to the call: should ffhip_stream_sync have to repeat prediction and filter, it repeats it behind them */
    const FfhipVp8Then then = {d_bgra, pitch, image_stride};
    int rc = vp8_predict_loopfilter_impl(mbcols, mbrows, n_images, h_modes, d_modes, d_residual, residual_stride, d_resmap, filter_type, d_filters,
                                         d_y, d_u, d_v, plane_stride_y, plane_stride_uv, stream, &then);
    if (rc) return rc;
    return ffhip_yuv420_to_bgra(d_bgra, pitch, d_y, d_u, d_v, 16 * mbcols, 8 * mbcols, mbrows, mbcols, n_images, plane_stride_y, plane_stride_uv,
                                image_stride, stream);
}

static int device_cus() /* of the current device, asked every time */
{
    int cus = 256, dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}

/* Waves per workgroup, i.e. per frame at work: 16 while there is at most one frame per CU (four waves per SIMD either way), else 8 and two
 * frames per CU -- or 4 and four frames:
 * rows that start with the reference's wrapped 16x16 H_PRED (predict.c:346-353: the sample left of a row's first pixel is the LAST pixel of
 * the row above) wait for the whole row above: while such a row waits, its frame keeps ONE wave busy.  A stream with many of them -- one
 * row in seven with uniformly random modes -- is faster with four frames of four waves on a CU than with two of eight: 1 024 random-mode
 * 1080p frames 12.5 ms against 14.4 (an encoder's stream, which has next to none: 8.85 against 8.41).  Told from a sample of the host's
 * copies of the modes: the first column of up to 32 frames, `sampler(f)` yielding frame f's (modes NULL: it has no host copy). */
struct Vp8FirstColumn { const uint8_t *modes; int mbcols, mbrows; };
template <class Sampler>
static int frame_waves(int n_frames, int cus, Sampler sampler)
{
    if (n_frames < 4LL * cus) return n_frames <= cus ? 16 : 8;
    long long rows = 0, serial = 0;
    for (int f = 0, step = n_frames > 32 ? n_frames / 32 : 1; f < n_frames; f += step) {
        const Vp8FirstColumn c = sampler(f);
        if (!c.modes) continue;
        for (int y = 1; y < c.mbrows; y++, rows++) serial += c.modes[(long long)y * c.mbcols * 20] == 3;
    }
    return rows > 0 && serial * 16 >= rows ? 4 : 8;
}

static bool frames_take_fused_form(int n_images)
{
    /* the frame kernel wants a frame per workgroup and enough workgroups to fill the chip; a handful of frames is
     * faster as rows of any frame on any wave (ffhip_vp8_pred.hip).  FFHIP_VP8_FRAMES=rows|fused forces either. */
    const int cus = device_cus();
    const char *form = FFHIP_ENV("FFHIP_VP8_FRAMES");
    const char *thr = FFHIP_ENV("FFHIP_VP8_FRAMES_MIN");
    const int min_fused = thr ? atoi(thr) : cus / 2;
    return form ? !strcmp(form, "fused") : n_images >= min_fused;
}
extern "C" int ffhip_vp8_decode_frames_form(int n_images)
{
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    return frames_take_fused_form(n_images) ? 1 : 0;
}

extern "C" int ffhip_vp8_decode_frames(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes,
                                       const int16_t *d_residual, int64_t residual_stride, const int32_t *d_resmap, int filter_type,
                                       const uint8_t *d_filters, uint8_t *d_bgra, int pitch, int64_t image_stride, uint8_t *d_y, uint8_t *d_u,
                                       uint8_t *d_v, int64_t plane_stride_y, int64_t plane_stride_uv, void *stream)
{
    if (mbcols <= 0 || mbrows <= 0 || n_images < 0 || filter_type < 0 || filter_type > 2) return FFHIP_EINVAL;
    if (n_images == 0) return FFHIP_OK;
    if (!d_modes || !d_residual || !d_bgra || (filter_type != 0 && !d_filters)) return FFHIP_EINVAL;
    if ((d_y != nullptr) != (d_u != nullptr) || (d_y != nullptr) != (d_v != nullptr)) return FFHIP_EINVAL;
    if (((uintptr_t)d_residual & 3) || (residual_stride & 1) || ((uintptr_t)d_modes & 3)) return FFHIP_EINVAL;
    if (pitch < 64 * mbcols || (pitch & 15) || ((uintptr_t)d_bgra & 15) || (image_stride & 15)) return FFHIP_EINVAL;
    if (d_y && ((((uintptr_t)d_y | (uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)plane_stride_y | (uintptr_t)plane_stride_uv) & 3))) return FFHIP_EINVAL;
    const long long n_mb = (long long)mbcols * mbrows;
    if (n_mb * n_images > 0x3fffffffLL || n_mb >= (1LL << 23) || (long long)pitch * 16 * mbrows > 0x7fffffffLL) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;

    const int cus = device_cus();
    const bool fused = frames_take_fused_form(n_images);
    if (!fused) {
        if (!h_modes) return FFHIP_EINVAL; /* the row form checks small batches on the host copy */
        return decode_frames_rows(mbcols, mbrows, n_images, h_modes, d_modes, d_residual, residual_stride, d_resmap, filter_type, d_filters, d_bgra,
                                  pitch, image_stride, d_y, d_u, d_v, plane_stride_y, plane_stride_uv, stream);
    }

    int *async_err = ffhip_async_err_word();
    if (!async_err) return FFHIP_ENOMEM;
    /* mode bytes: as ffhip_vp8_predict_recon -- small batches on the host copy (when there is one), large ones by a kernel in front */
    const long long recs = n_mb * n_images;
    const bool host_checked = h_modes && recs <= (1LL << 17);
    if (host_checked && !ffhip_vp8_modes_ok_host(h_modes, recs)) return FFHIP_EINVAL;

    const char *nwv = FFHIP_ENV("FFHIP_VP8_FRAME_WAVES");
    int nw = nwv ? atoi(nwv) : frame_waves(n_images, cus, [&](int f) { return Vp8FirstColumn{h_modes ? h_modes + (long long)f * n_mb * 20 : nullptr, mbcols, mbrows}; });
    nw = std::max(1, std::min(16, nw));
    const size_t lds = SH_BYTES + (size_t)nw * AR_BYTES;
    const bool planes = d_y != nullptr;
    const bool map = d_resmap != nullptr;
    const void *kern = nullptr;
#define FR_PICK(T, P, M) if (filter_type == T && planes == P && map == M) kern = (const void *)k_vp8_frames<T, P, M>
    FR_PICK(0, false, false); FR_PICK(1, false, false); FR_PICK(2, false, false); FR_PICK(0, true, false); FR_PICK(1, true, false); FR_PICK(2, true, false);
    FR_PICK(0, false, true); FR_PICK(1, false, true); FR_PICK(2, false, true); FR_PICK(0, true, true); FR_PICK(1, true, true); FR_PICK(2, true, true);
#undef FR_PICK
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, nw * 64, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    const char *gv = FFHIP_ENV("FFHIP_VP8_FRAME_GRID");
    const long long grid = std::max<long long>(1, std::min<long long>(n_images, gv ? atoi(gv) : (long long)per_cu * cus));
    const int nslot = nw + 1;
    const unsigned slot_bytes = (unsigned)(192 * mbcols + 64);
    const size_t line_words = ((size_t)grid * nslot * slot_bytes + 3) / 4;
    uint32_t *scratch = ffhip_scratch(SCRATCH_VP8_FRAMES, stream, 4 + line_words);
    if (!scratch) return FFHIP_ENOMEM;
    FFHIP_CHECK(hipMemsetAsync(scratch, 0, 16, st), FFHIP_EIO);
    if (!host_checked) {
        const int rc = ffhip_vp8_check_modes_enqueue(d_modes, recs, scratch, async_err, stream);
        if (rc) return rc;
    }
    Vp8FrameArgs a = {};
    a.modes = d_modes; a.residual = d_residual; a.resmap = d_resmap; a.filters = d_filters;
    a.bgra = d_bgra; a.y = d_y; a.u = d_u; a.v = d_v;
    a.lines = (uint8_t *)(scratch + 4); a.ctrl = scratch; a.async_err = async_err;
    a.res_stride = residual_stride; a.image_stride = image_stride; a.plane_y = plane_stride_y; a.plane_uv = plane_stride_uv;
    a.pitch = pitch; a.mbcols = mbcols; a.mbrows = mbrows; a.n_images = n_images; a.nslot = nslot; a.slot_bytes = slot_bytes;
    {
        void *kargs[] = {(void *)&a};
        FFHIP_CHECK(hipLaunchKernel(kern, dim3((unsigned)grid), dim3((unsigned)nw * 64), kargs, lds, st), FFHIP_EIO);
    }
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

/* ---- ffhip_vp8_decode_items ---- */

static const void *items_kernel(int ft, bool map, int rule)
{
    if (rule == WEBP_RULE_LIBWEBP)
        return ft == 0 ? (const void *)k_vp8_frames_items_libwebp<0> : ft == 1 ? (const void *)k_vp8_frames_items_libwebp<1> : (const void *)k_vp8_frames_items_libwebp<2>;
#define FRI_PICK(T, M) if (ft == T && map == M) return (const void *)k_vp8_frames_items<T, M>
    FRI_PICK(0, false); FRI_PICK(1, false); FRI_PICK(2, false); FRI_PICK(0, true); FRI_PICK(1, true); FRI_PICK(2, true);
#undef FRI_PICK
    return nullptr;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" int ffhip_vp8_decode_items(const ffhip_vp8_item *items, int n, void *stream)
{
    return vp8_decode_items_rule(items, n, WEBP_RULE_REFERENCE, nullptr, nullptr, stream);
}

extern "C" int ffhip_debug_vp8_decode_items_libwebp(const ffhip_vp8_item *items, int n, const ffhip_size *display, void *stream)
{
    return vp8_decode_items_rule(items, n, WEBP_RULE_LIBWEBP, display, nullptr, stream);
}

int vp8_decode_items_rule(const ffhip_vp8_item *items, int n, int rule, const ffhip_size *display, uint8_t *const *planes, void *stream)
{
    const bool lw = rule == WEBP_RULE_LIBWEBP;
    if (n < 0 || (n > 0 && !items) || (lw && n > 0 && !display)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* every item checked as ffhip_vp8_residual_batch + ffhip_vp8_decode_frames check a batch of one */
    long long total_mb = 0, lv_mb = 0, chk_recs = 0, bases = 0;
    int n_lv = 0, n_chk = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_vp8_item &it = items[i];
        if (it.mbcols <= 0 || it.mbrows <= 0 || it.filter_type < 0 || it.filter_type > 2) return FFHIP_EINVAL;
        const long long n_mb = (long long)it.mbcols * it.mbrows;
        if (n_mb >= (1LL << 23)) return FFHIP_EINVAL;
        if (!it.d_modes || ((uintptr_t)it.d_modes & 3) || !it.d_bgra || ((uintptr_t)it.d_bgra & 15)) return FFHIP_EINVAL;
        if (it.pitch < 64LL * it.mbcols || it.pitch > 0x7fffffffLL || (it.pitch & 15) || it.pitch * 16 * it.mbrows > 0x7fffffffLL) return FFHIP_EINVAL;
        const bool lv = it.d_levels != nullptr;
        if (lv == (it.d_residual != nullptr)) return FFHIP_EINVAL; /* exactly one form of the residual */
        if (lv ? (!it.d_mbinfo || ((uintptr_t)it.d_levels & 15) || ((uintptr_t)it.d_mbinfo & 3)) : ((uintptr_t)it.d_residual & 3) != 0) return FFHIP_EINVAL;
        if ((uintptr_t)it.d_resmap & 3) return FFHIP_EINVAL;
        if (lw) { /* levels only, no residual map, the picture inside its macroblock grid; delivered planes 4-byte aligned */
            if (!lv || it.d_resmap || display[i].width < 1 || display[i].height < 1 || display[i].width > 16 * it.mbcols || display[i].height > 16 * it.mbrows)
                return FFHIP_EINVAL;
            if (planes && (!planes[3 * i] || !planes[3 * i + 1] || !planes[3 * i + 2] ||
                           (((uintptr_t)planes[3 * i] | (uintptr_t)planes[3 * i + 1] | (uintptr_t)planes[3 * i + 2]) & 3)))
                return FFHIP_EINVAL;
        }
        total_mb += n_mb;
        bases += (long long)(it.mbrows + 1) * (it.mbcols + 2); /* the progress bases of a workgroup's share stay below this */
        if (total_mb > 0x3fffffffLL || bases > 0x7fff0000LL) return FFHIP_EINVAL;
        if (lv) { n_lv++; lv_mb += n_mb; }
        if (!it.h_modes) { n_chk++; chk_recs += n_mb; }
    }
    for (int i = 0; i < n; i++) /* (the records last: a call the cheap checks refuse is refused without a pass over them) */
        if (items[i].h_modes && !ffhip_vp8_modes_ok_host(items[i].h_modes, (long long)items[i].mbcols * items[i].mbrows)) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    int *async_err = ffhip_async_err_word();
    if (!async_err) return FFHIP_ENOMEM;
    const int cus = device_cus();

    /* one launch per (filter type, residual-map form) present; in each, the frames dealt largest first to the least-loaded workgroup */
    struct Launch {
        int ft = 0, nw = 0, grid = 0, nslot = 0;
        bool map = false;
        unsigned slot_bytes = 0;
        size_t lds = 0, wg_first_off = 0, sched_off = 0;
        std::vector<int> frames;
        std::vector<Vp8FrameSlot> sched;
        std::vector<u32> wg_first;
    };
    std::vector<Launch> launches;
    size_t lines_bytes = 0;
    for (int m = 0; m < 2; m++)
        for (int ft = 0; ft < 3; ft++) {
            Launch L;
            L.ft = ft; L.map = m != 0;
            for (int i = 0; i < n; i++)
                if (items[i].filter_type == ft && (items[i].d_resmap != nullptr) == L.map) L.frames.push_back(i);
            if (L.frames.empty()) continue;
            const int nf = (int)L.frames.size();
            const int nw = frame_waves(nf, cus, [&](int f) { /* ffhip_vp8_decode_frames' choice for a batch of this many frames */
                const ffhip_vp8_item &it = items[L.frames[(size_t)f]];
                return Vp8FirstColumn{it.h_modes, it.mbcols, it.mbrows};
            });
            L.nw = nw;
            L.lds = SH_BYTES + (size_t)nw * (AR_BYTES + 32);
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, items_kernel(ft, L.map, rule), nw * 64, L.lds) != hipSuccess || per_cu < 1) {
                (void)hipGetLastError();
                per_cu = 1;
            }
            L.grid = (int)std::min<long long>(nf, (long long)per_cu * cus);
            L.nslot = nw + 1;
            int maxc = 0;
            for (int i : L.frames) maxc = std::max(maxc, items[i].mbcols);
            L.slot_bytes = (unsigned)(192 * maxc + 64);
            lines_bytes = std::max(lines_bytes, (size_t)L.grid * (size_t)(L.nslot + 1) * L.slot_bytes);
            std::vector<int> order = L.frames;
            auto mbs = [&](int i) { return (long long)items[i].mbcols * items[i].mbrows; };
            std::stable_sort(order.begin(), order.end(), [&](int x, int z) { return mbs(x) > mbs(z); });
            std::vector<std::vector<int>> share((size_t)L.grid);
            std::priority_queue<std::pair<long long, int>, std::vector<std::pair<long long, int>>, std::greater<std::pair<long long, int>>> load;
            for (int b = 0; b < L.grid; b++) load.push({0, b});
            for (int i : order) {
                const auto top = load.top();
                load.pop();
                share[(size_t)top.second].push_back(i);
                load.push({top.first + mbs(i), top.second});
            }
            for (int b = 0; b < L.grid; b++) {
                L.wg_first.push_back((u32)L.sched.size());
                int row = 0;
                u32 base = 0;
                for (int i : share[(size_t)b]) {
                    L.sched.push_back({i, row, base, 0u});
                    row += items[i].mbrows + 1;
                    base += (u32)(items[i].mbrows + 1) * (u32)(items[i].mbcols + 2);
                }
                L.sched.push_back({-1, row, base, 0u});
            }
            launches.push_back(std::move(L));
        }

    /* the tables, one upload: control words, frame descriptors, residual items, check items, per launch its workgroups' first slots and
     * slots; the residual stage's per-workgroup table (written on the device) behind them */
    size_t at = 64;
    const size_t off_frames = at;
    at = align16(at + (size_t)n * sizeof(Vp8FrameDesc));
    const size_t off_res = at;
    at = align16(at + (size_t)(n_lv + 1) * (lw ? sizeof(Vp8LwResItem) : sizeof(Vp8ResItem)));
    const size_t off_chk = at;
    at = align16(at + (size_t)(n_chk + 1) * sizeof(Vp8CheckItem));
    for (Launch &L : launches) {
        L.wg_first_off = at;
        at = align16(at + L.wg_first.size() * sizeof(u32));
        L.sched_off = at;
        at = align16(at + L.sched.size() * sizeof(Vp8FrameSlot));
    }
    const size_t blob = at, res_wg = (size_t)((lv_mb + 7) / 8);
    uint8_t *dev_tab = (uint8_t *)ffhip_scratch(SCRATCH_VP8_ITEMS, stream, blob / 4 + res_wg + 4);
    if (!dev_tab) return FFHIP_ENOMEM;
    int16_t *dev_res = nullptr;
    if (lv_mb) {
        dev_res = (int16_t *)ffhip_scratch(SCRATCH_VP8_ITEMS + 1, stream, (size_t)lv_mb * 192);
        if (!dev_res) return FFHIP_ENOMEM;
    }
    uint8_t *dev_lines = (uint8_t *)ffhip_scratch(SCRATCH_VP8_ITEMS + 2, stream, lines_bytes / 4 + 4);
    if (!dev_lines) return FFHIP_ENOMEM;
    uint8_t *dev_planes = nullptr; /* the libwebp rule: every frame's filtered planes, 384 B per macroblock, in stream scratch */
    if (lw) {
        dev_planes = (uint8_t *)ffhip_scratch(SCRATCH_VP8_LIBWEBP + 1, stream, (size_t)total_mb * 96 + 4);
        if (!dev_planes) return FFHIP_ENOMEM;
    }
    std::vector<Vp8LwColorItem> colour;
    uint8_t *pin = ffhip_pinned_staging(SCRATCH_VP8_ITEMS, stream, blob);
    if (!pin) return FFHIP_ENOMEM;
    memset(pin, 0, blob);
    {
        Vp8FrameDesc *fd = (Vp8FrameDesc *)(pin + off_frames);
        Vp8ResItem *ri = (Vp8ResItem *)(pin + off_res);
        Vp8LwResItem *rl = (Vp8LwResItem *)(pin + off_res);
        Vp8CheckItem *ci = (Vp8CheckItem *)(pin + off_chk);
        long long lv_at = 0, chk_at = 0;
        int k_lv = 0, k_chk = 0;
        for (int i = 0; i < n; i++) {
            const ffhip_vp8_item &it = items[i];
            const long long n_mb = (long long)it.mbcols * it.mbrows;
            Vp8FrameDesc &d = fd[i];
            d.modes = it.d_modes; d.resmap = it.d_resmap; d.bgra = it.d_bgra;
            d.res_stride = n_mb * 384; d.pitch = (int)it.pitch; d.mbcols = it.mbcols; d.mbrows = it.mbrows;
            memcpy(d.filters, it.filters, 24);
            if (lw) {
                Vp8LwResItem &r = rl[k_lv++];
                r.levels = it.d_levels; r.info = it.d_mbinfo; r.out = dev_res + lv_at * 384; r.first = lv_at;
                r.modes = const_cast<uint8_t *>(it.d_modes); /* byte [19] of every record is this call's to write */
                memcpy(r.quant, it.quant, sizeof(r.quant));
                d.residual = r.out;
                uint8_t *pl = dev_planes + lv_at * 384;
                d.bgra = pl; d.pitch = 0; /* the libwebp instances' planes stand where the BGRA instances have their picture */
                colour.push_back({pl, pl + 256 * n_mb, pl + 320 * n_mb, 16 * it.mbcols, 8 * it.mbcols, display[i].width, display[i].height, it.d_bgra, (long long)it.pitch});
                lv_at += n_mb;
            } else if (it.d_levels) {
                Vp8ResItem &r = ri[k_lv++];
                r.levels = it.d_levels; r.info = it.d_mbinfo; r.out = dev_res + lv_at * 384; r.first = lv_at;
                memcpy(r.quant, it.quant, sizeof(r.quant));
                d.residual = r.out;
                lv_at += n_mb;
            } else {
                d.residual = it.d_residual;
            }
            if (!it.h_modes) {
                ci[k_chk].modes = it.d_modes; ci[k_chk].first = chk_at;
                k_chk++;
                chk_at += n_mb;
            }
        }
        if (lw) rl[n_lv].first = lv_mb;
        else ri[n_lv].first = lv_mb;
        ci[n_chk].first = chk_recs;
        for (const Launch &L : launches) {
            memcpy(pin + L.wg_first_off, L.wg_first.data(), L.wg_first.size() * sizeof(u32));
            memcpy(pin + L.sched_off, L.sched.data(), L.sched.size() * sizeof(Vp8FrameSlot));
        }
    }
    FFHIP_CHECK(hipMemcpyAsync(dev_tab, pin, blob, hipMemcpyHostToDevice, st), FFHIP_EIO);
    if (ffhip_pinned_staged(SCRATCH_VP8_ITEMS, stream) != FFHIP_OK) return FFHIP_EIO;
    uint32_t *ctrl = (uint32_t *)dev_tab;
    if (n_chk) {
        const int rc = vp8_check_modes_items_enqueue((const Vp8CheckItem *)(dev_tab + off_chk), n_chk, chk_recs, ctrl, async_err, stream);
        if (rc) return rc;
    }
    if (lw) {
        const int rc = vp8_libwebp_residual_items_enqueue((const Vp8LwResItem *)(dev_tab + off_res), n_lv, lv_mb, stream);
        if (rc) return rc;
    } else if (n_lv) {
        const int rc = vp8_residual_items_enqueue((const Vp8ResItem *)(dev_tab + off_res), n_lv, lv_mb, (uint32_t *)(dev_tab + blob), stream);
        if (rc) return rc;
    }
    for (const Launch &L : launches) {
        /* the slot behind each workgroup's slots: zeros (another launch's layout may have put lines there) */
        FFHIP_CHECK(hipMemset2DAsync(dev_lines + (size_t)L.nslot * L.slot_bytes, (size_t)(L.nslot + 1) * L.slot_bytes, 0, L.slot_bytes, (size_t)L.grid, st),
                    FFHIP_EIO);
        Vp8ItemsArgs a = {};
        a.frames = (const Vp8FrameDesc *)(dev_tab + off_frames);
        a.sched = (const Vp8FrameSlot *)(dev_tab + L.sched_off);
        a.wg_first = (const u32 *)(dev_tab + L.wg_first_off);
        a.lines = dev_lines; a.ctrl = ctrl; a.async_err = async_err; a.nslot = L.nslot; a.slot_bytes = L.slot_bytes;
        void *kargs[] = {(void *)&a};
        FFHIP_CHECK(hipLaunchKernel(items_kernel(L.ft, L.map, rule), dim3((unsigned)L.grid), dim3((unsigned)L.nw * 64), kargs, L.lds, st), FFHIP_EIO);
        FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    }
    if (lw) {
        const int rc = vp8_libwebp_color_items(colour.data(), (int)colour.size(), stream);
        if (rc) return rc;
        if (planes)
            for (int i = 0; i < n; i++) {
                const size_t n_mb = (size_t)items[i].mbcols * items[i].mbrows;
                const uint8_t *pl = colour[(size_t)i].y;
                FFHIP_CHECK(hipMemcpyAsync(planes[3 * i], pl, 256 * n_mb, hipMemcpyDeviceToDevice, st), FFHIP_EIO);
                FFHIP_CHECK(hipMemcpyAsync(planes[3 * i + 1], pl + 256 * n_mb, 64 * n_mb, hipMemcpyDeviceToDevice, st), FFHIP_EIO);
                FFHIP_CHECK(hipMemcpyAsync(planes[3 * i + 2], pl + 320 * n_mb, 64 * n_mb, hipMemcpyDeviceToDevice, st), FFHIP_EIO);
            }
    }
    return FFHIP_OK;
}
