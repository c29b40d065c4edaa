/* ffhip_tensor_body.h -- the record and the per-lane body of the tensor sink (ffhip_tensor.hip).  Plain C++ without builtins, __host__ too:
 * a CPU program can run the body lane by lane over host buffers and hold its addressing against exact-size allocations.
 *
 * A picture's output is a set of RUNS of contiguous elements: the rows of an HWC tensor (3 x width elements, R,G,B,R,G,B,...), the plane rows
 * of a CHW tensor (width elements of one channel; run = 3 * row + channel, so the three runs that read a source row lie side by side).  A run
 * starts at ANY element of the destination, so it is cut along the destination's 16-byte blocks: block u of a run is
 * (run start & ~15) + 16 u.  A block that lies inside its run is the body: one aligned 16-byte store of 16 / 8 / 4 elements packed in
 * registers.  The first and the last block of a run may reach outside it: the head and the tail, stored element by element, nothing outside
 * the run touched.  One UNIT = one block of one run; unit t of an item is block t % units of run t / units (`units` = the most blocks a run
 * of the item can touch), so consecutive lanes walk along a run and on into the next: narrow pictures' rows share a wave, a wide row is
 * spread over as many waves as it has blocks.  Source pixels are dwords at 4 (x0 + pixel): loads stay dword-aligned wherever a block begins.
 *
 * The forms with alpha are further instances of the same unit: NC = 4 channels (rows of 4 x width elements, four plane
 * rows per source row, a block beginning 0..3 elements into a pixel) or 3 composited over a background, and an alpha policy AP that says
 * what becomes of a colour byte on its way -- the per-pixel step tensor_alpha_step, in front of the element's conversion. */
#ifndef FFHIP_TENSOR_BODY_H
#define FFHIP_TENSOR_BODY_H

#include <stdint.h>

#include "ffpic_hip.h"
#include "ffhip_alpha_body.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

/* the kernel's pointers come out of a record: said to be global here, they get global loads and stores instead of flat ones */
#ifdef __HIP_DEVICE_COMPILE__
#define TENSOR_GLOBAL __attribute__((address_space(1)))
#else
#define TENSOR_GLOBAL
#endif

#define FFHIP_TENSOR_WG_THREADS 256
#define FFHIP_TENSOR_UNITS_PER_LANE 8
#define FFHIP_TENSOR_WG_UNITS (FFHIP_TENSOR_WG_THREADS * FFHIP_TENSOR_UNITS_PER_LANE)

struct TensorItemDesc { /* 64 bytes, 16-byte aligned: scalar loads */
    const uint8_t *src;                 /* pixel (x0, y0) of the picture */
    uint8_t *dst;                       /* element 0 of the output */
    long long pitch;                    /* source row pitch, bytes */
    long long row_stride, plane_stride; /* elements */
    int width, height;
    uint32_t units;                     /* blocks a run can touch at most: (run bytes + 15) / 16 + 1 */
    uint32_t total;                     /* runs * units */
    uint32_t first_wg, n_wgs;           /* its workgroups: FFHIP_TENSOR_WG_UNITS units each */
    uint32_t pad_[2];
};
struct TensorScale { float scale[3], bias[3]; }; /* per OUTPUT channel */

/* What the sink makes of the alpha byte.  NONE: ignored, three channels -- the twelve instances of 4.10.  The others are
 * a mode of ffhip_tensor_alpha met with a straight or a premultiplied source: KEEP (four channels, the colour as stored: STRAIGHT from a
 * straight source, PREMULTIPLIED from a premultiplied one), PREMUL and UNPREMUL (four channels, the colour through the rule), OVER_S and
 * OVER_P (three channels, the colour composited over the background) */
enum { TENSOR_ALPHA_NONE = 0, TENSOR_ALPHA_KEEP, TENSOR_ALPHA_PREMUL, TENSOR_ALPHA_UNPREMUL, TENSOR_ALPHA_OVER_S, TENSOR_ALPHA_OVER_P };
struct TensorAlpha { uint32_t background; float alpha_scale, alpha_bias; }; /* background: B,G,R from the low byte, as a pixel */

typedef uint32_t tensor_u32x4 __attribute__((ext_vector_type(4)));

/* the per-pixel step: colour byte c of a pixel with alpha a under policy AP, g the background's byte of the same colour */
template <int AP> __host__ __device__ inline uint32_t tensor_alpha_step(uint32_t c, uint32_t a, uint32_t g)
{
    if (AP == TENSOR_ALPHA_PREMUL) return alpha_premultiply(c, a);
    if (AP == TENSOR_ALPHA_UNPREMUL) return alpha_unpremultiply(c, a);
    if (AP == TENSOR_ALPHA_OVER_S) return alpha_over_straight(c, a, g);
    if (AP == TENSOR_ALPHA_OVER_P) return alpha_over_premultiplied(c, a, g);
    return c;
}

/* the bits of one output element: channel `ch` (0..2, output order) of pixel `px` (B,G,R,A from the low byte) */
template <int DT, bool BGR> __host__ __device__ inline uint32_t tensor_elem(uint32_t px, int ch, const TensorScale &s)
{
    const uint32_t byte = (px >> (8 * (BGR ? ch : 2 - ch))) & 0xffu;
    if (DT == FFHIP_TENSOR_U8) return byte;
    const float sc = ch == 0 ? s.scale[0] : (ch == 1 ? s.scale[1] : s.scale[2]);
    const float bi = ch == 0 ? s.bias[0] : (ch == 1 ? s.bias[1] : s.bias[2]);
    const float prod = (float)byte * sc; /* built with -ffp-contract=off: product and sum round separately */
    const float f = prod + bi;
    if (DT == FFHIP_TENSOR_F16) return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f); /* round to nearest even */
    return __builtin_bit_cast(uint32_t, f);
}
/* the same under an alpha policy: channel 3 is the alpha byte, with a scale and a bias of its own */
template <int DT, bool BGR, int AP> __host__ __device__ inline uint32_t tensor_elem_alpha(uint32_t px, int ch, const TensorScale &s, const TensorAlpha &al)
{
    const int pos = BGR ? ch : 2 - ch;
    const uint32_t a = px >> 24;
    const uint32_t byte = ch == 3 ? a : tensor_alpha_step<AP>((px >> (8 * pos)) & 0xffu, a, (al.background >> (8 * pos)) & 0xffu);
    if (DT == FFHIP_TENSOR_U8) return byte;
    const float sc = ch == 0 ? s.scale[0] : (ch == 1 ? s.scale[1] : (ch == 2 ? s.scale[2] : al.alpha_scale));
    const float bi = ch == 0 ? s.bias[0] : (ch == 1 ? s.bias[1] : (ch == 2 ? s.bias[2] : al.alpha_bias));
    const float prod = (float)byte * sc;
    const float f = prod + bi;
    if (DT == FFHIP_TENSOR_F16) return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f);
    return __builtin_bit_cast(uint32_t, f);
}
template <int DT> __host__ __device__ inline void tensor_store_elem(TENSOR_GLOBAL uint8_t *p, uint32_t bits)
{
    if (DT == FFHIP_TENSOR_U8) *p = (uint8_t)bits;
    else if (DT == FFHIP_TENSOR_F16) *(TENSOR_GLOBAL uint16_t *)p = (uint16_t)bits;
    else *(TENSOR_GLOBAL uint32_t *)p = bits;
}

/* unit t (< d.total) of item d: NC output channels (3, or 4 with the alpha channel last) under alpha policy AP */
template <int DT, bool PLANAR, bool BGR, int NC = 3, int AP = TENSOR_ALPHA_NONE>
__host__ __device__ inline void tensor_unit(const TensorItemDesc &d, const TensorScale &s, uint32_t t, const TensorAlpha &al = TensorAlpha{0u, 1.0f, 0.0f})
{
    const auto elem = [&](uint32_t px, int ch) { return AP == TENSOR_ALPHA_NONE ? tensor_elem<DT, BGR>(px, ch, s) : tensor_elem_alpha<DT, BGR, AP>(px, ch, s, al); };
    constexpr int ES = DT == FFHIP_TENSOR_U8 ? 1 : (DT == FFHIP_TENSOR_F16 ? 2 : 4); /* element size */
    constexpr int EPB = 16 / ES;                                                     /* elements per block */
    constexpr int NP = PLANAR ? EPB : (EPB + 2 * (NC - 1)) / NC;                     /* source pixels a body block needs at most: 6 / 4 / 2, or 5 / 3 / 2 */
    constexpr int ND = PLANAR ? 4 : (NC * NP * ES + 3) / 4;                          /* dwords of converted elements */
    const uint32_t run = t / d.units, u = t - run * d.units;
    const uint32_t row = PLANAR ? run / (uint32_t)NC : run;
    const int c = PLANAR ? (int)(run - row * (uint32_t)NC) : 0;
    const long long run_len = PLANAR ? d.width : (long long)NC * d.width;
    const TENSOR_GLOBAL uint32_t *src = (const TENSOR_GLOBAL uint32_t *)(d.src + (long long)row * d.pitch);
    const uintptr_t start = (uintptr_t)d.dst + (uintptr_t)(((long long)row * d.row_stride + (long long)c * d.plane_stride) * ES);
    TENSOR_GLOBAL uint8_t *blk = (TENSOR_GLOBAL uint8_t *)((start & ~(uintptr_t)15) + 16u * (uintptr_t)u);
    const long long j0 = ((long long)(uintptr_t)blk - (long long)start) / ES; /* the run's element at the block's first byte; < 0 in the head */
    if (j0 >= run_len) return;                                               /* the run ended before this block */
    if (j0 < 0 || j0 + EPB > run_len) {
        /* head or tail: the elements of the block that belong to the run, one store each */
        for (int e = 0; e < EPB; e++) {
            const long long j = j0 + e;
            if (j < 0 || j >= run_len) continue;
            const uint32_t p = PLANAR ? (uint32_t)j : (uint32_t)j / (uint32_t)NC;
            const int ch = PLANAR ? c : (int)((uint32_t)j - (uint32_t)NC * p);
            tensor_store_elem<DT>(blk + e * ES, elem(src[p], ch));
        }
        return;
    }
    /* body: the block's elements converted into `dw`, packed, and stored as one 16-byte block */
    const uint32_t p0 = PLANAR ? (uint32_t)j0 : (uint32_t)j0 / (uint32_t)NC;
    uint32_t px[NP], dw[ND + 1];
    if (PLANAR) {
        __builtin_memcpy(px, src + p0, sizeof(px)); /* pixels p0 .. p0 + EPB - 1, all inside the row; dword-aligned only */
    } else {
        const uint32_t last = (uint32_t)d.width - 1u; /* the block may end inside pixel p0 + NP - 2: no read beyond the rectangle */
        for (int k = 0; k < NP; k++) px[k] = src[p0 + k < last ? p0 + k : last];
    }
    for (int k = 0; k <= ND; k++) dw[k] = 0;
    for (int m = 0; m < (PLANAR ? EPB : NC * NP); m++) {
        const uint32_t bits = PLANAR ? elem(px[m], c) : elem(px[m / NC], m % NC);
        dw[m * ES / 4] |= bits << (8 * (m * ES % 4));
    }
    tensor_u32x4 out;
    if (PLANAR) {
        out = tensor_u32x4{dw[0], dw[1], dw[2], dw[3]};
    } else {
        /* the block begins `r` elements into pixel p0: the packed stream shifted down by r elements */
        const uint32_t sb = ((uint32_t)j0 - (uint32_t)NC * p0) * ES;       /* bytes: 0..2, 0..4, 0..8; four channels: 0..3, 0..6, 0..12 */
        const uint32_t ds = ES == 1 ? 0u : sb >> 2, bs = ES == 4 ? 0u : sb & 3u;
        uint32_t o[4];
        for (int k = 0; k < 4; k++) {
            const int k1 = k + 1 < ND ? k + 1 : ND, k2 = k + 2 < ND ? k + 2 : ND, k3 = k + 3 < ND ? k + 3 : ND; /* dw[ND] = 0: never needed */
            const int k4 = k + 4 < ND ? k + 4 : ND;
            const uint32_t lo = ds == 0 ? dw[k] : (ds == 1 ? dw[k1] : (NC == 3 || ds == 2 ? dw[k2] : dw[k3]));
            const uint32_t hi = ds == 0 ? dw[k1] : (ds == 1 ? dw[k2] : (NC == 3 || ds == 2 ? dw[k3] : dw[k4]));
            o[k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bs));
        }
        out = tensor_u32x4{o[0], o[1], o[2], o[3]};
    }
    *(TENSOR_GLOBAL tensor_u32x4 *)blk = out;
}

#endif
