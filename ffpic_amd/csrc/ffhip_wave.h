/* ffhip_wave.h -- device helpers of the kernels that walk a band of rows, a lane a row (ffhip_staged.h), of whoever else hands a register
 * to the next lane, and the workgroup prefix sum of the encoders' scan, count and copy kernels. */
#ifndef FFHIP_WAVE_H
#define FFHIP_WAVE_H

#include "ffhip_internal.h"

/* wave_shr:1 -- lane r gets lane r - 1's v; lane 0: 0 */
template <class T> __device__ __forceinline__ T wave_shr1(T v) { return (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }

/* byte i (static) of a run of dwords */
template <int N> __device__ __forceinline__ int byte_of(const u32 (&w)[N], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

/* exclusive prefix sum of v over a workgroup of WG threads; *total: the sum; wave_sum: WG / 64 words of LDS */
template <int WG> __device__ static inline u32 wg_scan(u32 v, u32 *wave_sum, u32 *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    u32 before = 0, all = 0;
    for (int w = 0; w < WG / 64; w++) {
        if (w < wave) before += wave_sum[w];
        all += wave_sum[w];
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

#endif
