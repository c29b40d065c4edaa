/* ffhip_wave.h -- two device helpers of the kernels that walk a band of rows, a lane a row (ffhip_staged.h), and of whoever else hands a
 * register to the next lane. */
#ifndef FFHIP_WAVE_H
#define FFHIP_WAVE_H

#include "ffhip_internal.h"

/* wave_shr:1 -- lane r gets lane r - 1's v; lane 0: 0 */
template <class T> __device__ __forceinline__ T wave_shr1(T v) { return (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }

/* byte i (static) of a run of dwords */
template <int N> __device__ __forceinline__ int byte_of(const u32 (&w)[N], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

#endif
