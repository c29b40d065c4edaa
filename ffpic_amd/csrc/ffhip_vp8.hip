/*
 * ffhip_vp8.hip -- VP8 (WebP lossy) residual stage for batches of macroblocks:
 * dequantisation, inverse WHT of the Y2 block and the 4x4 inverse DCTs, bit-exact with
 *   vp8_get_coefficients' dequant store   format/webp.c:1061
 *   IWHT_long / IWHT_fast                 format/webp.c:1067-1106
 *   idct_4x4_16                           utils/idct.c:100-151
 *   the per-MB assembly                   format/webp.c:1147-1196
 * including the reference's rule that a block is transformed only when more than one
 * token was read or its DC is non-zero (webp.c:1172,1188).
 *
 * HBM-bound byte/integer work: 800 B of levels + 32 B of info in, 768 B of residual out
 * per macroblock (6.25 B/pixel).  32 lanes own one macroblock and move its bytes linearly, 16 per lane
 * and instruction; blocks are assembled inside lane pairs (k_vp8_residual); the Y2 lane hands the 16 DC values
 * to the luma lanes of the same wave through LDS (in-order within a wave, no barrier).
 */
#include "ffhip_internal.h"

struct Vp8ResArgs {
    const int16_t *levels; /* [n_mb][25][16] */
    const uint8_t *info;   /* [n_mb][32]: nz[25], has_y2, segment */
    const uint16_t *quant; /* [4][8]: y1_dc y1_ac y2_dc y2_ac uv_dc uv_ac - - */
    int16_t *out;          /* [n_mb][24][16] */
    long long n_mb;
};

/* x is an int16 value here and k < 2^16: the product fits 32 bits and is a full-rate v_mul_i32_i24 (v_mul_lo_u32 runs at a quarter of the rate) */
__device__ __forceinline__ int vp8_mul(int x, int k) { return __mul24(x, k) >> 16; }

__device__ __forceinline__ u32 pk_add(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(s16x2, a) + __builtin_bit_cast(s16x2, b)); }
__device__ __forceinline__ u32 pk_sub(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b)); }
/* ((x * k) >> 16) of both int16 halves: two 24-bit multiplies, the shift is the byte pick of one v_perm */
__device__ __forceinline__ u32 vp8_mul_pair(u32 x, int k)
{
    const int plo = __mul24((int)(short)(x & 0xffffu), k), phi = __mul24((int)x >> 16, k);
    return __builtin_amdgcn_perm((u32)phi, (u32)plo, 0x07060302u);
}

/* utils/idct.c:100-151 on packed pairs p[2r + h] = (c[4r + 2h], c[4r + 2h + 1]).  The vertical pass only ever
 * keeps int16 (idct.c:124 truncates its results), so it runs on two columns at a time in 16-bit lanes: sums
 * wrap exactly like the low halves of the reference's int sums, and every (x * k) >> 16 fits 16 bits.  The
 * horizontal pass needs the bits above 16 for its (.. + 4) >> 3 and stays in 32 bits. */
__device__ __forceinline__ void vp8_idct4x4(u32 p[8])
{
    u32 T[8];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const u32 x0 = p[h], x1 = p[2 + h], x2 = p[4 + h], x3 = p[6 + h];
        const u32 s = pk_add(x0, x2), d = pk_sub(x0, x2);
        const u32 lo = pk_sub(pk_sub(vp8_mul_pair(x1, 35468), x3), vp8_mul_pair(x3, 20091));
        const u32 hi = pk_add(pk_add(x1, vp8_mul_pair(x1, 20091)), vp8_mul_pair(x3, 35468));
        T[h] = pk_add(s, hi); T[2 + h] = pk_add(d, lo); T[4 + h] = pk_sub(d, lo); T[6 + h] = pk_sub(s, hi);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int x0 = (short)(T[2 * r] & 0xffffu), x1 = (int)T[2 * r] >> 16, x2 = (short)(T[2 * r + 1] & 0xffffu), x3 = (int)T[2 * r + 1] >> 16;
        const int s = x0 + x2, d = x0 - x2;
        const int lo = vp8_mul(x1, 35468) - x3 - vp8_mul(x3, 20091);
        const int hi = x1 + vp8_mul(x1, 20091) + vp8_mul(x3, 35468);
        p[2 * r] = __builtin_amdgcn_perm((u32)((d + lo + 4) >> 3), (u32)((s + hi + 4) >> 3), 0x05040100u);
        p[2 * r + 1] = __builtin_amdgcn_perm((u32)((s - hi + 4) >> 3), (u32)((d - lo + 4) >> 3), 0x05040100u);
    }
}

/* Four dwords per lane, picked inside every lane pair in ONE instruction each (v_cndmask_b32 with a DPP source operand):
 * lanes in `own` keep s1, the others take s0 of the pair's even (FROM_ODD = false: quad_perm [0,0,2,2]) or odd ([1,1,3,3])
 * lane.  A v_mov_b32_dpp broadcast followed by a v_cndmask, as the compiler writes the same thing, is twice the VALU
 * work: 32 of this kernel's 276 instructions.  (s_nop 1: the two wait states a DPP read needs after the VALU write of
 * its source, which the hazard pass cannot insert inside an asm block.) */
template <bool FROM_ODD>
__device__ __forceinline__ u32x4 pair_pick(u32x4 s0, u32x4 s1, unsigned long long own)
{
    u32 d0, d1, d2, d3;
    if (FROM_ODD)
        asm("s_mov_b64 vcc, %12\n\ts_nop 1\n\t"
            "v_cndmask_b32_dpp %0, %4, %8, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %1, %5, %9, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %2, %6, %10, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %3, %7, %11, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf"
            : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)
            : "v"(s0[0]), "v"(s0[1]), "v"(s0[2]), "v"(s0[3]), "v"(s1[0]), "v"(s1[1]), "v"(s1[2]), "v"(s1[3]), "s"(own)
            : "vcc");
    else
        asm("s_mov_b64 vcc, %12\n\ts_nop 1\n\t"
            "v_cndmask_b32_dpp %0, %4, %8, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %1, %5, %9, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %2, %6, %10, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_dpp %3, %7, %11, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf"
            : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)
            : "v"(s0[0]), "v"(s0[1]), "v"(s0[2]), "v"(s0[3]), "v"(s1[0]), "v"(s1[1]), "v"(s1[2]), "v"(s1[3]), "s"(own)
            : "vcc");
    return u32x4{d0, d1, d2, d3};
}

/* 32 lanes own one macroblock.  Memory moves LINEARLY: lane t loads 16-byte chunk t of the macroblock's 800 bytes of
 * levels and chunk 32 + t (t < 18), and stores chunk t and chunk 32 + t (t < 16) of its 768 bytes of residual, so
 * every vector memory instruction covers one contiguous run -- with a block (two chunks) per lane straight from
 * memory, each instruction touched half of every 64-byte segment, which held the kernel at 5.1 TB/s where the same
 * arithmetic over linear accesses measures 5.7-5.9.  Blocks are then assembled inside lane PAIRS with two DPP
 * broadcasts: even lane 2b computes luma block b from chunks 2b (its own) and 2b + 1 (its neighbour's); odd lane
 * 2j + 1 computes block 16 + j (U/V blocks 16-23, the Y2 block 24 on lane 17) from chunks 32 + 2j (its neighbour's
 * second load) and 32 + 2j + 1 (its own).  The results go back the same way (pair_pick). */
template <bool PATTERN> /* PATTERN: the loads and the stores without the arithmetic (diagnostics, FFHIP_VP8_RESIDUAL_PATTERN=1: the kernel's access pattern as its ceiling) */
__global__ __launch_bounds__(256) void k_vp8_residual(Vp8ResArgs a)
{
    __shared__ __attribute__((aligned(16))) short y2in[8][16];
    __shared__ __attribute__((aligned(16))) int y2t[8][16];
    const int t = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long long mb = (long long)blockIdx.x * 8 + slot;
    if (mb >= a.n_mb) return; /* whole 32-lane slots: the lane pairs below are never split */
#include "ffhip_vp8_residual_body.inc"
}

/* ffhip_vp8_decode_items: the macroblocks of all its levels items end to end, each 32-lane slot with its own item's buffers and
 * quantisers.  The body is k_vp8_residual's as included text (a forceinline function changed the JPEG kernels' register allocation).
 * A workgroup reads the item of its first macroblock from the per-workgroup table; a slot's item is that one or a later one (items
 * of fewer than eight macroblocks end inside a workgroup), found by walking the items' prefix. */
__global__ __launch_bounds__(256) void k_vp8_residual_items(const Vp8ResItem *items, const u32 *wg_item, long long n_mb_all)
{
    constexpr bool PATTERN = false;
    __shared__ __attribute__((aligned(16))) short y2in[8][16];
    __shared__ __attribute__((aligned(16))) int y2t[8][16];
    const int t = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long long gmb = (long long)blockIdx.x * 8 + slot;
    if (gmb >= n_mb_all) return;
    typedef __attribute__((address_space(4))) const Vp8ResItem cres;
    typedef __attribute__((address_space(4))) const u32 cu32;
    const int it0 = (int)((cu32 *)wg_item)[blockIdx.x];
    if ((long long)blockIdx.x * 8 + 7 < ((cres *)items)[it0 + 1].first) {
        /* the whole workgroup in one item (every workgroup but those at an item's end): its record by scalar loads -- a chain of
         * vector loads in front of the levels made this short-lived kernel 7 % slower than k_vp8_residual */
        cres *const d = (cres *)items + it0;
        const Vp8ResArgs a = {d->levels, d->info, items[it0].quant, d->out, 0};
        const long long mb = gmb - d->first;
#include "ffhip_vp8_residual_body.inc"
    } else {
        int it = it0;
        while (gmb >= items[it + 1].first) it++; /* (the sentinel behind the last item holds the total) */
        const Vp8ResItem &d = items[it];
        const Vp8ResArgs a = {d.levels, d.info, d.quant, d.out, 0};
        const long long mb = gmb - d.first;
#include "ffhip_vp8_residual_body.inc"
    }
}

/* one workgroup per item: its index over the workgroups whose first macroblock is its own (as k_jpeg_items_table) */
__global__ __launch_bounds__(256) void k_vp8_residual_items_table(const Vp8ResItem *items, u32 *wg_item)
{
    const long long b0 = (items[blockIdx.x].first + 7) / 8, b1 = (items[blockIdx.x + 1].first + 7) / 8;
    for (long long b = b0 + threadIdx.x; b < b1; b += 256) wg_item[b] = blockIdx.x;
}

int vp8_residual_items_enqueue(const Vp8ResItem *d_items, int n, long long n_mb, uint32_t *d_wg_item, void *stream)
{
    hipLaunchKernelGGL(k_vp8_residual_items_table, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, d_items, d_wg_item);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    hipLaunchKernelGGL(k_vp8_residual_items, dim3((unsigned)((n_mb + 7) / 8)), dim3(256), 0, (hipStream_t)stream, d_items, d_wg_item, n_mb);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}

extern "C" int ffhip_vp8_residual_batch(long long n_mb, const int16_t *d_levels, const uint8_t *d_mbinfo,
                                        const uint16_t *d_quant, int16_t *d_residual, void *stream)
{
    if (n_mb < 0) return FFHIP_EINVAL;
    if (n_mb == 0) return FFHIP_OK;
    if (!d_levels || !d_mbinfo || !d_quant || !d_residual) return FFHIP_EINVAL;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_residual & 15) || ((uintptr_t)d_mbinfo & 3) || ((uintptr_t)d_quant & 3) || n_mb > 0x7fffffffLL * 8)
        return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    Vp8ResArgs a = {d_levels, d_mbinfo, d_quant, d_residual, n_mb};
    if (FFHIP_ENV("FFHIP_VP8_RESIDUAL_PATTERN")) hipLaunchKernelGGL(k_vp8_residual<true>, dim3((unsigned)((n_mb + 7) / 8)), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_vp8_residual<false>, dim3((unsigned)((n_mb + 7) / 8)), dim3(256), 0, (hipStream_t)stream, a);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}
