/* ffhip_deflate_internal.h -- what the deflate entries share with the PNG encoder (ffhip_deflate.c, ffhip_deflate_gpu.hip, ffhip_png_enc.c,
 * ffhip_png_enc_gpu.hip) */
#ifndef FFHIP_DEFLATE_INTERNAL_H
#define FFHIP_DEFLATE_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_deflate_body.h"

#ifdef __cplusplus
extern "C" {
#endif
/* host: every chunk of src[0 .. len) through ffhip_def_chunk.  *out: n_chunks x FFHIP_DEF_OUT_BYTES, chunk c's output at c x
 * FFHIP_DEF_OUT_BYTES; *res: n_chunks results; both malloc'ed, the caller frees them.  FFHIP_ENOMEM or FFHIP_OK */
int ffhip_deflate_chunks_host(const uint8_t *src, size_t len, uint8_t **out, ffhip_def_result **res, uint64_t *n_chunks);
#ifdef __cplusplus
}
#endif

/* device: one stream's chunks for k_deflate_chunks.  Chunk c reads src[c x CHUNK ..), and matches reach back to src[0]; tok: len words;
 * out: n_wgs x FFHIP_DEF_OUT_BYTES, zeroed by the call; res: n_wgs results */
typedef struct ffhip_def_stream {
    const uint8_t *src;
    unsigned long long len;
    uint32_t *tok, *out;
    ffhip_def_result *res;
    uint32_t first_wg, n_wgs; /* its chunks among the call's */
} ffhip_def_stream;
#ifdef __cplusplus
/* k_deflate_chunks over `total` chunks of the device records; wg_item: the per-chunk table (k_items_table<ffhip_def_stream>'s).  Only enqueues */
int ffhip_deflate_chunks_enqueue(const ffhip_def_stream *d_streams, const uint32_t *d_wg_item, unsigned long long total, void *stream);
#endif

#ifdef __HIPCC__
/* exclusive prefix sum of v over a workgroup of WG threads; *total: the sum; wave_sum: WG / 64 words of LDS */
template <int WG> __device__ static inline uint32_t ffhip_def_wg_scan(uint32_t v, uint32_t *wave_sum, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < WG / 64; w++) {
        if (w < wave) before += wave_sum[w];
        all += wave_sum[w];
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}
#endif

#endif
