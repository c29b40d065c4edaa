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
/* k_deflate_chunks over `total` chunks of the device records; wg_item: the per-chunk table (k_items_table<ffhip_def_stream>'s, or the chunk half of k_items_tables2's).  Only enqueues */
int ffhip_deflate_chunks_enqueue(const ffhip_def_stream *d_streams, const uint32_t *d_wg_item, unsigned long long total, void *stream);
#endif

#endif
