/* ffhip_webp_alpha_internal.h -- what ffhip_webp_alpha.c and ffhip_webp_alpha_gpu.hip share besides include/ffpic_hip.h.  Plain C. */
#ifndef FFHIP_WEBP_ALPHA_INTERNAL_H
#define FFHIP_WEBP_ALPHA_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_vp8l_internal.h"
#include "ffhip_webp_alpha_body.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the chunk walk and the ALPH header byte say.  has_alpha 0: the file stays opaque, nothing else is set */
typedef struct ffhip_webp_alpha_head {
    int has_alpha, compression, filter, pre_processing;
    uint32_t width, height; /* the frame tag's */
    const uint8_t *data;    /* the payload behind the header byte: width x height bytes, or a headerless VP8L stream */
    size_t data_len;
} ffhip_webp_alpha_head;

/* The libwebp rule's chunk walk (ffhip_webp.c, walk_chunks) with two things remembered on the way to the `VP8 ` chunk: the VP8X flag byte
 * and the first ALPH chunk behind it.  The walk's own verdicts for a file it refuses; FFHIP_EINVAL for a refused ALPH header byte or a
 * short raw plane.  Every pointer it leaves lies inside file[0 .. len) */
int ffhip_webp_alpha_find(const uint8_t *file, size_t len, ffhip_webp_alpha_head *out);

#ifdef __cplusplus
}
#endif

#endif
