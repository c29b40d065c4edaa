/* ffhip_vp8l_enc_internal.h -- what ffhip_vp8l_enc.c and ffhip_vp8l_enc_gpu.hip share: the rule's body and the argument check */
#ifndef FFHIP_VP8L_ENC_INTERNAL_H
#define FFHIP_VP8L_ENC_INTERNAL_H

#include "ffhip_vp8l_enc_body.h"
#include "ffhip_png_enc_internal.h" /* ffhip_pngenc_source_ok: the source record is the PNG encoder's */

#ifdef __cplusplus
extern "C" {
#endif
int ffhip_vp8lenc_source_ok(const ffhip_png_source *s, int flags); /* sides 1..16384, flags within the two */
#ifdef __cplusplus
}
#endif

#endif
