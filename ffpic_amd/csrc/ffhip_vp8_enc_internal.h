/* ffhip_vp8_enc_internal.h -- what ffhip_vp8_enc.c and ffhip_vp8_enc_gpu.hip share: the rule's body, the argument check and the steps of a
 * quantiser index */
#ifndef FFHIP_VP8_ENC_INTERNAL_H
#define FFHIP_VP8_ENC_INTERNAL_H

#include "ffhip_vp8_enc_body.h"

#ifdef __cplusplus
extern "C" {
#endif
int ffhip_vp8enc_source_ok(const ffhip_jpeg_source *s); /* 1 or 3 channels, sides 1..16383; everything but where `pixels` lives */
int ffhip_vp8enc_params_ok(int quality, int filter);    /* 0..100; -1..63 */
void ffhip_vp8enc_steps(int y_ac_qi, uint16_t *q /* [6] */);
#ifdef __cplusplus
}
#endif

#endif
