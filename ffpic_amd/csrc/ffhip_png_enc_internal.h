/* ffhip_png_enc_internal.h -- what ffhip_png_enc.c and ffhip_png_enc_gpu.hip share: the argument checks and the file's first bytes */
#ifndef FFHIP_PNG_ENC_INTERNAL_H
#define FFHIP_PNG_ENC_INTERNAL_H

#include "ffhip_png_enc_body.h"
#include "ffhip_deflate_internal.h"

#ifdef __cplusplus
extern "C" {
#endif
int ffhip_pngenc_source_ok(const ffhip_png_source *s, int filter);
void ffhip_pngenc_header(int width, int height, int channels, uint8_t out[FFHIP_PE_HEADER]); /* signature and IHDR */
#ifdef __cplusplus
}
#endif

#endif
