/* ffhip_jpeg_enc_internal.h -- what the host side of the JPEG encoder (ffhip_jpeg_enc.c) gives the device calls (ffhip_jpeg_enc_gpu.hip):
 * the argument checks, a picture's geometry, the header's bytes and the code tables in the form the block code reads. */
#ifndef FFHIP_JPEG_ENC_INTERNAL_H
#define FFHIP_JPEG_ENC_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_jpeg_enc_body.h"

typedef struct ffhip_jenc_geometry {
    int h, v, ncomp;
    int mcu_cols, mcu_rows;
    int bpm;        /* blocks of an MCU in the scan */
    int64_t mcus, blocks;
} ffhip_jenc_geometry;

#ifdef __cplusplus
extern "C" {
#endif
int ffhip_jenc_params_ok(int width, int height, int layout, int restart);
int ffhip_jenc_source_ok(const ffhip_jpeg_source *s, int layout); /* everything but where `pixels` lives */
void ffhip_jenc_geom(int width, int height, int layout, ffhip_jenc_geometry *g);
size_t ffhip_jenc_header(int width, int height, int layout, int quality, int restart, uint8_t *out /* FFHIP_JPEG_ENC_HEADER_MAX */);
void ffhip_jenc_code_tables(uint32_t *tab /* [2][JE_TAB_WORDS] */);
#ifdef __cplusplus
}
#endif

#endif
