/* ffhip_vp8l_internal.h -- what ffhip_vp8l.c and ffhip_vp8l_gpu.hip share besides include/ffpic_hip.h.  Plain C. */
#ifndef FFHIP_VP8L_INTERNAL_H
#define FFHIP_VP8L_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_vp8l_body.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A file whose container, header and transform list have been read: everything of it but the residual image.  The block images are the
 * transforms' sub-images as the stream holds them, one ARGB word a block, on the heap: ffhip_vp8l_close frees them */
typedef struct ffhip_vp8l_file {
    ffhip_vp8l_info info;
    ffhip_vp8l_steps steps;      /* the device form; valid while device_form */
    int device_form;             /* colour indexing absent, or the first transform of the file */
    const uint8_t *stream;       /* the VP8L chunk behind its signature byte */
    size_t stream_len;
    uint64_t image_bit;          /* where the residual image begins in it */
    uint32_t xsize[4];           /* by transform: the width of the image it is undone on */
    uint32_t *predictor_image, *cross_image;
    uint32_t predictor_words, cross_words;
    uint32_t palette[256];       /* 0x00000000 beyond the file's entries */
} ffhip_vp8l_file;

/* FFHIP_EINVAL for everything "lossless WebP" refuses in front of the residual image */
int ffhip_vp8l_open(const uint8_t *file, size_t len, ffhip_vp8l_file *pf);
void ffhip_vp8l_close(ffhip_vp8l_file *pf);
/* the residual image, info.residual_width x height words, into `residual` */
int ffhip_vp8l_read_residual(const ffhip_vp8l_file *pf, uint32_t *residual);
/* every transform undone on the host by the functions of ffhip_vp8l_body.h: residual -> width x height ARGB words at `argb` (rows
 * packed), the alpha rule not yet applied.  residual is used up */
int ffhip_vp8l_invert_host(const ffhip_vp8l_file *pf, uint32_t *residual, uint32_t *argb);

#ifdef __cplusplus
}
#endif

#endif
