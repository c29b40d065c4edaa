/* ffhip_jpeg_prog_internal.h -- what ffhip_jpeg_progressive.c shares with the device front end (ffhip_huff_prog_gpu.hip) and the file
 * calls (ffhip_pipeline.hip): the parsed progressive file with its scan list.  Internal to libffpic_hip.so. */
#ifndef FFHIP_JPEG_PROG_INTERNAL_H
#define FFHIP_JPEG_PROG_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_jpeg_prog_body.h"

#ifdef __cplusplus
extern "C" {
#endif

struct prog_file {
    struct jpeg_frame fr;
    int n_scans;
    struct prog_scan scan[FFHIP_JPEG_MAX_SCANS]; /* pic, data and seg_base are the decoder's to fill in; tab[] indexes `tabs` */
    const uint8_t *raw[FFHIP_JPEG_MAX_SCANS];    /* each scan's entropy-coded bytes in the file */
    size_t raw_len[FFHIP_JPEG_MAX_SCANS];
    struct huff *tabs;                           /* the snapshots, malloc'd: ffhip_prog_free */
    int n_tabs, cap_tabs;
};

int ffhip_prog_parse(const uint8_t *file, size_t len, struct prog_file *pf); /* 0, FFHIP_EINVAL or FFHIP_ENOMEM (nothing to free then) */
void ffhip_prog_free(struct prog_file *pf);
int ffhip_prog_k_eff(const struct prog_file *pf, int k_max); /* scans with Ss above this are skipped */
uint32_t ffhip_prog_stage_scan(uint8_t *dst, const uint8_t *src, size_t len, uint32_t *seg, uint32_t n_seg);
int ffhip_prog_decode_host(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v,
                           uint16_t *quant, int k_max, int counts[3]);
void ffhip_prog_note_last(const int v[5]); /* what ffhip_debug_progressive_last reports for the calling thread */

#ifdef __cplusplus
}
#endif
#endif
