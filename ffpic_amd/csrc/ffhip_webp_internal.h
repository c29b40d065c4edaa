/* ffhip_webp_internal.h -- what the host front end (ffhip_webp.c) hands the device front end (ffhip_vp8_bool_gpu.hip): a lossy WebP's
 * frame header, parsed up to prob_skip_false (read_vp8_ctl_partition, format/webp.c:897-935), with the first partition's decoder
 * state at that point. */
#ifndef FFHIP_WEBP_INTERNAL_H
#define FFHIP_WEBP_INTERNAL_H

#include "ffhip_vp8_bool.h"
#include "ffpic_hip.h"

typedef struct ffhip_webp_frame {
    ffhip_webp_info info;
    uint32_t p0_off, p0_len;             /* the first partition: offset in the file, bytes of it that are in the file */
    uint32_t value, range, pos;          /* its decoder behind the frame header (pos counts from p0_off) */
    int32_t count;
    ffb_mbhdr_probs mb;
    uint32_t part_off[8], part_len[8];   /* the token partitions, offsets in the file */
    uint8_t probs[1056];                 /* coeff_prob [4][8][3][11] */
} ffhip_webp_frame;

#ifdef __cplusplus
extern "C" {
#endif
/* container walk + frame header; every offset it leaves lies inside [0, len) */
int ffhip_webp_read_header(const uint8_t *file, size_t len, ffhip_webp_frame *out);
/* the two macroblock loops on the host, behind ffhip_webp_read_header */
int ffhip_webp_parse_frame(const uint8_t *file, const ffhip_webp_frame *f, uint8_t *modes, int16_t *levels, uint8_t *mbinfo, int32_t *resmap);
/* the same two under WEBP_RULE_LIBWEBP (ffhip_vp8_bool.h): the frame tag's sizes, the padded chunk walk, segment ids only where they are coded,
 * quantisers and filter parameters by RFC 6386, the identity residual map; info.quant / .filters hold the spec-derived values */
int ffhip_webp_read_header_libwebp(const uint8_t *file, size_t len, ffhip_webp_frame *out);
int ffhip_webp_parse_frame_libwebp(const uint8_t *file, const ffhip_webp_frame *f, uint8_t *modes, int16_t *levels, uint8_t *mbinfo, int32_t *resmap);
#ifdef __cplusplus
}
#endif

#endif
