/* ffhip_webp.c -- host front end for lossy WebP (plain C, no GPU): the container walk of WEBP_load (format/webp.c:2016-2066), the
 * frame tag and key-frame header of WEBP_read_frame (:1872-1926), read_vp8_ctl_partition (:897-935) with read_dequantization
 * (:458-548) as ffhip_vp8_dequant_factors, and the two per-macroblock parsers of ffhip_vp8_bool.h looped as vp8_decode loops them
 * (:1833-1851).  What comes out is what ffhip_vp8_decode_items takes: mode records, levels, token counts, the residual map of the
 * skipped macroblocks, quantisers and filter parameters.  The contract is the reference's decoder bit for bit, not RFC 6386: every
 * departure from RFC 6386 and libwebp is a named flag of tests/vp8_spec.py, the refusal of some valid files among them. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip_webp_internal.h"
#include "ffhip_vp8_quant.h"

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t rd24(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }
static int is4(const uint8_t *p, const char *tag) { return memcmp(p, tag, 4) == 0; }

static int clamp127(int v) { return v < 0 ? 0 : v > 127 ? 127 : v; }

/* RFC 6386 section 14.1 */
static const uint16_t dc_q[128] = FFB_DC_Q;
static const uint16_t ac_q[128] = FFB_AC_Q;

int ffhip_vp8_dequant_factors(const ffhip_vp8_quant_header *h, uint16_t *out /* [4][8] */)
{
    if (!h || !out || h->y_ac_qi > 127) return FFHIP_EINVAL;
    memset(out, 0, 32 * sizeof(uint16_t));
    const int nseg = h->segmentation_enabled ? 4 : 1; /* webp.c:515: the other segments keep the zeros of the calloc'ed decoder */
    for (int i = 0; i < nseg; i++) {
        uint16_t quant = h->y_ac_qi; /* a uint16_t in the reference: a negative sum wraps and clamps to index 127 */
        if (h->segmentation_enabled) {
            if (!h->update_mb_segmentation_map) quant = (uint16_t)(quant + h->quantizer_update_value[i]); /* webp.c:518-522: this flag, */
            else quant = (uint16_t)h->quantizer_update_value[i];                                           /* not segment_feature_mode  */
        }
        uint16_t *q = out + 8 * i;
        q[0] = dc_q[clamp127((int)quant + h->y_dc_delta)];
        q[1] = ac_q[clamp127((int)quant)];
        q[2] = (uint16_t)(dc_q[clamp127((int)quant + h->y2_dc_delta)] * 2);
        q[3] = (uint16_t)(ac_q[clamp127((int)quant + h->y2_ac_delta)] * 155 / 100);
        q[4] = dc_q[clamp127((int)quant + h->uv_dc_delta)];
        q[5] = ac_q[clamp127((int)quant + h->uv_ac_delta)];
        if (q[2] > 132) q[2] = 132;
        if (q[3] < 8) q[3] = 8;
    }
    return FFHIP_OK;
}

/* WEBP_RULE_LIBWEBP: RFC 6386 section 9.6 / 14.1 as libwebp derives the factors (`_quant` of tests/vp8_spec.py): segment_feature_mode says
 * absolute or delta, every index and sum clamps to 0..127 as an int, all four segments are derived (without segmentation all from y_ac_qi),
 * and the cap of 132 sits on the chroma DC factor. */
static void quant_factors_libwebp(const ffhip_vp8_quant_header *h, int feature_mode, uint16_t *out /* [4][8] */)
{
    memset(out, 0, 32 * sizeof(uint16_t));
    for (int i = 0; i < 4; i++) {
        int q = h->y_ac_qi;
        if (h->segmentation_enabled) q = feature_mode ? h->quantizer_update_value[i] : q + h->quantizer_update_value[i];
        uint16_t *o = out + 8 * i;
        o[0] = dc_q[clamp127(q + h->y_dc_delta)];
        o[1] = ac_q[clamp127(q)];
        o[2] = (uint16_t)(dc_q[clamp127(q + h->y2_dc_delta)] * 2);
        o[3] = (uint16_t)(ac_q[clamp127(q + h->y2_ac_delta)] * 155 / 100);
        o[4] = dc_q[clamp127(q + h->uv_dc_delta)];
        o[5] = ac_q[clamp127(q + h->uv_ac_delta)];
        if (o[3] < 8) o[3] = 8;
        if (o[4] > 132) o[4] = 132;
    }
}

/* WEBP_RULE_LIBWEBP: section 9.6 / 15.2 (`_filters` of tests/vp8_spec.py): all four segments, and ONE clamp, behind the deltas. */
static void filter_params_libwebp(const ffhip_vp8_filter_header *h, uint8_t *filters /* [4][2][3] */, int *filter_type)
{
    const int ft = h->loop_filter_level == 0 ? 0 : (h->filter_type ? 1 : 2);
    *filter_type = ft;
    memset(filters, 0, 24);
    if (!ft) return;
    for (int s = 0; s < 4; s++)
        for (int b = 0; b < 2; b++) {
            int level = h->loop_filter_level;
            if (h->segmentation_enabled) level = h->segment_feature_mode ? h->lf_update_value[s] : level + h->lf_update_value[s];
            if (h->loop_filter_adj_enable) level += h->mode_ref_lf_delta0 + (b ? h->mb_mode_delta0 : 0);
            level = level < 0 ? 0 : level > 63 ? 63 : level;
            if (!level) continue;
            int il = level;
            if (h->sharpness_level) {
                il >>= h->sharpness_level > 4 ? 2 : 1;
                if (il > 9 - h->sharpness_level) il = 9 - h->sharpness_level;
            }
            if (il < 1) il = 1;
            uint8_t *f = filters + (s * 2 + b) * 3;
            f[0] = (uint8_t)(2 * level + il);
            f[1] = (uint8_t)il;
            f[2] = level >= 40 ? 2 : (level >= 15 ? 1 : 0);
        }
}

/* The chunk walk.  *vp8 = offset of the `VP8 ` chunk header, canvas[2] = the VP8X canvas fields as the reference reads them
 * (READ_UINT24 of the stored bytes, without the format's "+ 1"), 0 when there is no VP8X chunk. */
static inline int walk_chunks(const uint8_t *file, size_t len, size_t *vp8, uint32_t canvas[2], const int rule)
{
    if (len < 12 || !is4(file, "RIFF") || !is4(file + 8, "WEBP")) return FFHIP_EINVAL;
    size_t pos = 12;
    canvas[0] = canvas[1] = 0;
    while (pos + 4 <= len) {
        const uint8_t *c = file + pos;
        if (is4(c, "VP8X")) { /* struct webp_vp8x: 18 bytes, size field 10 (webp.c:2020-2030) */
            if (pos + 18 > len || rd32(c + 4) != 10) return FFHIP_EINVAL;
            if (c[8] & 2) return FFHIP_EWEBP_ANIMATION;
            canvas[0] = rd24(c + 12);
            canvas[1] = rd24(c + 15);
            pos += 18;
        } else if (rule != WEBP_RULE_LIBWEBP && is4(c, "ALPH")) { /* struct webp_alpha: 9 bytes, size field 1 (webp.c:2031-2039) */
            if (pos + 9 > len || rd32(c + 4) != 1) return FFHIP_EINVAL;
            pos += 9;
        } else if (is4(c, "VP8 ")) {
            if (pos + 8 > len) return FFHIP_EINVAL;
            *vp8 = pos;
            return FFHIP_OK;
        } else if (is4(c, "VP8L")) {
            return FFHIP_EWEBP_LOSSLESS;
        } else if (is4(c, "ANIM") || is4(c, "ANMF")) {
            return FFHIP_EWEBP_ANIMATION;
        } else { /* skipped by its size, without the format's padding byte (webp.c:2061-2065) */
            if (pos + 8 > len) return FFHIP_EINVAL;
            const uint32_t size = rd32(c + 4);
            if (size > len - pos - 8) return FFHIP_EINVAL;
            pos += 8 + (size_t)size;
            if (rule == WEBP_RULE_LIBWEBP) pos += size & 1; /* the format's padding byte; an ALPH chunk of any size is walked over like this too */
        }
    }
    return FFHIP_EINVAL; /* no VP8 chunk */
}

/* chunk header (8) + frame tag (3) + start code (3) + sizes (4) */
static int read_frame_tag(const uint8_t *file, size_t len, size_t vp8, uint32_t *p0_size, int *fw, int *fh)
{
    if (vp8 + 18 > len) return FFHIP_EINVAL;
    const uint8_t *t = file + vp8 + 8;
    if (t[0] & 1) return FFHIP_EWEBP_INTER_FRAME;
    if (t[3] != 0x9d || t[4] != 0x01 || t[5] != 0x2a) return FFHIP_EINVAL;
    *p0_size = (uint32_t)(t[0] >> 5) | ((uint32_t)t[1] | (uint32_t)t[2] << 8) << 3;
    *fw = (t[6] | t[7] << 8) & 0x3fff;
    *fh = (t[8] | t[9] << 8) & 0x3fff;
    if (*fw == 0 || *fh == 0) return FFHIP_EINVAL;
    return FFHIP_OK;
}

static inline void fill_dims(ffhip_webp_info *info, int fw, int fh, const uint32_t canvas[2], const int rule)
{
    if (rule == WEBP_RULE_LIBWEBP) { /* the frame tag's sizes are the picture */
        info->mbcols = (fw + 15) >> 4;
        info->mbrows = (fh + 15) >> 4;
        info->width = fw;
        info->height = fh;
        return;
    }
    const int w4 = ((fw + 3) >> 2) << 2, h4 = ((fh + 3) >> 2) << 2; /* webp.c:1810-1813 */
    info->mbcols = (w4 + 15) >> 4;
    info->mbrows = (h4 + 15) >> 4;
    info->width = canvas[0] ? (int)canvas[0] : w4; /* webp.c:2069-2074 */
    info->height = canvas[1] ? (int)canvas[1] : h4;
}

static inline int webp_probe_rule(const uint8_t *file, size_t len, int *width, int *height, int *mbcols, int *mbrows, const int rule)
{
    if (!file) return FFHIP_EINVAL;
    size_t vp8 = 0;
    uint32_t canvas[2], p0;
    int fw, fh;
    int rc = walk_chunks(file, len, &vp8, canvas, rule);
    if (rc) return rc;
    rc = read_frame_tag(file, len, vp8, &p0, &fw, &fh);
    if (rc) return rc;
    ffhip_webp_info info;
    fill_dims(&info, fw, fh, canvas, rule);
    if (width) *width = info.width;
    if (height) *height = info.height;
    if (mbcols) *mbcols = info.mbcols;
    if (mbrows) *mbrows = info.mbrows;
    return FFHIP_OK;
}

int ffhip_webp_probe(const uint8_t *file, size_t len, int *width, int *height, int *mbcols, int *mbrows)
{
    return webp_probe_rule(file, len, width, height, mbcols, mbrows, WEBP_RULE_REFERENCE);
}

int ffhip_webp_probe_ex(const uint8_t *file, size_t len, unsigned flags, int *width, int *height, int *mbcols, int *mbrows)
{
    if (flags & ~FFHIP_WEBP_PIXELS_LIBWEBP) return FFHIP_EINVAL;
    if (flags & FFHIP_WEBP_PIXELS_LIBWEBP) return webp_probe_rule(file, len, width, height, mbcols, mbrows, WEBP_RULE_LIBWEBP);
    return webp_probe_rule(file, len, width, height, mbcols, mbrows, WEBP_RULE_REFERENCE);
}

static inline int webp_read_header_rule(const uint8_t *file, size_t len, ffhip_webp_frame *f, const int rule)
{
    static const uint8_t update_probs[1056] = FFB_COEFF_UPDATE_PROBS;
    static const uint8_t default_probs[1056] = FFB_DEFAULT_COEFF_PROBS;
    if (!file || !f) return FFHIP_EINVAL;
    if (len >= 0xffffffffu) return FFHIP_EINVAL;
    memset(f, 0, sizeof *f);
    size_t vp8 = 0;
    uint32_t canvas[2], p0_size;
    int fw, fh;
    int rc = walk_chunks(file, len, &vp8, canvas, rule);
    if (rc) return rc;
    rc = read_frame_tag(file, len, vp8, &p0_size, &fw, &fh);
    if (rc) return rc;
    fill_dims(&f->info, fw, fh, canvas, rule);
    const size_t p0_off = vp8 + 18;
    f->p0_off = (uint32_t)p0_off;
    f->p0_len = (uint32_t)(p0_size <= len - p0_off ? p0_size : len - p0_off);

    ffb_dec d;
    ffb_init(&d, file + p0_off, f->p0_len);
    ffb_bit(&d, 128); /* color_space */
    ffb_bit(&d, 128); /* clamp */
    /* read_vp8_segmentation_adjust (webp.c:357-396) */
    ffhip_vp8_quant_header qh;
    ffhip_vp8_filter_header lh;
    memset(&qh, 0, sizeof qh);
    memset(&lh, 0, sizeof lh);
    const int seg_on = ffb_bit(&d, 128);
    int update_map = rule == WEBP_RULE_LIBWEBP ? 0 : 1; /* the reference: also when segmentation is off (webp.c:393) */
    if (rule == WEBP_RULE_LIBWEBP) f->mb.seg_prob[0] = f->mb.seg_prob[1] = f->mb.seg_prob[2] = 255; /* a tree probability the header does not set */
    if (seg_on) {
        update_map = ffb_bit(&d, 128);
        if (ffb_bit(&d, 128)) { /* update_segment_feature_data */
            lh.segment_feature_mode = (uint8_t)ffb_bit(&d, 128);
            for (int i = 0; i < 4; i++) qh.quantizer_update_value[i] = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 7) : 0;
            for (int i = 0; i < 4; i++) lh.lf_update_value[i] = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 6) : 0;
        }
        if (update_map)
            for (int i = 0; i < 3; i++)
                if (ffb_bit(&d, 128)) f->mb.seg_prob[i] = (uint8_t)ffb_bits(&d, 8);
    }
    f->mb.update_map = (uint8_t)update_map;
    qh.segmentation_enabled = lh.segmentation_enabled = (uint8_t)seg_on;
    qh.update_mb_segmentation_map = (uint8_t)update_map;
    lh.filter_type = (uint8_t)ffb_bit(&d, 128);
    lh.loop_filter_level = (uint8_t)ffb_bits(&d, 6);
    lh.sharpness_level = (uint8_t)ffb_bits(&d, 3);
    /* read_mb_lf_adjustments (webp.c:398-423) */
    lh.loop_filter_adj_enable = (uint8_t)ffb_bit(&d, 128);
    if (lh.loop_filter_adj_enable && ffb_bit(&d, 128)) {
        for (int i = 0; i < 4; i++) {
            const int v = ffb_bit(&d, 128) ? ffb_sbits(&d, 6) : 0;
            if (i == 0) lh.mode_ref_lf_delta0 = (int8_t)v;
        }
        for (int i = 0; i < 4; i++) {
            const int v = ffb_bit(&d, 128) ? ffb_sbits(&d, 6) : 0;
            if (i == 0) lh.mb_mode_delta0 = (int8_t)v;
        }
    }
    /* read_token_partition (webp.c:425-456): the sizes stand behind the first partition AS THE TAG GIVES ITS LENGTH */
    const int nparts = 1 << ffb_bits(&d, 2);
    if ((size_t)p0_size > len - p0_off || (size_t)3 * (nparts - 1) > len - p0_off - p0_size) return FFHIP_EINVAL; /* truncated */
    size_t next = p0_off + p0_size + (size_t)3 * (nparts - 1);
    /* the last partition ends with the file in the reference (webp.c:452-454); here with the chunk, where that is shorter */
    size_t end = len;
    const size_t chunk_end = vp8 + 8 + (size_t)rd32(file + vp8 + 4);
    for (int i = 0; i < nparts - 1; i++) {
        const uint32_t sz = rd24(file + p0_off + p0_size + 3 * i);
        if (sz > len - next) return FFHIP_EINVAL; /* a partition that points outside the file */
        f->part_off[i] = (uint32_t)next;
        f->part_len[i] = sz;
        next += sz;
    }
    if (chunk_end >= next && chunk_end < end) end = chunk_end;
    f->part_off[nparts - 1] = (uint32_t)next;
    f->part_len[nparts - 1] = (uint32_t)(end - next);
    f->info.nbr_partitions = nparts;
    lh.nbr_partitions = (uint8_t)nparts;
    /* read_dequantization (webp.c:458-548) */
    qh.y_ac_qi = (uint8_t)ffb_bits(&d, 7);
    qh.y_dc_delta = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 4) : 0;
    qh.y2_dc_delta = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 4) : 0;
    qh.y2_ac_delta = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 4) : 0;
    qh.uv_dc_delta = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 4) : 0;
    qh.uv_ac_delta = ffb_bit(&d, 128) ? (int8_t)ffb_sbits(&d, 4) : 0;
    /* read_token_proba_update (webp.c:550-894): refresh_entropy_probs first (:863) */
    ffb_bit(&d, 128);
    for (int i = 0; i < 1056; i++) f->probs[i] = ffb_bit(&d, update_probs[i]) ? (uint8_t)ffb_bits(&d, 8) : default_probs[i];
    f->mb.no_skip = (uint8_t)ffb_bit(&d, 128);
    f->mb.prob_skip = f->mb.no_skip ? (uint8_t)ffb_bits(&d, 8) : 0;
    if (d.err) return FFHIP_EINVAL; /* the header runs off the first partition */
    f->value = d.value;
    f->range = d.range;
    f->count = d.count;
    f->pos = d.pos;
    f->info.quant_header = qh;
    f->info.filter_header = lh;
    int ftype = 0;
    if (rule == WEBP_RULE_LIBWEBP) { /* segment_feature_mode travels in the filter header; the public structs stay as they are */
        quant_factors_libwebp(&qh, lh.segment_feature_mode, &f->info.quant[0][0]);
        filter_params_libwebp(&lh, &f->info.filters[0][0][0], &ftype);
        f->info.filter_type = ftype;
        return FFHIP_OK;
    }
    rc = ffhip_vp8_dequant_factors(&qh, &f->info.quant[0][0]);
    if (rc) return rc;
    rc = ffhip_vp8_filter_params(&lh, &f->info.filters[0][0][0], &ftype);
    if (rc) return rc;
    f->info.filter_type = ftype;
    return FFHIP_OK;
}

int ffhip_webp_read_header(const uint8_t *file, size_t len, ffhip_webp_frame *f) { return webp_read_header_rule(file, len, f, WEBP_RULE_REFERENCE); }
int ffhip_webp_read_header_libwebp(const uint8_t *file, size_t len, ffhip_webp_frame *f) { return webp_read_header_rule(file, len, f, WEBP_RULE_LIBWEBP); }

static inline int webp_parse_frame_rule(const uint8_t *file, const ffhip_webp_frame *f, uint8_t *modes, int16_t *levels, uint8_t *mbinfo, int32_t *resmap,
                                        const int rule)
{
    const int cols = f->info.mbcols, rows = f->info.mbrows, nparts = f->info.nbr_partitions;
    const size_t n_mb = (size_t)cols * rows;
    memset(levels, 0, n_mb * 400 * sizeof(int16_t));
    memset(mbinfo, 0, n_mb * 32);
    uint16_t *top = calloc((size_t)cols, sizeof *top);
    if (!top) return FFHIP_ENOMEM;
    ffb_dec hd, part[8];
    hd.p = file + f->p0_off;
    hd.len = f->p0_len;
    hd.pos = f->pos;
    hd.value = f->value;
    hd.range = f->range;
    hd.count = f->count;
    hd.err = 0;
    for (int i = 0; i < nparts; i++) ffb_init(&part[i], file + f->part_off[i], f->part_len[i]);
    int32_t last_coded = -1; /* the reference's coeffs[384] lives outside both loops (webp.c:1830): a skipped macroblock shows the last coded one's */
    for (int y = 0; y < rows; y++) {
        ffb_dec *bt = &part[y & (nparts - 1)];
        uint32_t left9 = 0, left4 = 0;
        for (int x = 0; x < cols; x++) {
            const size_t mb = (size_t)y * cols + x;
            uint8_t *rec = modes + mb * 20, *info = mbinfo + mb * 32;
            const uint32_t above4 = y > 0 ? ffb_rec_bottom4(rec - (size_t)cols * 20) : 0;
            const int skip = ffb_mb_header(&hd, &f->mb, above4, &left4, rec);
            const int has_y2 = rec[0] != 4;
            uint32_t top9 = top[x];
            if (!skip) {
                if (rule == WEBP_RULE_LIBWEBP) ffb_mb_tokens_libwebp(bt, f->probs, has_y2, &top9, &left9, levels + mb * 400, info);
                else ffb_mb_tokens(bt, f->probs, has_y2, &top9, &left9, levels + mb * 400, info);
                last_coded = (int32_t)mb;
                resmap[mb] = (int32_t)mb;
            } else {
                top9 = ffb_skip_ctx(top9, has_y2);
                left9 = ffb_skip_ctx(left9, has_y2);
                /* WEBP_RULE_LIBWEBP: a skipped macroblock has a zero residual: its own row, which nothing was written to */
                resmap[mb] = rule != WEBP_RULE_LIBWEBP && last_coded >= 0 ? last_coded : (int32_t)mb; /* none yet: its own row, all zeros (the reference reads an uninitialised array) */
            }
            top[x] = (uint16_t)top9;
            info[25] = (uint8_t)has_y2;
            info[26] = rec[18];
        }
    }
    free(top);
    int err = hd.err;
    for (int i = 0; i < nparts; i++) err |= part[i].err;
    return err ? FFHIP_EINVAL : FFHIP_OK; /* truncated: a partition was asked for a byte beyond its length */
}

int ffhip_webp_parse_frame(const uint8_t *file, const ffhip_webp_frame *f, uint8_t *modes, int16_t *levels, uint8_t *mbinfo, int32_t *resmap)
{
    return webp_parse_frame_rule(file, f, modes, levels, mbinfo, resmap, WEBP_RULE_REFERENCE);
}
int ffhip_webp_parse_frame_libwebp(const uint8_t *file, const ffhip_webp_frame *f, uint8_t *modes, int16_t *levels, uint8_t *mbinfo, int32_t *resmap)
{
    return webp_parse_frame_rule(file, f, modes, levels, mbinfo, resmap, WEBP_RULE_LIBWEBP);
}

int ffhip_webp_parse_ex(const uint8_t *file, size_t len, unsigned flags, ffhip_webp_parsed *out)
{
    if (flags & ~FFHIP_WEBP_PIXELS_LIBWEBP) return FFHIP_EINVAL;
    if (!file || !out || !out->modes || !out->levels || !out->mbinfo || !out->resmap) return FFHIP_EINVAL;
    const int libwebp = (flags & FFHIP_WEBP_PIXELS_LIBWEBP) != 0;
    ffhip_webp_frame f;
    const int rc = libwebp ? ffhip_webp_read_header_libwebp(file, len, &f) : ffhip_webp_read_header(file, len, &f);
    if (rc) return rc;
    if (out->n_mb_cap < (int64_t)f.info.mbcols * f.info.mbrows) return FFHIP_EINVAL;
    out->info = f.info;
    return libwebp ? ffhip_webp_parse_frame_libwebp(file, &f, out->modes, out->levels, out->mbinfo, out->resmap)
                   : ffhip_webp_parse_frame(file, &f, out->modes, out->levels, out->mbinfo, out->resmap);
}

int ffhip_webp_parse(const uint8_t *file, size_t len, ffhip_webp_parsed *out) { return ffhip_webp_parse_ex(file, len, 0u, out); }

struct webp_job {
    const uint8_t *const *files;
    const size_t *lens;
    ffhip_webp_parsed *outs;
    int *status;
    int first, last;
};
static void *webp_worker(void *arg)
{
    struct webp_job *jb = arg;
    for (int i = jb->first; i < jb->last; i++) jb->status[i] = ffhip_webp_parse(jb->files[i], jb->lens[i], &jb->outs[i]);
    return NULL;
}

int ffhip_webp_parse_batch(const uint8_t *const *files, const size_t *lens, int n, int n_threads, ffhip_webp_parsed *outs, int *status)
{
    if (n < 0 || (n > 0 && (!files || !lens || !outs || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n) n_threads = n;
    if (n_threads > 256) n_threads = 256;
    struct webp_job jobs[256];
    pthread_t tid[256];
    int started[256] = {0};
    for (int t = 0; t < n_threads; t++) {
        jobs[t] = (struct webp_job){files, lens, outs, status, (int)((long)n * t / n_threads), (int)((long)n * (t + 1) / n_threads)};
        if (t) started[t] = pthread_create(&tid[t], NULL, webp_worker, &jobs[t]) == 0;
    }
    webp_worker(&jobs[0]);
    for (int t = 1; t < n_threads; t++) {
        if (started[t]) pthread_join(tid[t], NULL);
        else webp_worker(&jobs[t]);
    }
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}
