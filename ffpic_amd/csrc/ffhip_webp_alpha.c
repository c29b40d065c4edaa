/*
 * ffhip_webp_alpha.c -- the host side of FFHIP_WEBP_ALPHA (include/ffpic_hip.h, "lossy WebP, the alpha plane"): the chunk
 * walk that finds a lossy file's ALPH chunk, its header byte, the probe, and ffhip_webp_alpha_plane, the whole alpha decode on the host:
 * a raw plane as it stands or a headerless VP8L stream through ffhip_vp8l_open_stream / ffhip_vp8l_read_residual /
 * ffhip_vp8l_invert_host, then the filter undone by the function of ffhip_webp_alpha_body.h that k_webp_alpha_unfilter compiles too.
 * Plain C11, no HIP.
 */
#include "ffhip_webp_alpha_internal.h"

#include <stdlib.h>
#include <string.h>

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static int is4(const uint8_t *p, const char *tag) { return memcmp(p, tag, 4) == 0; }

int ffhip_webp_alpha_find(const uint8_t *file, size_t len, ffhip_webp_alpha_head *out)
{
    memset(out, 0, sizeof(*out));
    if (!file || len < 12 || !is4(file, "RIFF") || !is4(file + 8, "WEBP")) return FFHIP_EINVAL;
    size_t pos = 12, vp8 = 0;
    const uint8_t *alph = NULL;
    uint32_t alph_size = 0;
    int vp8x = -1; /* the first VP8X chunk's flag byte */
    while (!vp8) {
        if (pos + 4 > len) return FFHIP_EINVAL; /* no VP8 chunk */
        const uint8_t *c = file + pos;
        if (is4(c, "VP8X")) {
            if (pos + 18 > len || rd32(c + 4) != 10) return FFHIP_EINVAL;
            if (c[8] & 2) return FFHIP_EWEBP_ANIMATION;
            if (vp8x < 0) vp8x = c[8];
            pos += 18;
        } else if (is4(c, "VP8 ")) {
            if (pos + 18 > len) return FFHIP_EINVAL;
            vp8 = pos;
        } else if (is4(c, "VP8L")) {
            return FFHIP_EWEBP_LOSSLESS;
        } else if (is4(c, "ANIM") || is4(c, "ANMF")) {
            return FFHIP_EWEBP_ANIMATION;
        } else {
            if (pos + 8 > len) return FFHIP_EINVAL;
            const uint32_t size = rd32(c + 4);
            if (size > len - pos - 8) return FFHIP_EINVAL;
            if (is4(c, "ALPH") && !alph && vp8x >= 0) { alph = c + 8; alph_size = size; }
            pos += 8 + (size_t)size + (size & 1);
        }
    }
    const uint8_t *t = file + vp8 + 8; /* the frame tag, start code and sizes */
    if (t[0] & 1) return FFHIP_EWEBP_INTER_FRAME;
    if (t[3] != 0x9d || t[4] != 0x01 || t[5] != 0x2a) return FFHIP_EINVAL;
    const uint32_t w = (uint32_t)(t[6] | t[7] << 8) & 0x3fff, h = (uint32_t)(t[8] | t[9] << 8) & 0x3fff;
    if (!w || !h) return FFHIP_EINVAL;
    if (!alph || !(vp8x & 0x10)) return FFHIP_OK;
    if (alph_size < 1) return FFHIP_EINVAL;
    const int head = alph[0];
    out->compression = head & 3;
    out->filter = (head >> 2) & 3;
    out->pre_processing = (head >> 4) & 3;
    out->width = w;
    out->height = h;
    out->data = alph + 1;
    out->data_len = alph_size - 1;
    if (out->compression > 1 || out->pre_processing > 1 || (head >> 6)) return FFHIP_EINVAL;
    if (out->compression == 0 && out->data_len < (size_t)w * h) return FFHIP_EINVAL; /* longer: the excess is ignored */
    out->has_alpha = 1;
    return FFHIP_OK;
}

int ffhip_webp_alpha_probe(const uint8_t *file, size_t len, int *has_alpha, int *compression, int *filter, int *pre_processing)
{
    if (!file || !has_alpha || !compression || !filter || !pre_processing) return FFHIP_EINVAL;
    ffhip_webp_alpha_head a;
    const int rc = ffhip_webp_alpha_find(file, len, &a);
    *has_alpha = rc ? 0 : a.has_alpha;
    *compression = rc || !a.has_alpha ? 0 : a.compression;
    *filter = rc || !a.has_alpha ? 0 : a.filter;
    *pre_processing = rc || !a.has_alpha ? 0 : a.pre_processing;
    return rc;
}

int ffhip_webp_alpha_plane(const uint8_t *file, size_t len, uint8_t *alpha, int64_t pitch)
{
    if (!file || !alpha) return FFHIP_EINVAL;
    ffhip_webp_alpha_head a;
    int rc = ffhip_webp_alpha_find(file, len, &a);
    if (rc) return rc;
    if (!a.has_alpha) return FFHIP_EINVAL; /* no plane to give */
    const uint32_t w = a.width, h = a.height;
    if (pitch < (int64_t)w) return FFHIP_EINVAL;
    const uint8_t *src = a.data;
    int64_t src_pitch = w;
    int step = 1;
    uint32_t *res = NULL, *argb = NULL;
    ffhip_vp8l_file *pf = NULL;
    if (a.compression == 1) {
        if (!(pf = (ffhip_vp8l_file *)malloc(sizeof(*pf)))) return FFHIP_ENOMEM;
        rc = ffhip_vp8l_open_stream(a.data, a.data_len, (int32_t)w, (int32_t)h, 0, 1, pf);
        if (rc) { free(pf); return rc; }
        if (!(res = (uint32_t *)malloc((size_t)pf->info.residual_width * h * 4)) || !(argb = (uint32_t *)malloc((size_t)w * h * 4))) rc = FFHIP_ENOMEM;
        if (!rc) rc = ffhip_vp8l_read_residual(pf, res);
        if (!rc) rc = ffhip_vp8l_invert_host(pf, res, argb);
        src = (const uint8_t *)argb + 1; /* the green byte of each word: little-endian hosts, the library's only kind */
        src_pitch = 4 * (int64_t)w;
        step = 4;
    }
    if (!rc) {
        if (a.filter) {
            ffhip_webp_alpha_unfilter_rows(src, src_pitch, step, a.filter, w, h, alpha, pitch);
        } else {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) alpha[(int64_t)y * pitch + x] = src[(int64_t)y * src_pitch + (int64_t)x * step];
        }
    }
    free(res);
    free(argb);
    if (pf) ffhip_vp8l_close(pf);
    free(pf);
    return rc;
}
