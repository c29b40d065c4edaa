/* ffhip_vp8l_enc.c -- the host side of the lossless WebP encoder (include/ffpic_hip.h "Lossless WebP encoding"): the argument
 * check, the bound, the residual picture with its modes, and a whole picture from host pixels to the file's bytes.  Plain C, no device;
 * every step is ffhip_vp8l_enc_body.h's, which the kernels compile too, run for lane 0 .. 63 in turn. */
#include "ffhip_vp8l_enc_internal.h"

#include <stdlib.h>
#include <string.h>

int ffhip_vp8lenc_source_ok(const ffhip_png_source *s, int flags)
{
    if (flags & ~(FFHIP_VP8L_ENC_SUBTRACT_GREEN | FFHIP_VP8L_ENC_PREDICT)) return 0;
    return ffhip_pngenc_source_ok(s, 0) && s->width <= 16384 && s->height <= 16384;
}

size_t ffhip_vp8l_encode_bound(int width, int height)
{
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return 0;
    return (size_t)ffhip_ve_bound((uint32_t)width, (uint32_t)height);
}

/* the residual picture, tile by tile; modes: a byte a tile, or NULL */
static void residual_picture(const ffhip_png_source *s, int flags, uint32_t *res, uint8_t *modes)
{
    const int w = s->width, h = s->height;
    const int tx = (int)ffhip_ve_sub_size((uint32_t)w), ty = (int)ffhip_ve_sub_size((uint32_t)h);
    for (int t = 0; t < tx * ty; t++) {
        const int x0 = (t % tx) << FFHIP_VP8L_ENC_TILE_BITS, y0 = (t / tx) << FFHIP_VP8L_ENC_TILE_BITS;
        const int x1 = x0 + FFHIP_VE_TILE < w ? x0 + FFHIP_VE_TILE : w, y1 = y0 + FFHIP_VE_TILE < h ? y0 + FFHIP_VE_TILE : h;
        int mode = 0;
        if (flags & FFHIP_VP8L_ENC_PREDICT) {
            uint32_t sums[14] = {0};
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) ffhip_ve_costs(s, flags, x, y, sums);
            mode = ffhip_ve_choose(sums);
            if (modes) modes[t] = (uint8_t)mode;
        }
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++) res[(size_t)y * (size_t)w + (size_t)x] = ffhip_ve_residual(s, flags, mode, x, y);
    }
}

int ffhip_vp8l_encode_residual(const ffhip_png_source *src, int flags, uint32_t *residual, uint8_t *modes)
{
    if (!ffhip_vp8lenc_source_ok(src, flags) || !residual || ((flags & FFHIP_VP8L_ENC_PREDICT) && !modes)) return FFHIP_EINVAL;
    residual_picture(src, flags, residual, modes);
    return FFHIP_OK;
}

typedef struct {
    ffhip_ve_parse_store parse;
    ffhip_ve_codes_store codes;
    uint32_t hist[FFHIP_VE_NSYM], table[FFHIP_VE_NSYM], lanes[FFHIP_DEF_LANES + 4];
} host_store;

int ffhip_vp8l_encode_picture(const ffhip_png_source *src, int flags, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_vp8lenc_source_ok(src, flags) || !len || (cap && !out)) return FFHIP_EINVAL;
    const uint32_t w = (uint32_t)src->width, h = (uint32_t)src->height;
    const uint64_t pixels = (uint64_t)w * h, n_chunks = ffhip_ve_chunks(pixels);
    const size_t tiles = (size_t)ffhip_ve_sub_size(w) * ffhip_ve_sub_size(h);
    const size_t n_words = (size_t)((ffhip_ve_bound(w, h) + 3) / 4 + 4);
    uint32_t *res = (uint32_t *)malloc((size_t)pixels * 4), *tok = (uint32_t *)malloc((size_t)pixels * 4);
    uint32_t *words = (uint32_t *)calloc(n_words, 4);
    uint8_t *modes = (uint8_t *)malloc(tiles);
    host_store *m = (host_store *)malloc(sizeof(*m));
    int rc = FFHIP_ENOMEM;
    if (res && tok && words && modes && m) {
        residual_picture(src, flags, res, modes);
        memset(m->hist, 0, sizeof(m->hist));
        for (uint64_t c = 0; c < n_chunks; c++) {
            const uint64_t at = c * FFHIP_VE_CHUNK, left = pixels - at;
            ffhip_ve_parse(&m->parse, res, at, (uint32_t)(left < FFHIP_VE_CHUNK ? left : FFHIP_VE_CHUNK), w, tok + at, m->hist);
        }
        uint64_t pos = ffhip_ve_codes(&m->codes, w, h, src->channels == 2 || src->channels == 4, flags, modes, m->hist, words, m->table);
        for (uint64_t c = 0; c < n_chunks; c++) {
            const uint64_t at = c * FFHIP_VE_CHUNK, left = pixels - at;
            const uint32_t n = (uint32_t)(left < FFHIP_VE_CHUNK ? left : FFHIP_VE_CHUNK);
            const uint32_t bits = ffhip_ve_count(m->lanes, m->table, res + at, tok + at, n, w);
            ffhip_ve_write(m->lanes, m->table, res + at, tok + at, n, w, words, pos);
            pos += bits;
        }
        const uint64_t size = ffhip_ve_finish(words, pos);
        const uint8_t *bytes = (const uint8_t *)words; /* the words are little-endian, as on the device */
        for (uint64_t k = 0; k < size && k < cap; k++) out[k] = bytes[k];
        *len = (size_t)size;
        rc = size > cap ? FFHIP_EVP8L_NOSPACE : FFHIP_OK;
    }
    free(res); free(tok); free(words); free(modes); free(m);
    return rc;
}
