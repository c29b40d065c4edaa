/* ffhip_png_enc.c -- the host side of the PNG encoder (include/ffpic_hip.h "PNG encoding"): the argument check, the filtered
 * picture, the bound, and a whole picture from host pixels to the file's bytes.  Plain C, no device; the filters, the row's choice and the
 * file's pieces are ffhip_png_enc_body.h's and the stream is ffhip_deflate_body.h's, which the kernels compile too. */
#include "ffhip_png_enc_internal.h"

#include <stdlib.h>
#include <string.h>

int ffhip_pngenc_source_ok(const ffhip_png_source *s, int filter)
{
    if (!s || !s->pixels || s->reserved != 0 || filter < 0 || filter > FFHIP_PNG_FILTER_ADAPTIVE) return 0;
    if (s->width < 1 || s->width > 65535 || s->height < 1 || s->height > 65535 || s->channels < 1 || s->channels > 4) return 0;
    const int64_t lim = (int64_t)1 << 30; /* every byte offset of the picture within 2^47: the 64-bit address arithmetic cannot wrap */
    if (s->row_stride <= -lim || s->row_stride >= lim || s->pixel_stride <= -lim || s->pixel_stride >= lim) return 0;
    for (int c = 0; c < s->channels; c++)
        if (s->chan[c] <= -lim || s->chan[c] >= lim) return 0;
    return 1;
}

void ffhip_pngenc_header(int width, int height, int channels, uint8_t out[FFHIP_PE_HEADER])
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    static const uint8_t type[5] = {0, 0, 4, 2, 6};
    memcpy(out, sig, 8);
    ffhip_pe_be32(out + 8, 13);
    memcpy(out + 12, "IHDR", 4);
    ffhip_pe_be32(out + 16, (uint32_t)width);
    ffhip_pe_be32(out + 20, (uint32_t)height);
    out[24] = 8; out[25] = type[channels]; out[26] = 0; out[27] = 0; out[28] = 0;
    ffhip_pe_be32(out + 29, ffhip_def_crc_bytes(0, out + 12, 17));
}

size_t ffhip_png_filtered_size(int width, int height, int channels)
{
    if (width < 1 || width > 65535 || height < 1 || height > 65535 || channels < 1 || channels > 4) return 0;
    return (size_t)ffhip_pe_filtered_len(width, height, channels);
}

size_t ffhip_png_encode_bound(int width, int height, int channels)
{
    const size_t flen = ffhip_png_filtered_size(width, height, channels);
    if (!flen) return 0;
    return FFHIP_PE_HEADER + 12 * (size_t)ffhip_def_chunks(flen) + ffhip_deflate_bound(flen) + 12 + 12;
}

static void filter_rows(const ffhip_png_source *s, int filter, uint8_t *out)
{
    const int64_t rb = (int64_t)s->width * s->channels;
    for (int row = 0; row < s->height; row++) {
        uint8_t *dst = out + (int64_t)row * (rb + 1);
        int type = filter, f[5];
        if (filter == FFHIP_PNG_FILTER_ADAPTIVE) {
            uint32_t sums[5] = {0, 0, 0, 0, 0};
            for (int64_t j = 0; j < rb; j++) {
                ffhip_pe_filter5(s, row, j, f);
                for (int t = 0; t < 5; t++) sums[t] += ffhip_pe_cost(f[t]);
            }
            type = ffhip_pe_choose(sums);
        }
        dst[0] = (uint8_t)type;
        for (int64_t j = 0; j < rb; j++) {
            ffhip_pe_filter5(s, row, j, f);
            dst[1 + j] = (uint8_t)ffhip_pe_pick(f, type);
        }
    }
}

int ffhip_png_filter_picture(const ffhip_png_source *src, int filter, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_pngenc_source_ok(src, filter) || !out || !len) return FFHIP_EINVAL;
    *len = ffhip_png_filtered_size(src->width, src->height, src->channels);
    if (*len > cap) return FFHIP_EPNG_NOSPACE;
    filter_rows(src, filter, out);
    return FFHIP_OK;
}

int ffhip_png_encode_picture(const ffhip_png_source *src, int filter, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_pngenc_source_ok(src, filter) || !len || (cap && !out)) return FFHIP_EINVAL;
    const size_t flen = ffhip_png_filtered_size(src->width, src->height, src->channels);
    uint8_t *filt = (uint8_t *)malloc(flen), *chunks = NULL;
    ffhip_def_result *res = NULL;
    uint64_t n_chunks = 0;
    if (!filt) return FFHIP_ENOMEM;
    filter_rows(src, filter, filt);
    const int rc = ffhip_deflate_chunks_host(filt, flen, &chunks, &res, &n_chunks);
    if (rc) {
        free(filt);
        return rc;
    }
    size_t o = 0;
#define PUT(p, n) do { for (size_t k__ = 0; k__ < (size_t)(n); k__++, o++) if (o < cap) out[o] = (p)[k__]; } while (0)
    uint8_t head[FFHIP_PE_HEADER], tail[FFHIP_PE_TAIL], crc_be[4];
    ffhip_pngenc_header(src->width, src->height, src->channels, head);
    PUT(head, FFHIP_PE_HEADER);
    uint32_t a = 1, b = 0;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const uint64_t left = flen - c * FFHIP_DEF_CHUNK;
        uint8_t ih[10];
        const int n = ffhip_pe_idat_head_len(c == 0);
        for (int k = 0; k < n; k++) ih[k] = ffhip_pe_idat_head_byte(c == 0, res[c].out_len, k);
        const uint32_t crc = ffhip_pe_idat_crc(c == 0, res[c].out_len, res[c].crc);
        PUT(ih, n);
        PUT(chunks + c * FFHIP_DEF_OUT_BYTES, res[c].out_len);
        ffhip_pe_be32(crc_be, crc);
        PUT(crc_be, 4);
        ffhip_def_adler_join(&a, &b, res[c].adler_a, res[c].adler_b, left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK);
    }
    ffhip_pe_tail(a, b, tail);
    PUT(tail, FFHIP_PE_TAIL);
#undef PUT
    free(filt); free(chunks); free(res);
    *len = o;
    return o > cap ? FFHIP_EPNG_NOSPACE : FFHIP_OK;
}
