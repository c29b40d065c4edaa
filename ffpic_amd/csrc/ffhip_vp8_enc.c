/* ffhip_vp8_enc.c -- the host side of the lossy WebP encoder (include/ffpic_hip.h "Lossy WebP encoding"): the argument
 * checks, the quantiser index and steps, the bound, the colour step, the macroblock step and a whole picture from host pixels to the file's
 * bytes.  Plain C, no device; every step is ffhip_vp8_enc_body.h's, which the kernels compile too. */
#include "ffhip_vp8_enc_internal.h"
#include "ffhip_jpeg_enc_internal.h" /* ffhip_jenc_source_ok: the source record is the JPEG encoder's */
#include "ffhip_vp8_quant.h"

#include <stdlib.h>
#include <string.h>

/* libwebp's 127 (1 - cbrt(l)) of a quality, evaluated once */
static const uint8_t quality_qi[101] = {
    127, 103, 96, 92, 89, 86, 83, 81, 79, 77, 75, 73, 72, 70, 69, 68, 66, 65, 64, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 51, 50,
    49,  48,  48, 47, 46, 45, 45, 44, 43, 43, 42, 41, 41, 40, 40, 39, 38, 38, 37, 37, 36, 36, 35, 35, 34, 33, 33, 32, 32, 31, 31, 30, 30, 29,
    29,  28,  28, 28, 27, 27, 26, 26, 24, 23, 22, 21, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9,  8,  7,  6,  5,  4,  3,  2,  1,  0,  0};
static const uint16_t dc_q[128] = FFB_DC_Q;
static const uint16_t ac_q[128] = FFB_AC_Q;

int ffhip_vp8enc_source_ok(const ffhip_jpeg_source *s)
{
    if (!s || (s->channels != 1 && s->channels != 3)) return 0;
    return ffhip_jenc_source_ok(s, s->channels == 1 ? FFHIP_JPEG_ENC_GREY : FFHIP_JPEG_ENC_444) && s->width <= V8E_MAX_SIDE && s->height <= V8E_MAX_SIDE;
}

int ffhip_vp8enc_params_ok(int quality, int filter) { return quality >= 0 && quality <= 100 && filter >= -1 && filter <= 63; }

void ffhip_vp8enc_steps(int qi, uint16_t *q)
{
    q[0] = dc_q[qi];
    q[1] = ac_q[qi];
    q[2] = (uint16_t)(2 * dc_q[qi]);
    q[3] = (uint16_t)(ac_q[qi] * 155 / 100 < 8 ? 8 : ac_q[qi] * 155 / 100);
    q[4] = dc_q[qi] > 132 ? 132 : dc_q[qi];
    q[5] = ac_q[qi];
}

int ffhip_vp8_encode_quality_index(int quality) { return quality < 0 || quality > 100 ? FFHIP_EINVAL : quality_qi[quality]; }

size_t ffhip_vp8_encode_bound(int width, int height)
{
    if (width < 1 || width > V8E_MAX_SIDE || height < 1 || height > V8E_MAX_SIDE) return 0;
    const int cols = v8e_mb_cols(width), rows = v8e_mb_cols(height), parts = 1 << v8e_log2_parts(rows);
    uint64_t n = 30 + v8e_p0_bound((uint64_t)cols * rows) + 3 * (uint64_t)(parts - 1) + 1;
    for (int k = 0; k < parts; k++) n += v8e_part_bound((uint64_t)cols * v8e_part_rows(rows, parts, k));
    return (size_t)n;
}

static void planes_of(const ffhip_jpeg_source *s, uint8_t *y, uint8_t *u, uint8_t *v)
{
    const int cols = v8e_mb_cols(s->width), rows = v8e_mb_cols(s->height);
    for (int py = 0; py < 16 * rows; py++)
        for (int px = 0; px < 16 * cols; px++) y[(size_t)py * 16 * cols + px] = (uint8_t)v8e_luma(s, px, py);
    for (int cy = 0; cy < 8 * rows; cy++)
        for (int cx = 0; cx < 8 * cols; cx++) {
            int cu, cv;
            v8e_chroma(s, cx, cy, &cu, &cv);
            u[(size_t)cy * 8 * cols + cx] = (uint8_t)cu;
            v[(size_t)cy * 8 * cols + cx] = (uint8_t)cv;
        }
}

int ffhip_vp8_encode_planes(const ffhip_jpeg_source *src, uint8_t *y, uint8_t *u, uint8_t *v)
{
    if (!ffhip_vp8enc_source_ok(src) || !y || !u || !v) return FFHIP_EINVAL;
    planes_of(src, y, u, v);
    return FFHIP_OK;
}

/* everything a picture's macroblock step reads and writes, in one allocation */
typedef struct {
    v8e_pic pic;
    uint8_t *mem;
} host_pic;

static int host_pic_make(host_pic *h, const ffhip_jpeg_source *s, int quality)
{
    const int cols = v8e_mb_cols(s->width), rows = v8e_mb_cols(s->height);
    const size_t n_mb = (size_t)cols * rows, luma = n_mb * 256, chroma = n_mb * 64;
    h->mem = (uint8_t *)malloc(n_mb * 800 + n_mb * 4 + 2 * (luma + 2 * chroma) + 2 * n_mb);
    if (!h->mem) return FFHIP_ENOMEM;
    uint8_t *at = h->mem;
    v8e_pic *p = &h->pic;
    memset(p, 0, sizeof(*p));
    p->levels = (int16_t *)at; at += n_mb * 800;
    p->mask = (uint32_t *)at; at += n_mb * 4;
    uint8_t *sy = at, *su = sy + luma, *sv = su + chroma;
    p->sy = sy; p->su = su; p->sv = sv;
    p->ry = sv + chroma; p->ru = p->ry + luma; p->rv = p->ru + chroma;
    p->ymode = p->rv + chroma; p->uvmode = p->ymode + n_mb;
    p->cols = cols; p->rows = rows;
    ffhip_vp8enc_steps(quality_qi[quality], p->q);
    planes_of(s, sy, su, sv);
    v8e_mb_store m;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) v8e_mb(p, &m, x, y, 0, 1);
    return FFHIP_OK;
}

int ffhip_vp8_encode_mbs(const ffhip_jpeg_source *src, int quality, uint8_t *ymode, uint8_t *uvmode, int16_t *levels, uint8_t *recon_y, uint8_t *recon_u,
                         uint8_t *recon_v)
{
    if (!ffhip_vp8enc_source_ok(src) || !ffhip_vp8enc_params_ok(quality, 0) || !ymode || !uvmode || !levels || !recon_y || !recon_u || !recon_v)
        return FFHIP_EINVAL;
    host_pic h;
    const int rc = host_pic_make(&h, src, quality);
    if (rc) return rc;
    const size_t n_mb = (size_t)h.pic.cols * h.pic.rows;
    memcpy(ymode, h.pic.ymode, n_mb);
    memcpy(uvmode, h.pic.uvmode, n_mb);
    memcpy(levels, h.pic.levels, n_mb * 800);
    memcpy(recon_y, h.pic.ry, n_mb * 256);
    memcpy(recon_u, h.pic.ru, n_mb * 64);
    memcpy(recon_v, h.pic.rv, n_mb * 64);
    free(h.mem);
    return FFHIP_OK;
}

int ffhip_vp8_encode_picture(const ffhip_jpeg_source *src, int quality, int filter, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_vp8enc_source_ok(src) || !ffhip_vp8enc_params_ok(quality, filter) || !len || (cap && !out)) return FFHIP_EINVAL;
    host_pic h;
    int rc = host_pic_make(&h, src, quality);
    if (rc) return rc;
    const v8e_pic *p = &h.pic;
    const int qi = quality_qi[quality], parts = 1 << v8e_log2_parts(p->rows);
    uint8_t *base = (uint8_t *)malloc((size_t)v8e_part_at(parts, p->cols, p->rows, parts));
    if (!base) {
        free(h.mem);
        return FFHIP_ENOMEM;
    }
    v8e_file f;
    memset(&f, 0, sizeof(f));
    f.parts = parts;
    f.p0 = (uint32_t)v8e_first_partition(p, qi, filter < 0 ? v8e_auto_filter(qi) : filter, base);
    for (int k = 0; k < parts; k++) f.part[k] = (uint32_t)v8e_token_partition(p, k, parts, base + v8e_part_at(k, p->cols, p->rows, parts));
    v8e_file_plan(&f, src->width, src->height);
    rc = f.status;
    *len = 0;
    if (rc == FFHIP_OK) {
        *len = (size_t)f.file_len;
        if (f.file_len > cap) rc = FFHIP_EVP8_NOSPACE;
        v8e_file_copy(&f, base, p->cols, p->rows, out, 0, f.file_len < cap ? f.file_len : cap, 0, 1);
    }
    free(base);
    free(h.mem);
    return rc;
}
