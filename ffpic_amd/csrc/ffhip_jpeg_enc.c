/* ffhip_jpeg_enc.c -- the host side of the baseline JPEG encoder (include/ffpic_hip.h "JPEG encoding"): the quantiser
 * tables of a quality, one block, the header, the bound, and a whole picture from host pixels to the file's bytes.  Plain C, no device; the
 * sample rule, the DCT, the quantiser and the block code are ffhip_jpeg_enc_body.h's, which the kernels compile too.  The argument checks
 * and the tables here are also what the device calls use (ffhip_jpeg_enc_internal.h). */
#include "ffhip_jpeg_enc_internal.h"

#include <stdlib.h>
#include <string.h>

/* T.81 K.1, K.2: natural order */
static const uint8_t k_std_luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                       69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                       81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t k_std_chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
/* T.81 K.3 - K.6: code counts by length, symbols */
static const uint8_t k_dc_counts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t k_ac_counts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t k_ac_symbols[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

/* ---- checks shared with the device calls ---- */
int ffhip_jenc_params_ok(int width, int height, int layout, int restart)
{
    return width >= 1 && width <= 65535 && height >= 1 && height <= 65535 && je_layout_ok(layout) && restart >= 0 && restart <= 65535;
}

int ffhip_jenc_source_ok(const ffhip_jpeg_source *s, int layout)
{
    if (!s || !s->pixels || s->reserved != 0 || !je_layout_ok(layout)) return 0;
    if (s->width < 1 || s->width > 65535 || s->height < 1 || s->height > 65535) return 0;
    /* every byte offset of the picture within 2^46: the 64-bit address arithmetic cannot wrap */
    const int64_t lim = (int64_t)1 << 30;
    if (s->row_stride <= -lim || s->row_stride >= lim || s->pixel_stride <= -lim || s->pixel_stride >= lim) return 0;
    if (s->channels == 4) return layout != FFHIP_JPEG_ENC_GREY && s->pixel_stride == 4 && (s->row_stride & 3) == 0 && ((uintptr_t)s->pixels & 3) == 0;
    if (s->channels != (layout == FFHIP_JPEG_ENC_GREY ? 1 : 3)) return 0;
    for (int c = 0; c < s->channels; c++)
        if (s->chan[c] <= -lim || s->chan[c] >= lim) return 0;
    return 1;
}

void ffhip_jenc_geom(int width, int height, int layout, ffhip_jenc_geometry *g)
{
    g->h = je_layout_h(layout); g->v = je_layout_v(layout); g->ncomp = je_layout_ncomp(layout);
    g->mcu_cols = (width + 8 * g->h - 1) / (8 * g->h);
    g->mcu_rows = (height + 8 * g->v - 1) / (8 * g->v);
    g->mcus = (int64_t)g->mcu_cols * g->mcu_rows;
    g->bpm = je_mcu_blocks(layout);
    g->blocks = g->mcus * g->bpm;
}

/* ---- tables ---- */
int ffhip_jpeg_encode_tables(int quality, uint16_t *quant)
{
    if (!quant) return FFHIP_EINVAL;
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; k++) {
        const int l = (k_std_luma[k] * s + 50) / 100, c = (k_std_chroma[k] * s + 50) / 100;
        quant[k] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        quant[64 + k] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    return FFHIP_OK;
}

void ffhip_jenc_code_tables(uint32_t *tab /* [2][JE_TAB_WORDS] */)
{
    memset(tab, 0, 2 * JE_TAB_WORDS * sizeof(uint32_t));
    for (int set = 0; set < 2; set++) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) { /* T.81 C.2: canonical codes */
            for (int i = 0; i < k_ac_counts[set][len - 1]; i++) tab[set * JE_TAB_WORDS + k_ac_symbols[set][k++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < k_dc_counts[set][len - 1]; i++) tab[set * JE_TAB_WORDS + 256 + k++] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
}

int ffhip_jpeg_encode_block(const uint8_t *samples, const uint16_t *quant, int16_t *coef)
{
    if (!samples || !quant || !coef) return FFHIP_EINVAL;
    int32_t d[64];
    for (int k = 0; k < 64; k++) {
        if (quant[k] == 0) return FFHIP_EINVAL;
        d[k] = samples[k];
    }
    je_fdct_quant(d, quant);
    for (int k = 0; k < 64; k++) coef[k] = (int16_t)d[k];
    return FFHIP_OK;
}

/* ---- header ---- */
static uint8_t *seg(uint8_t *p, int marker, int payload)
{
    *p++ = 0xFF; *p++ = (uint8_t)marker; *p++ = (uint8_t)((payload + 2) >> 8); *p++ = (uint8_t)(payload + 2);
    return p;
}

size_t ffhip_jenc_header(int width, int height, int layout, int quality, int restart, uint8_t *out /* FFHIP_JPEG_ENC_HEADER_MAX */)
{
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    const int ncomp = je_layout_ncomp(layout), sets = ncomp == 3 ? 2 : 1;
    uint16_t quant[128];
    ffhip_jpeg_encode_tables(quality, quant);
    uint8_t *p = out;
    *p++ = 0xFF; *p++ = 0xD8;
    p = seg(p, 0xE0, 14);
    memcpy(p, jfif, 14); p += 14;
    for (int t = 0; t < sets; t++) {
        p = seg(p, 0xDB, 65);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; k++) *p++ = (uint8_t)quant[64 * t + je_zz[k]];
    }
    p = seg(p, 0xC0, 6 + 3 * ncomp);
    *p++ = 8; *p++ = (uint8_t)(height >> 8); *p++ = (uint8_t)height; *p++ = (uint8_t)(width >> 8); *p++ = (uint8_t)width; *p++ = (uint8_t)ncomp;
    for (int c = 0; c < ncomp; c++) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c == 0 ? (je_layout_h(layout) << 4) | je_layout_v(layout) : 0x11);
        *p++ = (uint8_t)(c ? 1 : 0);
    }
    for (int t = 0; t < sets; t++) {
        p = seg(p, 0xC4, 17 + 12);
        *p++ = (uint8_t)t;
        memcpy(p, k_dc_counts[t], 16); p += 16;
        for (int k = 0; k < 12; k++) *p++ = (uint8_t)k;
        p = seg(p, 0xC4, 17 + 162);
        *p++ = (uint8_t)(0x10 | t);
        memcpy(p, k_ac_counts[t], 16); p += 16;
        memcpy(p, k_ac_symbols[t], 162); p += 162;
    }
    if (restart) {
        p = seg(p, 0xDD, 2);
        *p++ = (uint8_t)(restart >> 8); *p++ = (uint8_t)restart;
    }
    p = seg(p, 0xDA, 4 + 2 * ncomp);
    *p++ = (uint8_t)ncomp;
    for (int c = 0; c < ncomp; c++) { *p++ = (uint8_t)(c + 1); *p++ = (uint8_t)(c ? 0x11 : 0x00); }
    *p++ = 0; *p++ = 63; *p++ = 0;
    return (size_t)(p - out);
}

int ffhip_jpeg_encode_header(int width, int height, int layout, int quality, int restart, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_jenc_params_ok(width, height, layout, restart) || !len || (cap && !out)) return FFHIP_EINVAL;
    uint8_t h[FFHIP_JPEG_ENC_HEADER_MAX];
    *len = ffhip_jenc_header(width, height, layout, quality, restart, h);
    if (*len > cap) return FFHIP_EJPEG_NOSPACE;
    memcpy(out, h, *len);
    return FFHIP_OK;
}

size_t ffhip_jpeg_encode_bound(int width, int height, int layout, int restart)
{
    if (!ffhip_jenc_params_ok(width, height, layout, restart)) return 0;
    ffhip_jenc_geometry g;
    ffhip_jenc_geom(width, height, layout, &g);
    uint8_t h[FFHIP_JPEG_ENC_HEADER_MAX];
    const size_t header = ffhip_jenc_header(width, height, layout, 50, restart, h);
    const uint64_t per = restart ? (uint64_t)restart : (uint64_t)g.mcus; /* MCUs of a full interval */
    const uint64_t full = (uint64_t)g.mcus / per, rest = (uint64_t)g.mcus % per;
    uint64_t b = full * (2 * ((per * g.bpm * JE_BLOCK_MAX_BITS + 7) / 8) + 2);
    if (rest) b += 2 * ((rest * g.bpm * JE_BLOCK_MAX_BITS + 7) / 8) + 2;
    return header + (size_t)b;
}

/* ---- a picture ---- */
/* steps 2 to 4 as samples: the padded planes, luma raster [8 v mcu_rows][8 h mcu_cols], chroma [8 mcu_rows][8 mcu_cols] */
static void planes_host(const ffhip_jpeg_source *s, const ffhip_jenc_geometry *g, uint8_t *py, uint8_t *pu, uint8_t *pv)
{
    const int W = s->width, H = s->height, h = g->h, v = g->v;
    const int64_t yw = 8LL * h * g->mcu_cols, cw = 8LL * g->mcu_cols;
    const int64_t c0 = s->channels == 4 ? 2 : s->chan[0], c1 = s->channels == 4 ? 1 : s->chan[1], c2 = s->channels == 4 ? 0 : s->chan[2];
    for (int64_t y = 0; y < 8LL * v * g->mcu_rows; y++)
        for (int64_t x = 0; x < yw; x++) {
            const uint8_t *p = s->pixels + je_luma_src_row((int)y, H) * s->row_stride + je_src_col((int)x, W) * s->pixel_stride;
            int yy = p[c0], cb, cr;
            if (g->ncomp == 3) je_ycc(p[c0], p[c1], p[c2], &yy, &cb, &cr);
            py[y * yw + x] = (uint8_t)yy;
        }
    if (g->ncomp != 3) return;
    for (int64_t cy = 0; cy < 8LL * g->mcu_rows; cy++)
        for (int64_t cx = 0; cx < cw; cx++) {
            int cb[2][2] = {{0, 0}, {0, 0}}, cr[2][2] = {{0, 0}, {0, 0}}, yy;
            for (int dy = 0; dy < v; dy++)
                for (int dx = 0; dx < h; dx++) {
                    const uint8_t *p = s->pixels + je_chroma_src_row((int)cy, dy, H, v) * s->row_stride + je_src_col((int)cx * h + dx, W) * s->pixel_stride;
                    je_ycc(p[c0], p[c1], p[c2], &yy, &cb[dy][dx], &cr[dy][dx]);
                }
            int u = cb[0][0], w = cr[0][0];
            if (h == 2 && v == 2) { u = je_h2v2(cb[0][0], cb[0][1], cb[1][0], cb[1][1], (int)cx); w = je_h2v2(cr[0][0], cr[0][1], cr[1][0], cr[1][1], (int)cx); }
            else if (h == 2) { u = je_h2v1(cb[0][0], cb[0][1], (int)cx); w = je_h2v1(cr[0][0], cr[0][1], (int)cx); }
            pu[cy * cw + cx] = (uint8_t)u;
            pv[cy * cw + cx] = (uint8_t)w;
        }
}

static void block_host(const uint8_t *plane, int64_t stride, int64_t bx, int64_t by, const uint16_t *quant, int16_t *coef)
{
    int32_t d[64];
    for (int k = 0; k < 64; k++) d[k] = plane[(by * 8 + (k >> 3)) * stride + bx * 8 + (k & 7)];
    je_fdct_quant(d, quant);
    for (int k = 0; k < 64; k++) coef[k] = (int16_t)d[k];
}

int ffhip_jpeg_encode_picture(const ffhip_jpeg_source *src, int layout, int quality, int restart, uint8_t *out, size_t cap, size_t *len)
{
    if (!ffhip_jenc_source_ok(src, layout) || !ffhip_jenc_params_ok(src->width, src->height, layout, restart) || !len || (cap && !out)) return FFHIP_EINVAL;
    ffhip_jenc_geometry g;
    ffhip_jenc_geom(src->width, src->height, layout, &g);
    const int hv = g.h * g.v;
    const int64_t yw = 8LL * g.h * g.mcu_cols, cw = 8LL * g.mcu_cols;
    const size_t ysz = (size_t)(yw * 8 * g.v * g.mcu_rows), csz = g.ncomp == 3 ? (size_t)(cw * 8 * g.mcu_rows) : 0;
    uint16_t quant[128];
    uint32_t tab[2 * JE_TAB_WORDS];
    ffhip_jpeg_encode_tables(quality, quant);
    ffhip_jenc_code_tables(tab);
    int rc = FFHIP_ENOMEM;
    uint8_t *planes = (uint8_t *)malloc(ysz + 2 * csz);
    int16_t *coef = (int16_t *)malloc((size_t)g.blocks * 64 * sizeof(int16_t));
    uint64_t *start = (uint64_t *)malloc((size_t)g.blocks * sizeof(uint64_t));
    uint32_t *words = NULL, *mask = NULL;
    if (!planes || !coef || !start) goto done;
    planes_host(src, &g, planes, planes + ysz, planes + ysz + csz);
    int16_t *cy = coef, *cu = coef + g.mcus * hv * 64, *cv = cu + g.mcus * 64;
    for (int64_t my = 0; my < g.mcu_rows; my++)
        for (int64_t mx = 0; mx < g.mcu_cols; mx++) {
            const int64_t mcu = my * g.mcu_cols + mx;
            for (int j = 0; j < hv; j++) {
                const int sj = je_dc_source(j, (int)mx, (int)my, g.h, g.v, src->width, src->height);
                int16_t *blk = cy + (mcu * hv + j) * 64;
                block_host(planes, yw, mx * g.h + sj % g.h, my * g.v + sj / g.h, quant, blk);
                if (sj != j) memset(blk + 1, 0, 63 * sizeof(int16_t));
            }
            if (g.ncomp == 3) {
                block_host(planes + ysz, cw, mx, my, quant + 64, cu + mcu * 64);
                block_host(planes + ysz + csz, cw, mx, my, quant + 64, cv + mcu * 64);
            }
        }
    /* positions, block after block */
    int bad = 0;
    uint64_t pos = 0;
    for (int64_t b = 0; b < g.blocks; b++) {
        const int64_t mcu = b / g.bpm;
        const int j = (int)(b % g.bpm);
        const int starts = j == 0 && mcu > 0 && restart && mcu % restart == 0;
        const int bits = je_block_code(je_scan_block(cy, cu, cv, hv, mcu, j), je_scan_pred(cy, cu, cv, hv, mcu, j, restart), tab + (j >= hv && g.ncomp == 3 ? JE_TAB_WORDS : 0), NULL, &bad);
        if (starts) pos = je_up8(pos) + 16;
        start[b] = pos;
        pos += (uint64_t)bits;
    }
    const uint64_t stream = (je_up8(pos) >> 3) + 2; /* bytes, EOI included */
    words = (uint32_t *)calloc((size_t)(stream / 4 + 2), 4);
    mask = (uint32_t *)calloc((size_t)(stream / 32 + 2), 4);
    if (!words || !mask) goto done;
    for (int64_t b = 0; b < g.blocks; b++) {
        const int64_t mcu = b / g.bpm;
        const int j = (int)(b % g.bpm);
        je_sink s;
        je_sink_open(&s, words, start[b]);
        const int bits = je_block_code(je_scan_block(cy, cu, cv, hv, mcu, j), je_scan_pred(cy, cu, cv, hv, mcu, j, restart), tab + (j >= hv && g.ncomp == 3 ? JE_TAB_WORDS : 0), &s, &bad);
        if (j == g.bpm - 1 && (mcu == g.mcus - 1 || (restart && (mcu + 1) % restart == 0)))
            je_interval_end(&s, start[b] + (uint64_t)bits, mcu == g.mcus - 1 ? 0xD9 : 0xD0 + (int)(((mcu + 1) / restart - 1) & 7), mask);
        je_sink_close(&s);
    }
    {
        uint8_t head[FFHIP_JPEG_ENC_HEADER_MAX];
        const size_t hl = ffhip_jenc_header(src->width, src->height, layout, quality, restart, head);
        const uint8_t *bytes = (const uint8_t *)words;
        size_t o = hl;
        if (hl <= cap) memcpy(out, head, hl);
        else if (cap) memcpy(out, head, cap);
        for (uint64_t i = 0; i < stream; i++) {
            if (o < cap) out[o] = bytes[i];
            o++;
            if (bytes[i] == 0xFF && !((mask[i >> 5] >> (i & 31)) & 1)) {
                if (o < cap) out[o] = 0;
                o++;
            }
        }
        *len = o;
        rc = bad ? FFHIP_EJPEG_RANGE : (o > cap ? FFHIP_EJPEG_NOSPACE : FFHIP_OK);
    }
done:
    free(planes); free(coef); free(start); free(words); free(mask);
    return rc;
}
