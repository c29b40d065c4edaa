/* ffhip_jpeg_front.c -- where a JPEG header is read (ffhip_jpeg_front.h; DESIGN.md 4.32 has what the callers decide differently).  Plain C11, no
 * HIP.  Stands where the marker loop and the segment readers of the reference stand: format/jpg.c:78-105, 640-655, 771-855. */
#include "ffhip_jpeg_front.h"

#include <string.h>

static const uint8_t k_zigzag[64] = FFHIP_JPEG_ZIGZAG;

int ffhip_jpeg_huff_build(struct huff *h, const uint8_t counts[16], const uint8_t *vals, int nvals)
{
    memset(h, 0, sizeof *h);
    int code = 0, k = 0;
    memcpy(h->vals, vals, (size_t)nvals);
    for (int len = 1; len <= 16; len++) {
        h->valptr[len] = k;
        h->mincode[len] = code;
        for (int i = 0; i < counts[len - 1]; i++, k++, code++) {
            if (k >= nvals) return -1;
            if (code >= (1 << len)) return -1; /* over-subscribed DHT (Kraft sum > 1): the code does not fit its length */
            if (len <= LOOK) {
                const int first = code << (LOOK - len), n = 1 << (LOOK - len);
                for (int j = 0; j < n; j++) h->look[first + j] = (uint16_t)((len << 8) | vals[k]);
            }
        }
        h->maxcode[len] = counts[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    h->present = 1;
    return 0;
}

void ffhip_jpeg_huff_fast(struct huff *h)
{
    for (int i = 0; i < (1 << LOOK); i++) {
        const unsigned e = h->look[i];
        const int len = (int)(e >> 8), run = (int)((e >> 4) & 15), mag = (int)(e & 15);
        if (!e || !mag || len + mag > LOOK) continue;
        int k = ((i << len) & ((1 << LOOK) - 1)) >> (LOOK - mag);
        if (k < (1 << (mag - 1))) k -= (1 << mag) - 1; /* EXTEND of T.81 F.2.2.1 */
        if (k >= -128 && k <= 127) h->fast[i] = (int16_t)((k * 256) + (run * 16) + len + mag);
    }
}

int ffhip_jpeg_walk_open(struct jpeg_walk *w, const uint8_t *f, size_t len)
{
    *w = (struct jpeg_walk){f, NULL, len, 2, 0, 0};
    return len < 4 || f[0] != 0xFF || f[1] != 0xD8 ? -1 : 0;
}

enum jpeg_event ffhip_jpeg_walk_next(struct jpeg_walk *w)
{
    const uint8_t *f = w->f;
    const size_t len = w->len;
    size_t p = w->p;
    if (p + 2 > len) return JPEG_END;
    if (f[p] != 0xFF) return JPEG_MALFORMED;
    while (p < len && f[p] == 0xFF) p++; /* fill bytes */
    if (p >= len) return JPEG_MALFORMED;
    w->marker = f[p++];
    w->p = p;
    if (w->marker == 0xD9) return JPEG_EOI;
    if (w->marker == 0x01 || (w->marker >= 0xD0 && w->marker <= 0xD7)) return JPEG_STANDALONE;
    if (p + 2 > len) return JPEG_MALFORMED;
    const size_t L = ((size_t)f[p] << 8) | f[p + 1]; /* counts its own two bytes */
    if (L < 2 || p + L > len) return JPEG_MALFORMED;
    w->seg = f + p + 2;
    w->seg_len = L - 2;
    w->p = p + L;
    return JPEG_SEGMENT;
}

int ffhip_jpeg_read_dqt(const uint8_t *s, size_t sl, uint16_t quant[4][64], int max_prec) /* stored de-zigzagged like read_dqt (jpg.c:78-105) */
{
    size_t i = 0;
    while (i < sl) {
        const int prec = s[i] >> 4, id = s[i] & 15;
        i++;
        if (prec > max_prec || id > 3 || i + (size_t)64 * (prec + 1) > sl) return -1;
        for (int k = 0; k < 64; k++, i += prec + 1) quant[id][k_zigzag[k]] = prec ? (uint16_t)((s[i] << 8) | s[i + 1]) : s[i];
    }
    return 0;
}

int ffhip_jpeg_read_dht(const uint8_t *s, size_t sl, struct huff dc[4], struct huff ac[4], int fast, unsigned *defined)
{
    size_t i = 0;
    while (i + 17 <= sl) {
        const int tc = s[i] >> 4, th = s[i] & 15;
        int n = 0;
        for (int k = 0; k < 16; k++) n += s[i + 1 + k];
        if (tc > 1 || th > 3 || n > 256 || i + 17 + (size_t)n > sl) return -1;
        struct huff *h = tc ? &ac[th] : &dc[th];
        if (ffhip_jpeg_huff_build(h, s + i + 1, s + i + 17, n)) return -1;
        if (fast) ffhip_jpeg_huff_fast(h);
        if (defined) *defined |= 1u << (tc * 4 + th);
        i += 17 + (size_t)n;
    }
    return 0;
}

int ffhip_jpeg_read_sof(const uint8_t *s, size_t sl, struct jpeg_frame *fr)
{
    if (sl < 6 || s[0] != 8) return -1;
    fr->height = (s[1] << 8) | s[2];
    fr->width = (s[3] << 8) | s[4];
    fr->ncomp = s[5];
    if ((fr->ncomp != 1 && fr->ncomp != 3) || sl < (size_t)(6 + 3 * fr->ncomp)) return -1;
    if (fr->width == 0 || fr->height == 0) return -1; /* height 0 = "see DNL": not this path */
    for (int c = 0; c < fr->ncomp; c++) {
        fr->cid[c] = s[6 + 3 * c];
        fr->h[c] = s[7 + 3 * c] >> 4;
        fr->v[c] = s[7 + 3 * c] & 15;
        fr->tq[c] = s[8 + 3 * c];
        if (fr->tq[c] > 3) return -1;
    }
    return 0;
}

int ffhip_jpeg_read_dri(const uint8_t *s, size_t sl, int *restart)
{
    if (sl >= 2) *restart = (s[0] << 8) | s[1];
    return sl >= 2 ? 0 : -1;
}

int ffhip_jpeg_frame_layout(struct jpeg_frame *fr)
{
    if (fr->ncomp == 1) fr->h[0] = fr->v[0] = 1; /* single-component scans are never interleaved */
    if (fr->h[0] < 1 || fr->v[0] < 1 || fr->h[0] * fr->v[0] > 4) return -1; /* jpg.c:501: Y[3][64*4] */
    for (int c = 1; c < fr->ncomp; c++)
        if (fr->h[c] != 1 || fr->v[c] != 1) return -1; /* colorspace.c:149-150: chroma is one block per MCU */
    return 0;
}

void ffhip_jpeg_frame_geom(const struct jpeg_frame *fr, ffhip_jpeg_geom *geom)
{
    geom->ncomp = fr->ncomp;
    geom->h = fr->h[0]; geom->v = fr->v[0];
    geom->mcu_cols = (fr->width + 8 * fr->h[0] - 1) / (8 * fr->h[0]);
    geom->mcu_rows = (fr->height + 8 * fr->v[0] - 1) / (8 * fr->v[0]);
    for (int c = 0; c < 3; c++) geom->qt_id[c] = c < fr->ncomp ? fr->tq[c] : 0;
}
