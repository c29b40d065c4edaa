/*
 * ffhip_jpeg_progressive.c -- host side of the progressive JPEG front end: the marker loop with its scan list, the staging of a scan's bytes,
 * and the reference decoder.  Plain C11, no HIP.
 *
 * Written from ITU-T T.81 Annex G, not from the reference's progressive branches (format/jpg.c:255-415, 512-576 walk non-interleaved scans
 * over the MCU grid and dequantise by the last scan's Se): a progressive file and a baseline file of the same quantised coefficients decode
 * to the same planes, and everything behind the planes is the existing reconstruction, so what the tests hold this decoder against is the baseline twin.
 *
 * Accepted: SOF2, 8-bit, Huffman, 1 or 3 components in the layouts of the baseline parser (h x v <= 4 for the first component, chroma 1 x 1,
 * a single component always 1 x 1); DC scans interleaved or not, AC scans of one component; DHT and DRI redefined between scans -- every scan
 * carries its own snapshot of the tables it uses (the same table id means a different table from scan to scan in optimised files).
 * Everything else is FFHIP_EINVAL at parse time, before anything is decoded (ffhip_prog_parse).  An incomplete progression that ends in
 * EOI is valid: bands never sent stay zero, bits never refined stay as they are.
 *
 * The per-block steps and the walk over a restart interval are ffhip_jpeg_prog_body.h, shared with the kernel.
 */
#include "ffpic_hip.h"
#include "ffhip_jpeg_prog_body.h"
#include "ffhip_jpeg_prog_internal.h"

#include <stdlib.h>
#include <string.h>

void ffhip_prog_free(struct prog_file *pf)
{
    free(pf->tabs);
    pf->tabs = NULL;
    pf->n_tabs = 0;
}

/* the current table `slot` (0..3 DC, 4..7 AC) as an index into pf->tabs: snapshotted at its first use behind its definition */
static int prog_snapshot(struct prog_file *pf, const struct huff *cur, int *snap, int slot)
{
    if (!cur[slot].present) return -1;
    if (snap[slot] >= 0) return snap[slot];
    if (pf->n_tabs == pf->cap_tabs) {
        const int cap = pf->cap_tabs ? 2 * pf->cap_tabs : 16;
        struct huff *t = realloc(pf->tabs, (size_t)cap * sizeof *t);
        if (!t) return -2;
        pf->tabs = t;
        pf->cap_tabs = cap;
    }
    pf->tabs[pf->n_tabs] = cur[slot];
    return snap[slot] = pf->n_tabs++;
}

/* the progressive parser: the marker walk over the whole file, every scan cut at the first marker that is no RSTn.  Its choices against ffhip_jpeg_parse's: DESIGN.md 4.32 */
int ffhip_prog_parse(const uint8_t *f, size_t len, struct prog_file *pf)
{
    memset(pf, 0, sizeof *pf);
    for (int t = 0; t < 4; t++)
        for (int i = 0; i < 64; i++) pf->fr.quant[t][i] = 1;
    struct jpeg_walk w;
    if (!f || ffhip_jpeg_walk_open(&w, f, len)) return FFHIP_EINVAL;
    struct huff *cur = calloc(8, sizeof *cur); /* the tables as the marker loop has them now */
    if (!cur) return FFHIP_ENOMEM;
    int snap[8], rc = FFHIP_EINVAL, have_sof = 0, restart = 0;
    int8_t last_al[3][64]; /* per component and coefficient: the Al of its latest scan, -1 = none yet */
    memset(last_al, -1, sizeof last_al);
    for (int i = 0; i < 8; i++) snap[i] = -1;
    for (;;) {
        const enum jpeg_event ev = ffhip_jpeg_walk_next(&w);
        if (ev == JPEG_EOI) break; /* ends the file, wherever it stands */
        if (ev == JPEG_STANDALONE) continue;
        if (ev != JPEG_SEGMENT) goto out; /* malformed, or the file ends without EOI */
        const int m = w.marker;
        const uint8_t *s = w.seg;
        const size_t sl = w.seg_len;
        if (m == 0xDB) {
            if (pf->n_scans) goto out; /* a DQT behind the first SOS: the planes would need two quantisers */
            if (ffhip_jpeg_read_dqt(s, sl, pf->fr.quant, 1)) goto out; /* 8 and 16 bit entries only */
        } else if (m == 0xC4) {
            unsigned built = 0;
            if (ffhip_jpeg_read_dht(s, sl, cur, cur + 4, 0, &built)) goto out; /* without the one-look-up path: never read here, fast[] stays zero */
            for (int t = 0; t < 8; t++)
                if (built >> t & 1) snap[t] = -1;
        } else if (m == 0xC2) { /* SOF2, once, the layout rule at once */
            if (have_sof || ffhip_jpeg_read_sof(s, sl, &pf->fr) || ffhip_jpeg_frame_layout(&pf->fr)) goto out;
            have_sof = 1;
        } else if (m >= 0xC0 && m <= 0xCF) {
            goto out; /* another frame type (baseline, lossless, arithmetic), DAC, JPG: not this path */
        } else if (m == 0xDD) {
            if (ffhip_jpeg_read_dri(s, sl, &restart)) goto out;
        } else if (m == 0xDA) {
            if (!have_sof || sl < 1 || pf->n_scans == FFHIP_JPEG_MAX_SCANS) goto out;
            const int ns = s[0];
            const struct jpeg_frame *fr = &pf->fr;
            if (ns < 1 || ns > fr->ncomp || sl < (size_t)(4 + 2 * ns)) goto out;
            struct prog_scan *sc = &pf->scan[pf->n_scans];
            memset(sc, 0, sizeof *sc);
            const uint8_t *t = s + 1 + 2 * ns;
            const int ss = t[0], se = t[1], ah = t[2] >> 4, al = t[2] & 15;
            if (se > 63 || se < ss || (ss == 0 && se != 0) || (ss > 0 && ns != 1) || al > 13 || ah > 13) goto out;
            sc->ncomp = (uint32_t)ns; sc->ss = (uint32_t)ss; sc->se = (uint32_t)se; sc->ah = (uint32_t)ah; sc->al = (uint32_t)al;
            for (int k = 0; k < ns; k++) {
                int c;
                for (c = 0; c < fr->ncomp && fr->cid[c] != s[1 + 2 * k]; c++) {}
                if (c == fr->ncomp) goto out;
                for (int q = 0; q < k; q++)
                    if (sc->comp[q] == (uint32_t)c) goto out;
                if (k && (uint32_t)c < sc->comp[k - 1]) goto out; /* B.2.3: in the frame's order */
                sc->comp[k] = (uint32_t)c;
                const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
                if (td > 3 || ta > 3) goto out;
                /* G.1.1.1.1: a first scan of every coefficient it carries, or the refinement of the previous pass by one bit */
                if (ss > 0 && last_al[c][0] < 0) goto out; /* AC before the component's DC */
                for (int i = ss; i <= se; i++) {
                    if (ah == 0 ? last_al[c][i] >= 0 : (last_al[c][i] != ah || al != ah - 1)) goto out;
                    last_al[c][i] = (int8_t)al;
                }
                if (ss == 0 && ah != 0) continue; /* a DC refinement reads raw bits */
                const int id = prog_snapshot(pf, cur, snap, ss == 0 ? td : 4 + ta);
                if (id == -2) { rc = FFHIP_ENOMEM; goto out; }
                if (id < 0) goto out; /* a table not yet defined */
                sc->tab[k] = (uint32_t)id;
            }
            if (ns > 1) {
                ffhip_jpeg_geom g;
                ffhip_jpeg_frame_geom(fr, &g);
                sc->units = (uint32_t)g.mcu_cols * (uint32_t)g.mcu_rows;
                sc->bw = (uint32_t)g.mcu_cols;
            } else { /* the component's own grid: ceil(ceil(W h_c / h_max) / 8) x ceil(ceil(H v_c / v_max) / 8); the first component's factors are the largest */
                const int c = (int)sc->comp[0];
                const uint32_t hmax = (uint32_t)fr->h[0], vmax = (uint32_t)fr->v[0];
                const uint32_t cw = ((uint32_t)fr->width * (uint32_t)fr->h[c] + hmax - 1) / hmax;
                const uint32_t chh = ((uint32_t)fr->height * (uint32_t)fr->v[c] + vmax - 1) / vmax;
                sc->bw = (cw + 7) / 8;
                sc->units = sc->bw * ((chh + 7) / 8);
            }
            sc->restart = restart ? (uint32_t)restart : sc->units;
            sc->n_seg = (sc->units + sc->restart - 1) / sc->restart;
            /* the entropy-coded bytes: up to the first marker that is no RSTn */
            const size_t p = w.p;
            size_t q = p;
            while (q + 1 < len && !(f[q] == 0xFF && f[q + 1] != 0 && !(f[q + 1] >= 0xD0 && f[q + 1] <= 0xD7))) q++;
            if (q + 1 >= len) goto out; /* no marker behind the scan: the EOI is missing */
            if (q - p > 0x7fffffffu) goto out;
            if ((size_t)(sc->n_seg - 1) * 2 > q - p) goto out; /* fewer bytes than the scan's RSTn markers alone take: nothing is sized by such a header */
            pf->raw[pf->n_scans] = f + p;
            pf->raw_len[pf->n_scans] = q - p;
            pf->n_scans++;
            w.p = q;
        }
    }
    if (!pf->n_scans) goto out;
    /* levels: a scan waits for every earlier scan that touches one of its (component, coefficient) pairs */
    for (int a = 0; a < pf->n_scans; a++) {
        struct prog_scan *sa = &pf->scan[a];
        sa->level = 1;
        for (int b = 0; b < a; b++) {
            const struct prog_scan *sb = &pf->scan[b];
            if (sb->se < sa->ss || sa->se < sb->ss) continue;
            int shared = 0;
            for (uint32_t i = 0; i < sa->ncomp; i++)
                for (uint32_t k = 0; k < sb->ncomp; k++) shared |= sa->comp[i] == sb->comp[k];
            if (shared && sb->level + 1 > sa->level) sa->level = sb->level + 1;
        }
    }
    rc = FFHIP_OK;
out:
    free(cur);
    if (rc) ffhip_prog_free(pf);
    return rc;
}

/* k_max as the scans see it: a kept scan (Ss <= k) that reaches beyond k keeps every scan of its band too -- a refinement needs the history of
 * the coefficients it passes over.  Ordinary scripts (bands that do not straddle) leave k_max as it is. */
int ffhip_prog_k_eff(const struct prog_file *pf, int k_max)
{
    int k = k_max < 0 ? 0 : k_max > 63 ? 63 : k_max;
    for (int again = 1; again;) {
        again = 0;
        for (int i = 0; i < pf->n_scans; i++)
            if ((int)pf->scan[i].ss <= k && (int)pf->scan[i].se > k && pf->scan[i].ah != 0) { k = (int)pf->scan[i].se; again = 1; }
    }
    return k;
}

/* A scan's bytes without their stuffing into dst (room for len bytes), cut at the RSTn markers: seg[k] = where interval k starts, seg[found] = the
 * end.  At most n_seg intervals: a further RSTn, like any other marker, ends the scan.  Returns the intervals found. */
uint32_t ffhip_prog_stage_scan(uint8_t *dst, const uint8_t *src, size_t len, uint32_t *seg, uint32_t n_seg)
{
    uint8_t *d = dst;
    const uint8_t *end = src + len;
    uint32_t k = 0;
    seg[0] = 0;
    while (src < end) {
        const uint8_t *ff = memchr(src, 0xFF, (size_t)(end - src));
        const size_t run = ff ? (size_t)(ff - src) : (size_t)(end - src);
        memcpy(d, src, run);
        d += run;
        src += run;
        if (!ff || src + 1 >= end) break; /* (a lone trailing FF is not data) */
        const uint8_t b = src[1];
        if (b == 0) { *d++ = 0xFF; src += 2; continue; }
        if (b < 0xD0 || b > 0xD7 || k + 1 >= n_seg) break;
        seg[++k] = (uint32_t)(d - dst);
        src += 2;
    }
    seg[k + 1] = (uint32_t)(d - dst);
    return k + 1;
}

static _Thread_local int g_prog_last[5];
void ffhip_prog_note_last(const int v[5]) { memcpy(g_prog_last, v, sizeof g_prog_last); }
int ffhip_debug_progressive_last(int out[5])
{
    if (!out) return FFHIP_EINVAL;
    memcpy(out, g_prog_last, sizeof g_prog_last);
    return FFHIP_OK;
}

int ffhip_jpeg_probe_any(const uint8_t *file, size_t len, ffhip_jpeg_geom *geom, int *width, int *height, int *progressive)
{
    if (!file || !geom) return FFHIP_EINVAL;
    if (progressive) *progressive = 0;
    int rc = ffhip_jpeg_probe(file, len, geom, width, height);
    if (rc != FFHIP_EINVAL) return rc;
    struct prog_file *pf = malloc(sizeof *pf);
    if (!pf) return FFHIP_ENOMEM;
    rc = ffhip_prog_parse(file, len, pf);
    if (rc == FFHIP_OK) {
        ffhip_jpeg_frame_geom(&pf->fr, geom);
        if (width) *width = pf->fr.width;
        if (height) *height = pf->fr.height;
        if (progressive) *progressive = 1;
        ffhip_prog_free(pf);
    }
    free(pf);
    return rc;
}

/* the decoder behind ffhip_jpeg_progressive_decode; counts[0..2] += scans decoded, scans skipped, levels */
int ffhip_prog_decode_host(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v,
                           uint16_t *quant, int k_max, int counts[3])
{
    if (!file || !coef_y || !quant || k_max < 0 || k_max > 63) return FFHIP_EINVAL;
    struct prog_file *pf = malloc(sizeof *pf);
    if (!pf) return FFHIP_ENOMEM;
    int rc = ffhip_prog_parse(file, len, pf);
    if (rc) { free(pf); return rc; }
    ffhip_jpeg_geom g;
    ffhip_jpeg_frame_geom(&pf->fr, &g);
    if ((expect && !ffhip_jpeg_geom_same(expect, &g)) || (g.ncomp == 3 && (!coef_u || !coef_v))) {
        ffhip_prog_free(pf);
        free(pf);
        return FFHIP_EINVAL;
    }
    memcpy(quant, pf->fr.quant, sizeof pf->fr.quant);
    const size_t mcus = (size_t)g.mcu_cols * g.mcu_rows;
    memset(coef_y, 0, mcus * g.h * g.v * 64 * sizeof(int16_t));
    if (g.ncomp == 3) {
        memset(coef_u, 0, mcus * 64 * sizeof(int16_t));
        memset(coef_v, 0, mcus * 64 * sizeof(int16_t));
    }
    const struct prog_pic pc = {(uint32_t)g.ncomp, (uint32_t)g.h, (uint32_t)g.v, (uint32_t)g.mcu_cols, (uint32_t)g.mcu_rows, 0};
    int16_t *const plane[3] = {coef_y, coef_u, coef_v};
    const int k_eff = ffhip_prog_k_eff(pf, k_max);
    int levels = 0;
    for (int i = 0; i < pf->n_scans && rc == FFHIP_OK; i++) {
        struct prog_scan sc = pf->scan[i];
        if ((int)sc.ss > k_eff) { if (counts) counts[1]++; continue; }
        if (counts) counts[0]++;
        if ((int)sc.level > levels) levels = (int)sc.level;
        uint8_t *clean = malloc(pf->raw_len[i] + 1);
        uint32_t *seg = malloc(((size_t)sc.n_seg + 1) * sizeof *seg);
        if (!clean || !seg) rc = FFHIP_ENOMEM;
        else if (ffhip_prog_stage_scan(clean, pf->raw[i], pf->raw_len[i], seg, sc.n_seg) != sc.n_seg) rc = FFHIP_EINVAL; /* fewer intervals than the scan needs */
        sc.data = 0;
        sc.seg_base = 0;
        for (uint32_t iv = 0; iv < sc.n_seg && rc == FFHIP_OK; iv++)
            if (ffhip_prog_interval(&sc, &pc, iv, clean, seg, pf->tabs, plane)) rc = FFHIP_EINVAL;
        free(clean);
        free(seg);
    }
    if (counts) counts[2] += levels;
    ffhip_prog_free(pf);
    free(pf);
    return rc;
}

int ffhip_jpeg_progressive_decode(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect, int16_t *coef_y, int16_t *coef_u,
                                  int16_t *coef_v, uint16_t *quant /* [4][64] */, int k_max)
{
    int counts[3] = {0, 0, 0};
    const int rc = ffhip_prog_decode_host(file, len, expect, coef_y, coef_u, coef_v, quant, k_max, counts);
    const int last[5] = {1, counts[0], counts[1], counts[2], 0};
    ffhip_prog_note_last(last);
    return rc;
}
