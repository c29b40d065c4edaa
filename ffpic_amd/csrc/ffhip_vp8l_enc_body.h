/* ffhip_vp8l_enc_body.h -- the lossless WebP encoder's rule (include/ffpic_hip.h "Lossless WebP encoding") as ONE body for
 * the host entries (ffhip_vp8l_enc.c, gcc) and the kernels (ffhip_vp8l_enc_gpu.hip, hipcc).
 *
 * The pieces without lanes (FFHIP_DEF_HD): a source pixel with green subtracted, the 14 predictors' costs and the choice, a pixel's residual,
 * the distance-code map, a token's bits, the file's last step and the bound.  The predictors themselves are ffhip_vp8l_body.h's, the
 * decoder's.  The pieces in LANE FORM, as ffhip_deflate_body.h defines it (a section is what lane `lane` does; sections talk only through
 * FFHIP_DEF_MAX / _ADD / _OR): a chunk's parse, a picture's codes with the file's head, a chunk's bit count and a chunk's bits.  The length
 * rule is ffhip_def_code_lengths, the canonical codes are ffhip_def_codes, the bits go through ffhip_def_put.
 * Every loop runs to a bound known at its entry. */
#ifndef FFHIP_VP8L_ENC_BODY_H
#define FFHIP_VP8L_ENC_BODY_H

#include "ffpic_hip.h"
#include "ffhip_vp8l_body.h"
#include "ffhip_deflate_body.h"

#define FFHIP_VE_CHUNK 4096u /* FFHIP_VP8L_ENC_CHUNK of the public header */
#define FFHIP_VE_MIN_MATCH 3u
#define FFHIP_VE_TILE (1 << FFHIP_VP8L_ENC_TILE_BITS)
/* the five alphabets of a group, end to end: the picture's counters and its table of codes */
#define FFHIP_VE_G 0
#define FFHIP_VE_R 280
#define FFHIP_VE_B 536
#define FFHIP_VE_A 792
#define FFHIP_VE_D 1048
#define FFHIP_VE_NSYM 1088
#define FFHIP_VE_TOK_LIT 0x80000000u   /* the position's residual word as a literal */
#define FFHIP_VE_TOK_MATCH 0x40000000u /* | length << 1 | 1 for distance xsize, 0 for distance 1 */
#define FFHIP_VE_HEAD_BITS 168u        /* RIFF, size, WEBP, VP8L, size, 2f: the VP8L bits start here */
#define FFHIP_VE_HEAD_BOUND 4096u      /* the 21 bytes, the transform bits and the tables of both groups: below 31 200 bits */

FFHIP_DEF_HD uint32_t ffhip_ve_sub_size(uint32_t n) { return (n + FFHIP_VE_TILE - 1) >> FFHIP_VP8L_ENC_TILE_BITS; }
FFHIP_DEF_HD uint64_t ffhip_ve_chunks(uint64_t pixels) { return (pixels + FFHIP_VE_CHUNK - 1) / FFHIP_VE_CHUNK; }

/* a CERTAIN bound on the file: the head, 16 bits a tile for the sub-image, 60 bits a pixel (a literal is four codes of at most 15 bits; a
 * match covers at least two pixels with at most 15 + 10 + 15 bits), a byte of padding */
FFHIP_DEF_HD uint64_t ffhip_ve_bound(uint32_t w, uint32_t h)
{
    const uint64_t tiles = (uint64_t)ffhip_ve_sub_size(w) * ffhip_ve_sub_size(h), pixels = (uint64_t)w * h;
    return FFHIP_VE_HEAD_BOUND + 2 * tiles + (pixels * 60 + 7) / 8 + 2;
}

/* pixel (x, y) as an ARGB word: grey as R = G = B, a missing alpha 255; with FFHIP_VP8L_ENC_SUBTRACT_GREEN red and blue less green */
FFHIP_DEF_HD uint32_t ffhip_ve_pixel(const ffhip_png_source *s, int flags, int64_t x, int64_t y)
{
    const uint8_t *p = s->pixels + y * s->row_stride + x * s->pixel_stride;
    uint32_t r, g, b, a = 255;
    if (s->channels <= 2) {
        r = g = b = p[s->chan[0]];
        if (s->channels == 2) a = p[s->chan[1]];
    } else {
        r = p[s->chan[0]];
        g = p[s->chan[1]];
        b = p[s->chan[2]];
        if (s->channels == 4) a = p[s->chan[3]];
    }
    if (flags & FFHIP_VP8L_ENC_SUBTRACT_GREEN) {
        r = (r - g) & 255u;
        b = (b - g) & 255u;
    }
    return a << 24 | r << 16 | g << 8 | b;
}

/* per byte, a - b modulo 256 */
FFHIP_DEF_HD uint32_t ffhip_ve_sub(uint32_t a, uint32_t b)
{
    return (((a | 0x00ff00ffu) - (b & 0xff00ff00u)) & 0xff00ff00u) | (((a | 0xff00ff00u) - (b & 0x00ff00ffu)) & 0x00ff00ffu);
}

/* a residual word's four bytes read as signed, their absolute values' sum */
FFHIP_DEF_HD uint32_t ffhip_ve_cost(uint32_t r)
{
    uint32_t s = 0;
    FFHIP_VP8L_UNROLL
    for (int k = 0; k < 32; k += 8) {
        const uint32_t v = (r >> k) & 255u;
        s += v < 128u ? v : 256u - v;
    }
    return s;
}

/* What predicts pixel (x, y) of a picture w wide.  1: the format fixes it whatever the mode, *fixed is the prediction (the first pixel
 * against 0xff000000, the top row from the left, the left column from above).  0: the mode decides; n = L, T, TR, TL, the rightmost
 * pixel's TR being the row's first pixel */
FFHIP_DEF_HD int ffhip_ve_neighbours(const ffhip_png_source *s, int flags, int64_t x, int64_t y, uint32_t n[4], uint32_t *fixed)
{
    if (y == 0) {
        *fixed = x ? ffhip_ve_pixel(s, flags, x - 1, 0) : 0xff000000u;
        return 1;
    }
    if (x == 0) {
        *fixed = ffhip_ve_pixel(s, flags, 0, y - 1);
        return 1;
    }
    n[0] = ffhip_ve_pixel(s, flags, x - 1, y);
    n[1] = ffhip_ve_pixel(s, flags, x, y - 1);
    n[2] = x + 1 < s->width ? ffhip_ve_pixel(s, flags, x + 1, y - 1) : ffhip_ve_pixel(s, flags, 0, y);
    n[3] = ffhip_ve_pixel(s, flags, x - 1, y - 1);
    return 0;
}

/* sums[mode] += the cost of pixel (x, y) under every mode; a pixel the format fixes adds nothing, which is the same for all */
FFHIP_DEF_HD void ffhip_ve_costs(const ffhip_png_source *s, int flags, int64_t x, int64_t y, uint32_t sums[14])
{
    uint32_t n[4], fixed;
    if (ffhip_ve_neighbours(s, flags, x, y, n, &fixed)) return;
    const uint32_t px = ffhip_ve_pixel(s, flags, x, y), L = n[0], T = n[1], TR = n[2], TL = n[3];
    sums[0] += ffhip_ve_cost(ffhip_ve_sub(px, 0xff000000u));
#define FFHIP_VE_ONE(k, expr) sums[k] += ffhip_ve_cost(ffhip_ve_sub(px, expr));
    FFHIP_VP8L_MODES(FFHIP_VE_ONE)
#undef FFHIP_VE_ONE
}

/* the mode of the smallest sum, the lowest of equal ones */
FFHIP_DEF_HD int ffhip_ve_choose(const uint32_t sums[14])
{
    int m = 0;
    uint32_t best = sums[0];
    FFHIP_VP8L_UNROLL
    for (int k = 1; k < 14; k++)
        if (sums[k] < best) {
            best = sums[k];
            m = k;
        }
    return m;
}

/* the residual word of pixel (x, y) whose tile has `mode`: the pixel itself without FFHIP_VP8L_ENC_PREDICT */
FFHIP_DEF_HD uint32_t ffhip_ve_residual(const ffhip_png_source *s, int flags, int mode, int64_t x, int64_t y)
{
    const uint32_t px = ffhip_ve_pixel(s, flags, x, y);
    if (!(flags & FFHIP_VP8L_ENC_PREDICT)) return px;
    uint32_t n[4], fixed;
    if (!ffhip_ve_neighbours(s, flags, x, y, n, &fixed)) fixed = ffhip_vp8l_predict(mode, n[0], n[1], n[2], n[3]);
    return ffhip_ve_sub(px, fixed);
}

/* the smallest distance code that decodes to distance d in a picture xs wide, for the distances the parse makes (1 and xs): the
 * neighbourhood map's code 1 is the pixel above, its code 2 the pixel to the left; any other distance is d + 120 */
FFHIP_DEF_HD uint32_t ffhip_ve_dist_code(uint32_t d, uint32_t xs) { return d == xs ? 1u : d == 1u ? 2u : d + 120u; }

/* a length or a distance code as prefix symbol, count of extra bits and their value */
FFHIP_DEF_HD int ffhip_ve_prefix_of(uint32_t value, int *extra_bits, uint32_t *extra)
{
    const uint32_t d = value - 1;
    if (d < 4) {
        *extra_bits = 0;
        *extra = 0;
        return (int)d;
    }
    const int hb = 31 - __builtin_clz(d), e = hb - 1;
    *extra_bits = e;
    *extra = d & ((1u << e) - 1);
    return 2 * hb + (int)((d >> e) & 1u);
}

/* the format's order of the 19 code-length code lengths: 17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, .. 15 */
FFHIP_DEF_HD int ffhip_ve_clen_order(int i) { return i == 0 ? 17 : i == 1 ? 18 : i < 8 ? i - 2 : i == 8 ? 16 : i - 3; }

FFHIP_DEF_HD uint32_t ffhip_ve_tok_len(uint32_t tok) { return (tok >> 1) & 0x1fffu; }

/* A token's bits under a group's table (entry: bits << 16 | the code, its first bit lowest): *v, the count (at most 60) returned; 0 for no
 * token.  word: the position's residual word */
FFHIP_DEF_HD int ffhip_ve_token_bits(const uint32_t *table, uint32_t tok, uint32_t word, uint32_t xs, uint64_t *v)
{
    *v = 0;
    if (tok & FFHIP_VE_TOK_LIT) {
        uint32_t e = table[FFHIP_VE_G + ((word >> 8) & 255u)];
        uint64_t b = e & 0xffffu;
        int n = (int)(e >> 16);
        e = table[FFHIP_VE_R + ((word >> 16) & 255u)];
        b |= (uint64_t)(e & 0xffffu) << n;
        n += (int)(e >> 16);
        e = table[FFHIP_VE_B + (word & 255u)];
        b |= (uint64_t)(e & 0xffffu) << n;
        n += (int)(e >> 16);
        e = table[FFHIP_VE_A + (word >> 24)];
        b |= (uint64_t)(e & 0xffffu) << n;
        n += (int)(e >> 16);
        *v = b;
        return n;
    }
    if (!(tok & FFHIP_VE_TOK_MATCH)) return 0;
    int eb;
    uint32_t ev;
    int sym = ffhip_ve_prefix_of(ffhip_ve_tok_len(tok), &eb, &ev);
    uint32_t e = table[FFHIP_VE_G + 256 + sym];
    uint64_t b = e & 0xffffu;
    int n = (int)(e >> 16);
    b |= (uint64_t)ev << n;
    n += eb;
    sym = ffhip_ve_prefix_of(ffhip_ve_dist_code((tok & 1u) ? xs : 1u, xs), &eb, &ev);
    e = table[FFHIP_VE_D + sym];
    b |= (uint64_t)(e & 0xffffu) << n;
    n += (int)(e >> 16);
    b |= (uint64_t)ev << n;
    n += eb;
    *v = b;
    return n;
}

/* nbits <= 64 bits of v at bit `pos` of the zeroed words */
FFHIP_DEF_FN void ffhip_ve_put(uint32_t *words, uint64_t pos, uint64_t v, int nbits)
{
    if (nbits > 32) {
        ffhip_def_put(words, pos, v & 0xffffffffu, 32);
        ffhip_def_put(words, pos + 32, v >> 32, nbits - 32);
    } else
        ffhip_def_put(words, pos, v, nbits);
}

/* exclusive prefix sum of vals[0 .. 64) in front of `lane`, and the sum of all */
FFHIP_DEF_FN uint32_t ffhip_ve_prefix(const uint32_t *vals, int lane, uint32_t *total)
{
#ifdef __HIPCC__
    const uint32_t own = vals[lane];
    uint32_t incl = own;
    FFHIP_DEF_ROLLED
    for (int off = 1; off < FFHIP_DEF_LANES; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    *total = __shfl(incl, FFHIP_DEF_LANES - 1);
    return incl - own;
#else
    uint32_t before = 0, all = 0;
    for (int k = 0; k < FFHIP_DEF_LANES; k++) {
        if (k < lane) before += vals[k];
        all += vals[k];
    }
    *total = all;
    return before;
#endif
}

/* ---- a chunk's parse ---- */
typedef struct ffhip_ve_parse_store {
    uint32_t hist[FFHIP_VE_NSYM];
    uint32_t lane_a[FFHIP_DEF_LANES], lane_b[FFHIP_DEF_LANES]; /* a step's lengths and which distance */
} ffhip_ve_parse_store;

/* Chunk [at, at + n) of the residual picture res (xs words a row), 0 < n <= FFHIP_VE_CHUNK.  tok: the chunk's n token words, one a position
 * (0 where no token starts); hist: the picture's FFHIP_VE_NSYM counters, which take the chunk's counts by FFHIP_DEF_ADD */
FFHIP_DEF_FN void ffhip_ve_parse(ffhip_ve_parse_store *m, const uint32_t *res, uint64_t at, uint32_t n, uint32_t xs, uint32_t *tok, uint32_t *hist)
{
    const uint32_t *in = res + at;
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int k = lane; k < FFHIP_VE_NSYM; k += FFHIP_DEF_LANES) m->hist[k] = 0;
    FFHIP_DEF_LANES_END
    uint32_t next = 0; /* the first position no token covers yet */
    FFHIP_DEF_ROLLED
    for (uint32_t base = 0; base < n; base += FFHIP_DEF_LANES) {
        FFHIP_DEF_LANES_BEGIN
            const uint32_t p = base + (uint32_t)lane;
            uint32_t best = 0, above = 0;
            if (p < n && p >= next) {
                const uint32_t maxlen = n - p;
                FFHIP_DEF_ROLLED
                for (uint32_t c = 0; c < 2 && best < maxlen; c++) {
                    const uint32_t dist = c ? xs : 1u;
                    if (c && xs == 1u) break; /* one candidate */
                    if (at + p < dist) continue;
                    const uint32_t *q = in + ((int64_t)p - (int64_t)dist);
                    uint32_t l = 0;
                    FFHIP_DEF_ROLLED
                    while (l < maxlen && q[l] == in[p + l]) l++;
                    if (l >= FFHIP_VE_MIN_MATCH && l > best) {
                        best = l;
                        above = c;
                    }
                }
            }
            m->lane_a[lane] = best;
            m->lane_b[lane] = above;
        FFHIP_DEF_LANES_END
        uint64_t starts = 0;
        FFHIP_DEF_ROLLED
        for (int turn = 0; turn < FFHIP_DEF_LANES; turn++) {
            if (next >= n || next >= base + FFHIP_DEF_LANES) break;
            const uint32_t l = next - base, len = FFHIP_DEF_UNIFORM(m->lane_a[l]);
            starts |= 1ull << l;
            next += len ? len : 1u;
        }
        FFHIP_DEF_LANES_BEGIN
            const uint32_t p = base + (uint32_t)lane;
            if (p < n) {
                uint32_t t = 0;
                if ((starts >> lane) & 1) {
                    const uint32_t len = m->lane_a[lane], above = m->lane_b[lane];
                    int eb;
                    uint32_t ev;
                    if (len) {
                        t = FFHIP_VE_TOK_MATCH | (len << 1) | above;
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_G + 256 + ffhip_ve_prefix_of(len, &eb, &ev)], 1u);
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_D + ffhip_ve_prefix_of(ffhip_ve_dist_code(above ? xs : 1u, xs), &eb, &ev)], 1u);
                    } else {
                        const uint32_t w = in[p];
                        t = FFHIP_VE_TOK_LIT;
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_G + ((w >> 8) & 255u)], 1u);
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_R + ((w >> 16) & 255u)], 1u);
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_B + (w & 255u)], 1u);
                        FFHIP_DEF_ADD(&m->hist[FFHIP_VE_A + (w >> 24)], 1u);
                    }
                }
                tok[p] = t;
            }
        FFHIP_DEF_LANES_END
    }
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int k = lane; k < FFHIP_VE_NSYM; k += FFHIP_DEF_LANES)
            if (m->hist[k]) FFHIP_DEF_ADD(&hist[k], m->hist[k]);
    FFHIP_DEF_LANES_END
}

/* ---- a picture's codes and the file's head ---- */
typedef struct ffhip_ve_codes_store {
    ffhip_def_store d; /* the length rule's store; freq_ll, len_ll and code_ll hold the alphabet at hand, seq_*, *_cl its lengths' coding */
    uint32_t sub_g[16]; /* the sub-image's table of modes */
    uint32_t lanes[FFHIP_DEF_LANES];
    uint32_t pos_lo, pos_hi; /* the next bit of the file */
    uint32_t simple, n_used, cl_used;
} ffhip_ve_codes_store;

FFHIP_DEF_FN uint64_t ffhip_ve_pos(const ffhip_ve_codes_store *m) { return (uint64_t)m->pos_lo | (uint64_t)m->pos_hi << 32; }
/* one lane's: nbits <= 32 of v at the store's position */
FFHIP_DEF_FN void ffhip_ve_emit(ffhip_ve_codes_store *m, uint32_t *words, uint64_t v, int nbits)
{
    const uint64_t pos = ffhip_ve_pos(m);
    ffhip_def_put(words, pos, v, nbits);
    m->pos_lo = (uint32_t)(pos + (uint64_t)nbits);
    m->pos_hi = (uint32_t)((pos + (uint64_t)nbits) >> 32);
}

/* One alphabet of n symbols with the counts freq: its lengths by the rule, the code written at the store's position -- the simple form for
 * at most two used symbols, all below 256 (none used: symbol 0), otherwise the lengths under the 19-symbol code -- and table[0 .. n) when
 * table is not NULL.  A code of ONE used symbol has the empty word: its tokens take no bits. */
FFHIP_DEF_NOINLINE void ffhip_ve_put_code(ffhip_ve_codes_store *m, const uint32_t *freq, int n, uint32_t *words, uint32_t *table)
{
    ffhip_def_store *d = &m->d;
    ffhip_def_code_lengths(d, freq, n, 15, d->len_ll);
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) {
            uint32_t used = 0;
            int top = 0;
            FFHIP_DEF_ROLLED
            for (int s = 0; s < n; s++)
                if (d->len_ll[s]) {
                    used++;
                    top = s;
                }
            m->n_used = used;
            m->simple = used == 0 || (used <= 2 && top < 256);
            if (!m->simple) {
                /* the lengths run by run of equal values.  Zeros: 18 for 138 .. 11, 17 for 10 .. 3, then singly.  A value v: once, unless it
                 * is the last non-zero value written (8 at the start); then 16 for 6 .. 3 of the rest, then singly */
                uint32_t k = 0;
                int prev = 8;
                FFHIP_DEF_ROLLED
                for (int s = 0; s < 20; s++) d->freq_cl[s] = 0;
                FFHIP_DEF_ROLLED
                for (int i = 0; i < n;) {
                    const int v = d->len_ll[i];
                    int run = 1;
                    FFHIP_DEF_ROLLED
                    while (i + run < n && d->len_ll[i + run] == v) run++;
                    i += run;
                    if (v && v != prev) {
                        d->seq_sym[k] = (uint8_t)v; d->seq_ext[k++] = 0;
                        prev = v;
                        run--;
                    }
                    FFHIP_DEF_ROLLED
                    while (run >= 3) {
                        const int take = v ? (run > 6 ? 6 : run) : (run > 138 ? 138 : run);
                        if (v) { d->seq_sym[k] = 16; d->seq_ext[k++] = (uint8_t)(take - 3); }
                        else if (take >= 11) { d->seq_sym[k] = 18; d->seq_ext[k++] = (uint8_t)(take - 11); }
                        else { d->seq_sym[k] = 17; d->seq_ext[k++] = (uint8_t)(take - 3); }
                        run -= take;
                    }
                    FFHIP_DEF_ROLLED
                    for (; run > 0; run--) { d->seq_sym[k] = (uint8_t)v; d->seq_ext[k++] = 0; }
                }
                d->n_seq = k;
                FFHIP_DEF_ROLLED
                for (uint32_t i = 0; i < k; i++) d->freq_cl[d->seq_sym[i]]++;
            }
        }
    FFHIP_DEF_LANES_END
    if (FFHIP_DEF_UNIFORM(m->simple)) {
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) {
                int s0 = 0, s1 = 0, seen = 0;
                FFHIP_DEF_ROLLED
                for (int s = 0; s < n; s++)
                    if (d->len_ll[s]) {
                        if (seen++) s1 = s; else s0 = s;
                    }
                ffhip_ve_emit(m, words, 1, 1);
                ffhip_ve_emit(m, words, m->n_used == 2, 1);
                ffhip_ve_emit(m, words, s0 > 1, 1);
                ffhip_ve_emit(m, words, (uint64_t)s0, s0 > 1 ? 8 : 1);
                if (m->n_used == 2) ffhip_ve_emit(m, words, (uint64_t)s1, 8);
            }
        FFHIP_DEF_LANES_END
    } else {
        ffhip_def_code_lengths(d, d->freq_cl, 19, 7, d->len_cl);
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) {
                ffhip_def_codes(d->len_cl, 19, d->code_cl);
                uint32_t cl_used = 0;
                int count = 19;
                FFHIP_DEF_ROLLED
                for (int s = 0; s < 19; s++) cl_used += d->len_cl[s] != 0;
                FFHIP_DEF_ROLLED
                while (count > 4 && !d->len_cl[ffhip_ve_clen_order(count - 1)]) count--;
                ffhip_ve_emit(m, words, 0, 1);
                ffhip_ve_emit(m, words, (uint64_t)(count - 4), 4);
                FFHIP_DEF_ROLLED
                for (int i = 0; i < count; i++) ffhip_ve_emit(m, words, d->len_cl[ffhip_ve_clen_order(i)], 3);
                ffhip_ve_emit(m, words, 0, 1); /* every length is coded: no max_symbol */
                FFHIP_DEF_ROLLED
                for (uint32_t i = 0; i < d->n_seq; i++) {
                    const int s = d->seq_sym[i], e = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0, nb = cl_used == 1 ? 0 : d->len_cl[s];
                    ffhip_ve_emit(m, words, (nb ? (uint64_t)d->code_cl[s] : 0u) | ((uint64_t)d->seq_ext[i] << nb), nb + e);
                }
            }
        FFHIP_DEF_LANES_END
    }
    if (!table) return;
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) ffhip_def_codes(d->len_ll, n, d->code_ll);
    FFHIP_DEF_LANES_END
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int s = lane; s < n; s += FFHIP_DEF_LANES)
            table[s] = d->len_ll[s] && m->n_used > 1 ? (uint32_t)d->len_ll[s] << 16 | d->code_ll[s] : 0u;
    FFHIP_DEF_LANES_END
}

/* an alphabet of n symbols of which only `sym` is used (none: sym < 0), without a table */
FFHIP_DEF_FN void ffhip_ve_put_single(ffhip_ve_codes_store *m, int n, int sym, uint32_t *words)
{
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int s = lane; s < n; s += FFHIP_DEF_LANES) m->d.freq_ll[s] = s == sym;
    FFHIP_DEF_LANES_END
    ffhip_ve_put_code(m, m->d.freq_ll, n, words, (uint32_t *)0);
}

/* The file's head into the zeroed words: RIFF / WEBP / VP8L (the two sizes are ffhip_ve_finish's), the VP8L header, the transforms in the
 * file's order with the coded sub-image (modes: a byte a tile), the picture's five codes from its counters hist.  table: the picture's
 * FFHIP_VE_NSYM entries.  Returns the bit where the first chunk's tokens start */
FFHIP_DEF_FN uint64_t ffhip_ve_codes(ffhip_ve_codes_store *m, uint32_t w, uint32_t h, int has_alpha, int flags, const uint8_t *modes, const uint32_t *hist,
                                     uint32_t *words, uint32_t *table)
{
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) {
            m->pos_lo = 0; m->pos_hi = 0;
            ffhip_ve_emit(m, words, 0x46464952u, 32); /* RIFF */
            m->pos_lo = 64;
            ffhip_ve_emit(m, words, 0x50424557u, 32); /* WEBP */
            ffhip_ve_emit(m, words, 0x4c385056u, 32); /* VP8L */
            m->pos_lo = 160;
            ffhip_ve_emit(m, words, 0x2f, 8);
            ffhip_ve_emit(m, words, w - 1, 14);
            ffhip_ve_emit(m, words, h - 1, 14);
            ffhip_ve_emit(m, words, has_alpha != 0, 1);
            ffhip_ve_emit(m, words, 0, 3);
            if (flags & FFHIP_VP8L_ENC_SUBTRACT_GREEN) ffhip_ve_emit(m, words, 1 | FFHIP_VP8L_ADD_GREEN << 1, 3);
            if (flags & FFHIP_VP8L_ENC_PREDICT) {
                ffhip_ve_emit(m, words, 1 | FFHIP_VP8L_PREDICTOR << 1, 3);
                ffhip_ve_emit(m, words, FFHIP_VP8L_ENC_TILE_BITS - 2, 3);
                ffhip_ve_emit(m, words, 0, 1); /* the sub-image has no colour cache */
            }
        }
    FFHIP_DEF_LANES_END
    if (flags & FFHIP_VP8L_ENC_PREDICT) {
        const uint32_t tiles = ffhip_ve_sub_size(w) * ffhip_ve_sub_size(h);
        FFHIP_DEF_LANES_BEGIN
            FFHIP_DEF_ROLLED
            for (int s = lane; s < 280; s += FFHIP_DEF_LANES) m->d.freq_ll[s] = 0;
        FFHIP_DEF_LANES_END
        FFHIP_DEF_LANES_BEGIN
            FFHIP_DEF_ROLLED
            for (uint32_t t = (uint32_t)lane; t < tiles; t += FFHIP_DEF_LANES) FFHIP_DEF_ADD(&m->d.freq_ll[modes[t]], 1u);
        FFHIP_DEF_LANES_END
        ffhip_ve_put_code(m, m->d.freq_ll, 280, words, m->d.w); /* the table's first 14 entries matter; w is free between the rule's runs */
        FFHIP_DEF_LANES_BEGIN
            if (lane < 16) m->sub_g[lane] = m->d.w[lane];
        FFHIP_DEF_LANES_END
        ffhip_ve_put_single(m, 256, 0, words);
        ffhip_ve_put_single(m, 256, 0, words);
        ffhip_ve_put_single(m, 256, 255, words);
        ffhip_ve_put_single(m, 40, -1, words);
        uint64_t pos = (uint64_t)FFHIP_DEF_UNIFORM(m->pos_lo) | (uint64_t)FFHIP_DEF_UNIFORM(m->pos_hi) << 32;
        FFHIP_DEF_ROLLED
        for (uint32_t base = 0; base < tiles; base += FFHIP_DEF_LANES) {
            FFHIP_DEF_LANES_BEGIN
                const uint32_t t = base + (uint32_t)lane;
                m->lanes[lane] = t < tiles ? m->sub_g[modes[t]] >> 16 : 0u;
            FFHIP_DEF_LANES_END
            FFHIP_DEF_LANES_BEGIN
                const uint32_t t = base + (uint32_t)lane;
                uint32_t all;
                const uint32_t before = ffhip_ve_prefix(m->lanes, lane, &all);
                if (t < tiles) {
                    const uint32_t e = m->sub_g[modes[t]];
                    ffhip_def_put(words, pos + before, e & 0xffffu, (int)(e >> 16));
                }
                if (lane == 0) m->n_used = all;
            FFHIP_DEF_LANES_END
            pos += FFHIP_DEF_UNIFORM(m->n_used); /* written again only behind the next step's first barrier */
        }
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) {
                m->pos_lo = (uint32_t)pos;
                m->pos_hi = (uint32_t)(pos >> 32);
            }
        FFHIP_DEF_LANES_END
    }
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) ffhip_ve_emit(m, words, 0, 3); /* no further transform, no colour cache, no meta prefix image */
    FFHIP_DEF_LANES_END
    ffhip_ve_put_code(m, hist + FFHIP_VE_G, 280, words, table + FFHIP_VE_G);
    ffhip_ve_put_code(m, hist + FFHIP_VE_R, 256, words, table + FFHIP_VE_R);
    ffhip_ve_put_code(m, hist + FFHIP_VE_B, 256, words, table + FFHIP_VE_B);
    ffhip_ve_put_code(m, hist + FFHIP_VE_A, 256, words, table + FFHIP_VE_A);
    ffhip_ve_put_code(m, hist + FFHIP_VE_D, 40, words, table + FFHIP_VE_D);
    return (uint64_t)FFHIP_DEF_UNIFORM(m->pos_lo) | (uint64_t)FFHIP_DEF_UNIFORM(m->pos_hi) << 32;
}

/* ---- a chunk's bits: counted, then written ---- */
/* the bits of the chunk's n tokens; lanes: 64 words of the store */
FFHIP_DEF_FN uint32_t ffhip_ve_count(uint32_t *lanes, const uint32_t *table, const uint32_t *in, const uint32_t *tok, uint32_t n, uint32_t xs)
{
    FFHIP_DEF_LANES_BEGIN
        uint32_t bits = 0;
        FFHIP_DEF_ROLLED
        for (uint32_t p = (uint32_t)lane; p < n; p += FFHIP_DEF_LANES) {
            uint64_t v;
            bits += (uint32_t)ffhip_ve_token_bits(table, tok[p], in[p], xs, &v);
        }
        lanes[lane] = bits;
    FFHIP_DEF_LANES_END
    uint32_t all = 0;
    FFHIP_DEF_ROLLED
    for (int k = 0; k < FFHIP_DEF_LANES; k++) all += lanes[k];
    return all;
}

/* the chunk's tokens' bits from bit `pos` of the file's zeroed words on */
FFHIP_DEF_FN void ffhip_ve_write(uint32_t *lanes, const uint32_t *table, const uint32_t *in, const uint32_t *tok, uint32_t n, uint32_t xs, uint32_t *words,
                                 uint64_t pos)
{
    FFHIP_DEF_ROLLED
    for (uint32_t base = 0; base < n; base += FFHIP_DEF_LANES) {
        FFHIP_DEF_LANES_BEGIN
            const uint32_t p = base + (uint32_t)lane;
            uint64_t v;
            lanes[lane] = p < n ? (uint32_t)ffhip_ve_token_bits(table, tok[p], in[p], xs, &v) : 0u;
        FFHIP_DEF_LANES_END
        FFHIP_DEF_LANES_BEGIN
            const uint32_t p = base + (uint32_t)lane;
            uint32_t all;
            const uint32_t before = ffhip_ve_prefix(lanes, lane, &all);
            if (p < n) {
                uint64_t v;
                const int nb = ffhip_ve_token_bits(table, tok[p], in[p], xs, &v);
                ffhip_ve_put(words, pos + before, v, nb);
            }
            if (lane == 0) lanes[FFHIP_DEF_LANES] = all;
        FFHIP_DEF_LANES_END
        pos += FFHIP_DEF_UNIFORM(lanes[FFHIP_DEF_LANES]); /* written again only behind the next step's first barrier */
    }
}

/* The file's last step, one lane's: end_bits is the bit behind the last token.  The VP8L chunk's size and, with a byte of padding when that
 * is odd, the RIFF size into words 4 and 1, which nothing else writes.  Returns the file's size, which is even */
FFHIP_DEF_HD uint64_t ffhip_ve_finish(uint32_t *words, uint64_t end_bits)
{
    const uint64_t payload = ((end_bits + 7) >> 3) - 20, padded = payload + (payload & 1);
    words[4] = (uint32_t)payload;
    words[1] = (uint32_t)(12 + padded);
    return 20 + padded;
}

#endif
