/* ffhip_inflate_body.h -- inflate of a zlib-wrapped deflate stream (RFC 1950, RFC 1951) in the form one WAVE runs it, as k_inflate
 * (ffhip_inflate_gpu.hip) and the host model ffhip_inflate_model (ffhip_inflate_model.c) compile it.  Plain C without
 * builtins; what ffhip_inflate.c accepts and refuses, this accepts and refuses, `partial` included.
 *
 * Two parts.
 *   The SERIAL part is wave-uniform: every lane runs it on the same bytes and gets the same values (the kernel's lanes all store the same
 * value at the same address of the storage, which is LDS there and a stack object in the model).  ffhip_inf_begin checks the zlib header;
 * ffhip_inf_batch reads block headers, builds the tables of a fixed or dynamic block and decodes up to FFHIP_INF_TOKENS tokens -- a
 * literal, or a length and a distance -- into at most FFHIP_INF_STEPS STEPS, each with its output offset (a running sum over the tokens).
 * The bit reader is ffhip_inflate.c's: up to 64 bits held, COUNTED zero bytes fed beyond the end, and a decode that consumed one of them
 * refused by the next check, so that no byte the caller did not give is ever read.
 *   The WRITER part is what lane L does in one step: ffhip_inf_step_load, then ffhip_inf_step_store.  A run of literal tokens is one step,
 * lane k stores byte k.  A match is copied in steps of 64 bytes; lane k of the step that starts at byte k0 of the match reads
 * dst[match - distance + ((k0 + k) % distance)], an address in FRONT of the match whatever the distance: no load of a step reads a byte a
 * store of the same step (or of an earlier step of the same match) writes, distance < length included.  A stored block is copied 64 bytes
 * a step.  The caller runs a step as all its loads, then all its stores, and orders the stores of earlier steps before the loads of a
 * match's first step (the kernel: a workgroup-scope fence; the model: nothing to do).
 *
 * The two invariants of the loops of ffhip_inf_batch:
 *   (1) every turn of every loop consumes at least one input bit or ends the stream;
 *   (2) an overrun of the counted padding is an error at the latest on the next turn.
 * On top of them every turn is counted, and a stream that takes more than 8 x len + 64 turns is FFHIP_EINVAL: (1) gives a valid stream
 * at most 8 x len turns.  The loops that consume no input -- the table builds, the steps of one match (at most five) -- are bounded by
 * constants. */
#ifndef FFHIP_INFLATE_BODY_H
#define FFHIP_INFLATE_BODY_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#ifdef __HIPCC__
#define FFHIP_INF_FN __host__ __device__ static inline __attribute__((always_inline)) /* the state stays in registers */
#else
#define FFHIP_INF_FN static inline
#endif

#define FFHIP_INF_EINVAL (-22) /* FFHIP_EINVAL */
#define FFHIP_INF_PRIMARY 10
#define FFHIP_INF_MAXBITS 15
#define FFHIP_INF_LANES 64
#define FFHIP_INF_TOKENS 64 /* of a batch */
#define FFHIP_INF_STEPS 64  /* of a batch: a match takes up to five */

enum { FFHIP_INF_LITERALS = 0, FFHIP_INF_MATCH = 1, FFHIP_INF_STORED = 2 };

typedef struct ffhip_inf_table {
    uint16_t fast[1 << FFHIP_INF_PRIMARY];  /* symbol << 4 | length; 0: no code of up to FFHIP_INF_PRIMARY bits starts like this */
    uint16_t count[FFHIP_INF_MAXBITS + 1]; /* codes of each length */
    uint16_t symbol[288];                  /* symbols in canonical order */
} ffhip_inf_table;

/* n <= 64 bytes to dst[to ..): lane k's is byte k */
typedef struct ffhip_inf_step {
    uint64_t to;
    uint64_t from;  /* literals: the first one's index in lit_byte[]; match: k0, the step's first byte within the match; stored: offset in src */
    uint32_t dist;  /* match */
    uint16_t n, kind;
} ffhip_inf_step;

/* what the serial part keeps outside registers: LDS in the kernel, a stack object in the model */
typedef struct ffhip_inf_store {
    ffhip_inf_table lit, dist; /* dist holds the code-length code while a dynamic block's lengths are read */
    ffhip_inf_step step[FFHIP_INF_STEPS];
    uint8_t lit_byte[FFHIP_INF_TOKENS];
    uint8_t lengths[320];
    uint16_t offs[FFHIP_INF_MAXBITS + 2];
} ffhip_inf_store;

enum { FFHIP_INF_AT_HEADER = 0, FFHIP_INF_IN_CODES = 1, FFHIP_INF_IN_STORED = 2 };

typedef struct ffhip_inf_state {
    const uint8_t *src;
    uint64_t ip, end;     /* offsets in src: the next byte to load, the stream's length */
    uint64_t hold;
    int bits, padded;     /* valid bits in hold, zero padding included; zero BITS fed beyond the end */
    uint64_t at, cap;     /* output bytes laid out so far */
    uint64_t turns, max_turns;
    uint64_t stored_from; /* the rest of a stored block: where in src, how many bytes */
    uint32_t stored_left;
    int partial, where, last, full, done;
    uint64_t out_len;     /* 0 until `done` */
    uint32_t want;        /* done && !full: the stream's Adler-32 */
} ffhip_inf_state;

FFHIP_INF_FN uint64_t ffhip_inf_load64(const uint8_t *p)
{
#ifdef __HIP_DEVICE_COMPILE__
    typedef struct __attribute__((packed)) { uint64_t v; } run8; /* one load at any byte address */
    return ((const run8 *)p)->v;
#else
    uint64_t v;
    memcpy(&v, p, 8); /* little-endian hosts only, as the rest of the library */
    return v;
#endif
}

FFHIP_INF_FN void ffhip_inf_refill(ffhip_inf_state *r)
{
    if (r->end - r->ip >= 8) {
        r->hold |= ffhip_inf_load64(r->src + r->ip) << r->bits;
        r->ip += (uint64_t)((63 - r->bits) >> 3);
        r->bits |= 56;
        return;
    }
    while (r->bits <= 56) {
        if (r->ip < r->end) r->hold |= (uint64_t)r->src[r->ip++] << r->bits;
        else r->padded += 8;
        r->bits += 8;
    }
}

/* a decode has used padding once fewer bits are left than were padded in; once true it stays true until a stored block resets the reader */
FFHIP_INF_FN int ffhip_inf_overrun(const ffhip_inf_state *r) { return r->bits < r->padded; }
FFHIP_INF_FN uint32_t ffhip_inf_peek(const ffhip_inf_state *r, int n) { return (uint32_t)(r->hold & ((1ull << n) - 1)); }
FFHIP_INF_FN void ffhip_inf_drop(ffhip_inf_state *r, int n) { r->hold >>= n; r->bits -= n; }
FFHIP_INF_FN uint32_t ffhip_inf_take(ffhip_inf_state *r, int n)
{
    const uint32_t v = ffhip_inf_peek(r, n);
    ffhip_inf_drop(r, n);
    return v;
}

/* a turn of a loop that consumes input: 0, or FFHIP_INF_EINVAL beyond the cap */
FFHIP_INF_FN int ffhip_inf_turn(ffhip_inf_state *r) { return ++r->turns > r->max_turns ? FFHIP_INF_EINVAL : 0; }

/* lengths[0 .. n) -> table, as ffhip_inflate.c's build_table: over-subscribed lengths are refused; an incomplete set only where
 * `single_ok` and it is one code of one bit, or no code at all */
FFHIP_INF_FN int ffhip_inf_build(ffhip_inf_table *t, uint16_t *offs, const uint8_t *lengths, int n, int single_ok)
{
    for (int l = 0; l <= FFHIP_INF_MAXBITS; l++) t->count[l] = 0;
    for (int i = 0; i < n; i++) t->count[lengths[i]]++;
    t->count[0] = 0;
    int left = 1, total = 0;
    for (int l = 1; l <= FFHIP_INF_MAXBITS; l++) {
        left = (left << 1) - t->count[l];
        if (left < 0) return FFHIP_INF_EINVAL;
        total += t->count[l];
    }
    if (left > 0 && !(single_ok && (total == 0 || (total == 1 && t->count[1] == 1)))) return FFHIP_INF_EINVAL;
    offs[1] = 0;
    for (int l = 1; l <= FFHIP_INF_MAXBITS; l++) offs[l + 1] = (uint16_t)(offs[l] + t->count[l]);
    for (int i = 0; i < n; i++)
        if (lengths[i]) t->symbol[offs[lengths[i]]++] = (uint16_t)i;
    for (int i = 0; i < (1 << FFHIP_INF_PRIMARY); i++) t->fast[i] = 0;
    uint32_t code = 0;
    int at = 0;
    for (int l = 1; l <= FFHIP_INF_PRIMARY; l++) {
        const int cnt = t->count[l];
        for (int k = 0; k < cnt; k++, code++, at++) {
            uint32_t rev = 0;
            for (int b = 0; b < l; b++) rev |= ((code >> b) & 1) << (l - 1 - b);
            const uint16_t e = (uint16_t)(t->symbol[at] << 4 | l);
            for (uint32_t i = rev; i < (1u << FFHIP_INF_PRIMARY); i += 1u << l) t->fast[i] = e;
        }
        code <<= 1;
    }
    return 0;
}

/* the next symbol, or -1 for a bit pattern that is no code of the table */
FFHIP_INF_FN int ffhip_inf_decode(ffhip_inf_state *r, const ffhip_inf_table *t)
{
    const uint16_t e = t->fast[ffhip_inf_peek(r, FFHIP_INF_PRIMARY)];
    if (e) {
        ffhip_inf_drop(r, e & 15);
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t h = r->hold;
    for (int l = 1; l <= FFHIP_INF_MAXBITS; l++) {
        code |= (uint32_t)(h & 1);
        h >>= 1;
        const uint32_t cnt = t->count[l];
        if (code - first < cnt) {
            ffhip_inf_drop(r, l);
            return t->symbol[index + (code - first)];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

/* RFC 1951's tables as arithmetic: no constant array for the two compilers to place */
FFHIP_INF_FN uint32_t ffhip_inf_len_extra(int s) { return s < 8 || s == 28 ? 0u : (uint32_t)(s >> 2) - 1; }
FFHIP_INF_FN uint32_t ffhip_inf_len_base(int s) { return s < 8 ? 3u + (uint32_t)s : s == 28 ? 258u : 3u + ((4u + ((uint32_t)s & 3)) << ((s >> 2) - 1)); }
FFHIP_INF_FN uint32_t ffhip_inf_dist_extra(int d) { return d < 4 ? 0u : (uint32_t)(d >> 1) - 1; }
FFHIP_INF_FN uint32_t ffhip_inf_dist_base(int d) { return d < 4 ? 1u + (uint32_t)d : 1u + ((2u + ((uint32_t)d & 1)) << ((d >> 1) - 1)); }
/* 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15: five bits each, twelve in the first word */
FFHIP_INF_FN int ffhip_inf_clen_order(int i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

FFHIP_INF_FN int ffhip_inf_dynamic_tables(ffhip_inf_state *r, ffhip_inf_store *m)
{
    ffhip_inf_refill(r);
    const int hlit = (int)ffhip_inf_take(r, 5) + 257, hdist = (int)ffhip_inf_take(r, 5) + 1, hclen = (int)ffhip_inf_take(r, 4) + 4;
    if (hlit > 286 || hdist > 30) return FFHIP_INF_EINVAL;
    uint8_t *lengths = m->lengths;
    for (int i = 0; i < 19; i++) lengths[i] = 0;
    for (int i = 0; i < hclen; i++) { /* 19 turns at the most, three bits each */
        if (r->bits < 3) ffhip_inf_refill(r);
        lengths[ffhip_inf_clen_order(i)] = (uint8_t)ffhip_inf_take(r, 3);
    }
    ffhip_inf_table *clen = &m->dist;
    if (ffhip_inf_overrun(r) || ffhip_inf_build(clen, m->offs, lengths, 19, 0)) return FFHIP_INF_EINVAL;
    int n = 0;
    while (n < hlit + hdist) { /* a turn takes a code of at least one bit, or ends the stream */
        if (ffhip_inf_turn(r)) return FFHIP_INF_EINVAL;
        ffhip_inf_refill(r);
        const int s = ffhip_inf_decode(r, clen);
        if (s < 0 || ffhip_inf_overrun(r)) return FFHIP_INF_EINVAL;
        if (s < 16) { lengths[n++] = (uint8_t)s; continue; }
        int prev = 0, rep;
        if (s == 16) {
            if (n == 0) return FFHIP_INF_EINVAL;
            prev = lengths[n - 1];
            rep = 3 + (int)ffhip_inf_take(r, 2);
        } else if (s == 17) {
            rep = 3 + (int)ffhip_inf_take(r, 3);
        } else {
            rep = 11 + (int)ffhip_inf_take(r, 7);
        }
        if (n + rep > hlit + hdist) return FFHIP_INF_EINVAL;
        while (rep--) lengths[n++] = (uint8_t)prev;
    }
    if (ffhip_inf_overrun(r) || lengths[256] == 0) return FFHIP_INF_EINVAL; /* no end-of-block code */
    if (ffhip_inf_build(&m->lit, m->offs, lengths, hlit, 0)) return FFHIP_INF_EINVAL;
    return ffhip_inf_build(&m->dist, m->offs, lengths + hlit, hdist, 1);
}

FFHIP_INF_FN void ffhip_inf_fixed_tables(ffhip_inf_store *m)
{
    uint8_t *lengths = m->lengths;
    for (int i = 0; i < 288; i++) lengths[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    (void)ffhip_inf_build(&m->lit, m->offs, lengths, 288, 0);
    for (int i = 0; i < 32; i++) lengths[i] = 5;
    (void)ffhip_inf_build(&m->dist, m->offs, lengths, 32, 0);
}

/* the zlib header, as ffhip_inflate_upto checks it.  cap: the most output; partial: output beyond cap ends the decode with success */
FFHIP_INF_FN int ffhip_inf_begin(ffhip_inf_state *r, const uint8_t *src, uint64_t len, uint64_t cap, int partial)
{
    r->src = src;
    r->ip = 2;
    r->end = len;
    r->hold = 0;
    r->bits = r->padded = 0;
    r->at = 0;
    r->cap = cap;
    r->turns = 0;
    r->max_turns = 8 * len + 64;
    r->stored_from = 0;
    r->stored_left = 0;
    r->partial = partial;
    r->where = FFHIP_INF_AT_HEADER;
    r->last = r->full = r->done = 0;
    r->out_len = 0;
    r->want = 0;
    if (len < 2) return FFHIP_INF_EINVAL;
    /* CMF, FLG: deflate with a window of up to 32 KiB, the check bits, no preset dictionary */
    if ((src[0] & 15) != 8 || (src[0] >> 4) > 7 || ((src[0] << 8 | src[1]) % 31) != 0 || (src[1] & 0x20)) return FFHIP_INF_EINVAL;
    return 0;
}

/* The next batch: the number of steps laid into m->step[], 0 included, or FFHIP_INF_EINVAL.  Once r->done the stream has ended behind
 * these steps: r->out_len is the output's length and, unless r->full, r->want the check value the finished output has to give.
 * Call it until r->done; a call that returns without r->done has laid at least one step. */
FFHIP_INF_FN int ffhip_inf_batch(ffhip_inf_state *r, ffhip_inf_store *m)
{
    int n_steps = 0, n_tok = 0;
    for (;;) {
        /* invariant (1): a turn below reads a block header (3 bits), a stored step (64 bytes, or the block's rest), or a token (a code of
         * at least one bit) -- or it ends the stream.  Invariant (2): every one of them checks the overrun before it goes on. */
        if (r->where == FFHIP_INF_AT_HEADER) {
            if (r->last || r->full) { /* the end: the check value, unless the caller wanted no more than this */
                r->done = 1;
                r->out_len = r->at;
                if (r->full) return n_steps;
                ffhip_inf_drop(r, r->bits & 7);
                if (r->bits < 32) ffhip_inf_refill(r);
                uint32_t want = 0;
                for (int k = 0; k < 4; k++) want = want << 8 | ffhip_inf_take(r, 8);
                r->want = want;
                return ffhip_inf_overrun(r) ? FFHIP_INF_EINVAL : n_steps;
            }
            if (ffhip_inf_turn(r)) return FFHIP_INF_EINVAL;
            ffhip_inf_refill(r);
            r->last = (int)ffhip_inf_take(r, 1);
            const int type = (int)ffhip_inf_take(r, 2);
            if (ffhip_inf_overrun(r)) return FFHIP_INF_EINVAL;
            if (type == 0) {
                ffhip_inf_drop(r, r->bits & 7); /* to the byte boundary; what the reader holds beyond it goes back to the stream */
                if (r->bits < 32) ffhip_inf_refill(r);
                const uint32_t n = ffhip_inf_take(r, 16), nn = ffhip_inf_take(r, 16);
                if (ffhip_inf_overrun(r) || (n ^ nn) != 0xffff) return FFHIP_INF_EINVAL;
                const uint64_t p = r->ip - (uint64_t)((r->bits - r->padded) / 8); /* the first byte the reader has not handed out */
                if (r->end - p < n) return FFHIP_INF_EINVAL;
                uint32_t take = n;
                if (take > r->cap - r->at) {
                    if (!r->partial) return FFHIP_INF_EINVAL;
                    take = (uint32_t)(r->cap - r->at);
                    r->full = 1;
                }
                r->stored_from = p;
                r->stored_left = take;
                r->ip = p + n;
                r->hold = 0;
                r->bits = r->padded = 0;
                r->where = FFHIP_INF_IN_STORED;
            } else if (type == 1) {
                ffhip_inf_fixed_tables(m);
                r->where = FFHIP_INF_IN_CODES;
            } else if (type == 2) {
                if (ffhip_inf_dynamic_tables(r, m)) return FFHIP_INF_EINVAL;
                r->where = FFHIP_INF_IN_CODES;
            } else {
                return FFHIP_INF_EINVAL;
            }
            continue;
        }
        if (n_tok >= FFHIP_INF_TOKENS || n_steps + 5 > FFHIP_INF_STEPS) return n_steps; /* the batch is full */
        if (r->where == FFHIP_INF_IN_STORED) {
            if (!r->stored_left) { r->where = FFHIP_INF_AT_HEADER; continue; }
            if (ffhip_inf_turn(r)) return FFHIP_INF_EINVAL;
            ffhip_inf_step *s = &m->step[n_steps++];
            const uint32_t n = r->stored_left < FFHIP_INF_LANES ? r->stored_left : FFHIP_INF_LANES;
            s->to = r->at;
            s->from = r->stored_from;
            s->dist = 0;
            s->n = (uint16_t)n;
            s->kind = FFHIP_INF_STORED;
            r->at += n;
            r->stored_from += n;
            r->stored_left -= n;
            continue;
        }
        /* a token */
        if (ffhip_inf_turn(r)) return FFHIP_INF_EINVAL;
        ffhip_inf_refill(r); /* >= 56 bits: a literal/length code, its extra bits, a distance code and its extra bits are at most 48 */
        int sym = ffhip_inf_decode(r, &m->lit);
        if (sym < 0 || ffhip_inf_overrun(r)) return FFHIP_INF_EINVAL;
        if (sym < 256) {
            if (r->at == r->cap) {
                if (!r->partial) return FFHIP_INF_EINVAL;
                r->full = 1;
                r->where = FFHIP_INF_AT_HEADER;
                continue;
            }
            ffhip_inf_step *s = n_steps ? &m->step[n_steps - 1] : (ffhip_inf_step *)0;
            if (!s || s->kind != FFHIP_INF_LITERALS) { /* a new run; a run's literals are tokens of this batch, 64 at the most */
                s = &m->step[n_steps++];
                s->to = r->at;
                s->from = (uint64_t)n_tok;
                s->dist = 0;
                s->n = 0;
                s->kind = FFHIP_INF_LITERALS;
            }
            m->lit_byte[n_tok++] = (uint8_t)sym;
            s->n++;
            r->at++;
            continue;
        }
        if (sym == 256) { r->where = FFHIP_INF_AT_HEADER; continue; }
        sym -= 257;
        if (sym >= 29) return FFHIP_INF_EINVAL; /* symbols 286 and 287 */
        uint64_t n = ffhip_inf_len_base(sym) + ffhip_inf_take(r, (int)ffhip_inf_len_extra(sym));
        const int d = ffhip_inf_decode(r, &m->dist);
        if (d < 0 || d >= 30) return FFHIP_INF_EINVAL; /* no such code; symbols 30 and 31 */
        const uint64_t back = ffhip_inf_dist_base(d) + ffhip_inf_take(r, (int)ffhip_inf_dist_extra(d));
        if (ffhip_inf_overrun(r) || back > r->at) return FFHIP_INF_EINVAL; /* before the start of the output */
        if (n > r->cap - r->at) {
            if (!r->partial) return FFHIP_INF_EINVAL;
            n = r->cap - r->at;
            r->full = 1;
            r->where = FFHIP_INF_AT_HEADER;
        }
        n_tok++;
        for (uint64_t k0 = 0; k0 < n; k0 += FFHIP_INF_LANES) { /* five steps at the most: n <= 258 */
            ffhip_inf_step *s = &m->step[n_steps++];
            s->to = r->at + k0;
            s->from = k0;
            s->dist = (uint32_t)back;
            s->n = (uint16_t)(n - k0 < FFHIP_INF_LANES ? n - k0 : FFHIP_INF_LANES);
            s->kind = FFHIP_INF_MATCH;
        }
        r->at += n;
    }
}

/* the writer, lane `lane` of step *s: its byte, if it has one.  A match's source lies in front of the match (s->to - s->from) */
FFHIP_INF_FN int ffhip_inf_step_load(const ffhip_inf_step *s, const ffhip_inf_store *m, const uint8_t *src, const uint8_t *dst, int lane, uint8_t *v)
{
    if (lane >= (int)s->n) return 0;
    if (s->kind == FFHIP_INF_LITERALS) {
        *v = m->lit_byte[s->from + (uint64_t)lane];
    } else if (s->kind == FFHIP_INF_STORED) {
        *v = src[s->from + (uint64_t)lane];
    } else {
        uint32_t i = (uint32_t)s->from + (uint32_t)lane; /* below 258 + 64 */
        if (i >= s->dist) i %= s->dist;
        *v = dst[s->to - s->from - s->dist + i];
    }
    return 1;
}

FFHIP_INF_FN void ffhip_inf_step_store(const ffhip_inf_step *s, uint8_t *dst, int lane, uint8_t v) { dst[s->to + (uint64_t)lane] = v; }

/* whether the stores of earlier steps have to be visible to this step's loads: a match's first step (its later steps read in front of
 * the match as well, and the match's own stores lie behind that) */
FFHIP_INF_FN int ffhip_inf_step_reads_output(const ffhip_inf_step *s) { return s->kind == FFHIP_INF_MATCH && s->from == 0; }

/* Adler-32 by the wave, in blocks of up to FFHIP_INF_ADLER_BLOCK bytes: lane `lane`'s share of block p[0 .. m) -- *s1 the sum of its
 * bytes, *s2 the sum of (m - i) x byte i -- and the fold of a block's sums over all lanes into the running (a, b).  No sum leaves 32
 * bits: s2 <= 255 x 4096 x 4097 / 2, m x a < 4096 x 65521 */
#define FFHIP_INF_ADLER_BLOCK 4096u
FFHIP_INF_FN void ffhip_inf_adler_lane(const uint8_t *p, uint32_t m, int lane, uint32_t *s1, uint32_t *s2)
{
    uint32_t a = 0, b = 0;
    for (uint32_t i = (uint32_t)lane; i < m; i += FFHIP_INF_LANES) {
        const uint32_t v = p[i];
        a += v;
        b += (m - i) * v;
    }
    *s1 = a;
    *s2 = b;
}
FFHIP_INF_FN void ffhip_inf_adler_fold(uint32_t *a, uint32_t *b, uint32_t m, uint32_t s1, uint32_t s2)
{
    *b = (*b + m * *a + s2) % 65521u;
    *a = (*a + s1) % 65521u;
}

#endif
