/*
 * ffhip_inflate.c -- inflate of a zlib-wrapped deflate stream (RFC 1950, RFC 1951), for the PNG file calls.  Plain C11,
 * host only, no HIP and no zlib: the library links nothing but HIP, -ldl and -lpthread.
 *
 * Huffman codes are decoded through a look-up table indexed by the next INFLATE_PRIMARY bits of the stream (deflate packs codes starting
 * at the least significant bit, so a table index is the code bit-reversed): an entry holds the symbol and its length.  A code longer than
 * the table's index is rare by construction (long codes are improbable symbols) and takes the canonical walk over the count table.
 *
 * The reader holds up to 64 bits.  Beyond the last byte it feeds zero bytes and counts them: a decode that consumed one of those bits has
 * run off the end of the stream and is refused, so no symbol is ever taken from bytes the caller did not give.  Nothing outside
 * src[0 .. len) is read and nothing outside dst[0 .. cap) is written.
 */
#include "ffpic_hip.h"
#include "ffhip_png_internal.h"

#include <string.h>

#define INFLATE_PRIMARY 10
#define INFLATE_MAXBITS 15

typedef struct {
    uint16_t fast[1 << INFLATE_PRIMARY]; /* symbol << 4 | length; 0: no code of up to INFLATE_PRIMARY bits starts like this */
    uint16_t count[INFLATE_MAXBITS + 1]; /* codes of each length */
    uint16_t symbol[288];                /* symbols in canonical order */
} huff_table;

typedef struct {
    const uint8_t *ip, *end;
    uint64_t hold;
    int bits;   /* valid bits in hold, zero padding included */
    int padded; /* zero BITS fed beyond the end */
} bit_reader;

static inline void refill(bit_reader *r)
{
    if (r->end - r->ip >= 8) {
        uint64_t v;
        memcpy(&v, r->ip, 8); /* little-endian hosts only, as the rest of the library */
        r->hold |= v << r->bits;
        r->ip += (63 - r->bits) >> 3;
        r->bits |= 56;
        return;
    }
    while (r->bits <= 56) {
        if (r->ip < r->end) r->hold |= (uint64_t)*r->ip++ << r->bits;
        else r->padded += 8;
        r->bits += 8;
    }
}

/* a decode has used padding once fewer bits are left than were padded in */
static int overrun(const bit_reader *r) { return r->bits < r->padded; }
static uint32_t peek(const bit_reader *r, int n) { return (uint32_t)(r->hold & ((1ull << n) - 1)); }
static void drop(bit_reader *r, int n) { r->hold >>= n; r->bits -= n; }
static uint32_t take(bit_reader *r, int n)
{
    const uint32_t v = peek(r, n);
    drop(r, n);
    return v;
}

/* lengths[0 .. n) -> table.  Over-subscribed lengths are refused; an incomplete set only where `single_ok` and it is one code of one bit
 * (the distance tree of a block with one distance, as zlib accepts it), or no code at all (a block of literals) */
static int build_table(huff_table *t, const uint8_t *lengths, int n, int single_ok)
{
    uint16_t offs[INFLATE_MAXBITS + 2];
    memset(t->count, 0, sizeof(t->count));
    for (int i = 0; i < n; i++) t->count[lengths[i]]++;
    t->count[0] = 0;
    int left = 1, total = 0;
    for (int l = 1; l <= INFLATE_MAXBITS; l++) {
        left = (left << 1) - t->count[l];
        if (left < 0) return FFHIP_EINVAL;
        total += t->count[l];
    }
    if (left > 0 && !(single_ok && (total == 0 || (total == 1 && t->count[1] == 1)))) return FFHIP_EINVAL;
    offs[1] = 0;
    for (int l = 1; l <= INFLATE_MAXBITS; l++) offs[l + 1] = (uint16_t)(offs[l] + t->count[l]);
    for (int i = 0; i < n; i++)
        if (lengths[i]) t->symbol[offs[lengths[i]]++] = (uint16_t)i;
    memset(t->fast, 0, sizeof(t->fast));
    uint32_t code = 0;
    int at = 0;
    for (int l = 1; l <= INFLATE_PRIMARY; l++) {
        for (int k = 0; k < t->count[l]; k++, code++, at++) {
            uint32_t rev = 0;
            for (int b = 0; b < l; b++) rev |= ((code >> b) & 1) << (l - 1 - b);
            const uint16_t e = (uint16_t)(t->symbol[at] << 4 | l);
            for (uint32_t i = rev; i < (1u << INFLATE_PRIMARY); i += 1u << l) t->fast[i] = e;
        }
        code <<= 1;
    }
    return FFHIP_OK;
}

/* the next symbol, or -1 for a bit pattern that is no code of the table */
static inline int decode(bit_reader *r, const huff_table *t)
{
    const uint16_t e = t->fast[peek(r, INFLATE_PRIMARY)];
    if (e) {
        drop(r, e & 15);
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t h = r->hold;
    for (int l = 1; l <= INFLATE_MAXBITS; l++) {
        code |= (uint32_t)(h & 1);
        h >>= 1;
        const uint32_t cnt = t->count[l];
        if (code - first < cnt) {
            drop(r, l);
            return t->symbol[index + (code - first)];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

static uint32_t adler32(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = n < 5552 ? n : 5552; /* the most bytes before b can leave 32 bits */
        n -= k;
        while (k--) { a += *p++; b += a; }
        a %= 65521;
        b %= 65521;
    }
    return b << 16 | a;
}

static int dynamic_tables(bit_reader *r, huff_table *lit, huff_table *dist, huff_table *clen)
{
    refill(r);
    const int hlit = (int)take(r, 5) + 257, hdist = (int)take(r, 5) + 1, hclen = (int)take(r, 4) + 4;
    if (hlit > 286 || hdist > 30) return FFHIP_EINVAL;
    uint8_t lengths[320];
    memset(lengths, 0, 19);
    for (int i = 0; i < hclen; i++) {
        if (r->bits < 3) refill(r);
        lengths[clen_order[i]] = (uint8_t)take(r, 3);
    }
    if (overrun(r) || build_table(clen, lengths, 19, 0)) return FFHIP_EINVAL;
    int n = 0;
    while (n < hlit + hdist) {
        refill(r);
        const int s = decode(r, clen);
        if (s < 0 || overrun(r)) return FFHIP_EINVAL;
        if (s < 16) { lengths[n++] = (uint8_t)s; continue; }
        int prev = 0, rep;
        if (s == 16) {
            if (n == 0) return FFHIP_EINVAL;
            prev = lengths[n - 1];
            rep = 3 + (int)take(r, 2);
        } else if (s == 17) {
            rep = 3 + (int)take(r, 3);
        } else {
            rep = 11 + (int)take(r, 7);
        }
        if (n + rep > hlit + hdist) return FFHIP_EINVAL;
        while (rep--) lengths[n++] = (uint8_t)prev;
    }
    if (overrun(r) || lengths[256] == 0) return FFHIP_EINVAL; /* no end-of-block code */
    if (build_table(lit, lengths, hlit, 0)) return FFHIP_EINVAL;
    return build_table(dist, lengths + hlit, hdist, 1);
}

static void fixed_tables(huff_table *lit, huff_table *dist)
{
    uint8_t lengths[288];
    for (int i = 0; i < 288; i++) lengths[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    build_table(lit, lengths, 288, 0);
    memset(lengths, 5, 32);
    build_table(dist, lengths, 32, 0);
}

/* one block of codes.  Returns FFHIP_OK at its end-of-block, 1 where `partial` and the output is full */
static int coded_block(bit_reader *r, const huff_table *lit, const huff_table *dist, uint8_t *dst, size_t cap, size_t *pos, int partial)
{
    size_t at = *pos;
    for (;;) {
        refill(r); /* >= 56 bits: a literal/length code, its extra bits, a distance code and its extra bits are at most 48 */
        int s = decode(r, lit);
        if (s < 0 || overrun(r)) return FFHIP_EINVAL;
        if (s < 256) {
            if (at == cap) { *pos = at; return partial ? 1 : FFHIP_EINVAL; }
            dst[at++] = (uint8_t)s;
            /* literals come in runs: up to two more out of the bits already here (15 + 10 + 10 of at least 56), table codes only.  One that
             * was made of padding is found out by the check above at the next turn; its byte lies inside dst[0 .. cap) */
            for (int k = 0; k < 2; k++) {
                const uint16_t e = lit->fast[peek(r, INFLATE_PRIMARY)];
                if (!e || e >= (256 << 4) || at == cap) break;
                drop(r, e & 15);
                dst[at++] = (uint8_t)(e >> 4);
            }
            continue;
        }
        if (s == 256) { *pos = at; return FFHIP_OK; }
        s -= 257;
        if (s >= 29) return FFHIP_EINVAL; /* symbols 286 and 287 */
        size_t n = len_base[s] + take(r, len_extra[s]);
        const int d = decode(r, dist);
        if (d < 0 || d >= 30) return FFHIP_EINVAL; /* no such code; symbols 30 and 31 */
        const size_t back = dist_base[d] + take(r, dist_extra[d]);
        if (overrun(r) || back > at) return FFHIP_EINVAL; /* before the start of the output */
        int full = 0;
        if (n > cap - at) {
            if (!partial) return FFHIP_EINVAL;
            n = cap - at;
            full = 1;
        }
        uint8_t *to = dst + at;
        const uint8_t *from = to - back;
        if (back >= 8 && cap - at >= n + 8) { /* eight bytes at a time, up to seven beyond the match but inside the output */
            for (size_t k = 0; k < n; k += 8) memcpy(to + k, from + k, 8);
        } else if (back >= n) {
            memcpy(to, from, n);
        } else if (back == 1) {
            memset(to, from[0], n);
        } else {
            for (size_t k = 0; k < n; k++) to[k] = from[k]; /* the copy overlaps itself on purpose */
        }
        at += n;
        if (full) { *pos = at; return 1; }
    }
}

int ffhip_inflate_upto(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial)
{
    if (!src || (!dst && cap) || !out_len) return FFHIP_EINVAL;
    *out_len = 0;
    if (len < 2) return FFHIP_EINVAL;
    /* CMF, FLG: deflate with a window of up to 32 KiB, the check bits, no preset dictionary */
    if ((src[0] & 15) != 8 || (src[0] >> 4) > 7 || ((src[0] << 8 | src[1]) % 31) != 0 || (src[1] & 0x20)) return FFHIP_EINVAL;
    bit_reader r = {src + 2, src + len, 0, 0, 0};
    static _Thread_local huff_table lit, dist, clen;
    size_t at = 0;
    int last, full = 0;
    do {
        refill(&r);
        last = (int)take(&r, 1);
        const int type = (int)take(&r, 2);
        if (overrun(&r)) return FFHIP_EINVAL;
        if (type == 0) {
            drop(&r, r.bits & 7); /* to the byte boundary; what the reader holds beyond it goes back to the stream */
            if (r.bits < 32) refill(&r);
            const uint32_t n = take(&r, 16), nn = take(&r, 16);
            if (overrun(&r) || (n ^ nn) != 0xffff) return FFHIP_EINVAL;
            const uint8_t *p = r.ip - (r.bits - r.padded) / 8; /* the first byte the reader has not handed out */
            if ((size_t)(r.end - p) < n) return FFHIP_EINVAL;
            size_t m = n;
            if (m > cap - at) {
                if (!partial) return FFHIP_EINVAL;
                m = cap - at;
                full = 1;
            }
            if (m) memcpy(dst + at, p, m);
            at += m;
            r.ip = p + n;
            r.hold = 0;
            r.bits = r.padded = 0;
        } else if (type == 1 || type == 2) {
            if (type == 1) fixed_tables(&lit, &dist);
            else if (dynamic_tables(&r, &lit, &dist, &clen)) return FFHIP_EINVAL;
            const int rc = coded_block(&r, &lit, &dist, dst, cap, &at, partial);
            if (rc < 0) return rc;
            full = rc;
        } else {
            return FFHIP_EINVAL;
        }
    } while (!last && !full);
    *out_len = at;
    if (full) return FFHIP_OK; /* the caller wanted no more than this: what follows, the check value included, is not looked at */
    drop(&r, r.bits & 7);
    if (r.bits < 32) refill(&r);
    uint32_t want = 0;
    for (int k = 0; k < 4; k++) want = want << 8 | take(&r, 8);
    if (overrun(&r) || want != adler32(dst, at)) return FFHIP_EINVAL;
    return FFHIP_OK;
}

int ffhip_inflate(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len)
{
    return ffhip_inflate_upto(src, len, dst, cap, out_len, 0);
}
