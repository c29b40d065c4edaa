/*
 * ffhip_vp8l.c -- the host side of the lossless WebP calls (include/ffpic_hip.h, "lossless WebP"): the container walk, the
 * probe, the VP8L stream decoder (header, transform list with its sub-images, colour cache, meta prefix image and code groups, two-level
 * prefix tables, the LZ77 copy loop), and ffhip_vp8l_picture, the whole decode on the host with the functions of ffhip_vp8l_body.h that
 * the kernels compile too.  Plain C11, no HIP.
 *
 * Written from the rule in the header, which was settled against libwebp through PIL:
 *   stream   bits LSB first; prefix code words MSB first
 *   image    [colour cache: 1, 4 bits] [meta prefix image: 1, 3 bits, an image -- the picture only] 5 codes a group, then the pixels
 *   code     simple: 1 or 2 symbols of 1 or 8 bits; normal: 4..19 code-length code lengths of 3 bits, [max_symbol], the lengths
 * Every bit read is checked against the end of the chunk: bits behind it read as 0 and the image they were asked for is refused.
 * ffhip_vp8l_open_stream is the way in for a stream without container, signature and header: the ALPH chunk of a lossy file
 * (ffhip_webp_alpha.c), whose one exception to the line above is `lenient_end` (ffhip_vp8l_internal.h).
 */
#include "ffhip_vp8l_internal.h"

#include <stdlib.h>
#include <string.h>

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t rd24(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }
static int is4(const uint8_t *p, const char *tag) { return memcmp(p, tag, 4) == 0; }
static uint32_t subsample(uint32_t n, int bits) { return (n + (1u << bits) - 1) >> bits; }

/* ---- the container ---- */

/* the VP8L chunk's payload; canvas[2] the VP8X chunk's width and height, 0 without one */
static int vp8l_container(const uint8_t *file, size_t len, const uint8_t **body, size_t *body_len, uint32_t canvas[2])
{
    canvas[0] = canvas[1] = 0;
    if (len < 12 || !is4(file, "RIFF") || !is4(file + 8, "WEBP")) return FFHIP_EINVAL;
    const uint32_t riff = rd32(file + 4);
    if (riff < 4 || riff > len - 8) return FFHIP_EINVAL;
    const size_t end = (size_t)riff + 8;
    size_t pos = 12;
    while (end - pos >= 8) {
        const uint8_t *c = file + pos;
        const uint32_t size = rd32(c + 4);
        if (size > end - pos - 8) return FFHIP_EINVAL;
        if (is4(c, "VP8X")) {
            if (size != 10 || pos != 12) return FFHIP_EINVAL;
            if (c[8] & 2) return FFHIP_EWEBP_ANIMATION;
            canvas[0] = rd24(c + 12) + 1;
            canvas[1] = rd24(c + 15) + 1;
        } else if (is4(c, "ANIM") || is4(c, "ANMF")) {
            return FFHIP_EWEBP_ANIMATION;
        } else if (is4(c, "VP8 ")) {
            return FFHIP_EINVAL;
        } else if (is4(c, "VP8L")) {
            *body = c + 8;
            *body_len = size;
            return FFHIP_OK;
        }
        const size_t step = 8 + (size_t)size + (size & 1);
        if (step > end - pos) break; /* the padding byte of the last chunk is missing */
        pos += step;
    }
    return FFHIP_EINVAL;
}

static int vp8l_header(const uint8_t *file, size_t len, const uint8_t **body, size_t *body_len, ffhip_vp8l_info *info)
{
    uint32_t canvas[2];
    const int rc = vp8l_container(file, len, body, body_len, canvas);
    if (rc) return rc;
    const uint8_t *b = *body;
    if (*body_len < 5 || b[0] != 0x2f) return FFHIP_EINVAL;
    const uint32_t v = rd32(b + 1);
    if (v >> 29) return FFHIP_EINVAL; /* the version */
    info->width = (int32_t)(v & 0x3fff) + 1;
    info->height = (int32_t)((v >> 14) & 0x3fff) + 1;
    info->has_alpha = (int32_t)((v >> 28) & 1);
    if (canvas[0] && (canvas[0] != (uint32_t)info->width || canvas[1] != (uint32_t)info->height)) return FFHIP_EINVAL;
    return FFHIP_OK;
}

int ffhip_vp8l_probe(const uint8_t *file, size_t len, int *width, int *height, int *has_alpha)
{
    if (!file || !width || !height || !has_alpha) return FFHIP_EINVAL;
    ffhip_vp8l_info info;
    const uint8_t *body;
    size_t body_len;
    memset(&info, 0, sizeof(info));
    const int rc = vp8l_header(file, len, &body, &body_len, &info);
    *width = rc ? 0 : info.width;
    *height = rc ? 0 : info.height;
    *has_alpha = rc ? 0 : info.has_alpha;
    return rc;
}

/* ---- bits ---- */

typedef struct bits {
    const uint8_t *p;
    size_t len;
    uint64_t pos; /* in bits */
} bits;

/* the next 32 bits at least, without taking them */
static inline uint64_t bits_peek(const bits *b)
{
    const size_t at = (size_t)(b->pos >> 3);
    uint64_t w = 0;
    if (b->len >= 8 && at <= b->len - 8) {
        memcpy(&w, b->p + at, 8); /* little-endian hosts: the library's only kind */
    } else {
        for (size_t k = 0; k < 8 && at < b->len && k < b->len - at; k++) w |= (uint64_t)b->p[at + k] << (8 * k);
    }
    return w >> (b->pos & 7);
}
static inline uint32_t bits_read(bits *b, int n) /* n <= 32 */
{
    const uint32_t v = (uint32_t)(bits_peek(b) & ((1ull << n) - 1));
    b->pos += (uint64_t)n;
    return v;
}
static inline int bits_over(const bits *b) { return b->pos > 8ull * b->len; }

/* ---- prefix codes: a root table of 8 bits, second-level tables behind it for the longer codes ---- */

#define ROOT_BITS 8
typedef struct entry {
    uint16_t value; /* the symbol; of a root entry that points on: the second-level table's offset from the root */
    uint8_t bits;   /* what the entry takes of the stream; 16 + n: a second-level table of n bits */
    uint8_t pad;
} entry;

typedef struct tables {
    entry *e;
    size_t used, cap;
} tables;

typedef struct code {
    size_t root;    /* offset into tables.e */
    int32_t single; /* the one symbol of a code that reads no bits, else -1 */
} code;

static int tables_need(tables *t, size_t more)
{
    if (t->used + more <= t->cap) return FFHIP_OK;
    size_t cap = t->cap ? t->cap : 4096;
    while (cap < t->used + more) cap *= 2;
    entry *e = (entry *)realloc(t->e, cap * sizeof(entry));
    if (!e) return FFHIP_ENOMEM;
    t->e = e;
    t->cap = cap;
    return FFHIP_OK;
}

static uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int k = 0; k < n; k++) r |= ((v >> k) & 1u) << (n - 1 - k);
    return r;
}

/* lengths[0 .. n) -> a code.  One symbol: no table.  Otherwise the lengths must fill the code space exactly */
static int code_build(const uint8_t *lengths, int n, tables *t, code *out)
{
    int count[16] = {0}, used = 0, last = 0, max_len = 0;
    for (int s = 0; s < n; s++) {
        if (!lengths[s]) continue;
        count[lengths[s]]++;
        used++;
        last = s;
        if (lengths[s] > max_len) max_len = lengths[s];
    }
    out->root = 0;
    out->single = -1;
    if (used == 0) return FFHIP_EINVAL;
    if (used == 1) { out->single = last; return FFHIP_OK; }
    uint32_t space = 0, next[16] = {0}, c = 0;
    for (int l = 1; l <= 15; l++) {
        space += (uint32_t)count[l] << (15 - l);
        c = (c + (uint32_t)count[l - 1]) << 1;
        next[l] = c;
    }
    if (space != 1u << 15) return FFHIP_EINVAL;
    const int sub_bits = max_len > ROOT_BITS ? max_len - ROOT_BITS : 0;
    /* which root entries lead on: those a longer code's first 8 bits select.  Every second-level table has max_len - 8 bits */
    uint8_t lead[1 << ROOT_BITS];
    memset(lead, 0, sizeof(lead));
    size_t total = 1u << ROOT_BITS;
    if (sub_bits) {
        uint32_t probe[16];
        memcpy(probe, next, sizeof(probe));
        for (int s = 0; s < n; s++) {
            const int l = lengths[s];
            if (!l) continue;
            const uint32_t low = reverse_bits(probe[l]++, l) & ((1u << ROOT_BITS) - 1);
            if (l > ROOT_BITS && !lead[low]) { lead[low] = 1; total += (size_t)1 << sub_bits; }
        }
    }
    const int rc = tables_need(t, total);
    if (rc) return rc;
    entry *root = t->e + t->used;
    out->root = t->used;
    t->used += total;
    size_t at = 1u << ROOT_BITS;
    for (uint32_t low = 0; low < (1u << ROOT_BITS); low++) {
        if (!lead[low]) continue;
        root[low].value = (uint16_t)at; /* at most 256 + 255 * 128 */
        root[low].bits = (uint8_t)(16 + sub_bits);
        root[low].pad = 0;
        at += (size_t)1 << sub_bits;
    }
    for (int s = 0; s < n; s++) {
        const int l = lengths[s];
        if (!l) continue;
        const uint32_t rev = reverse_bits(next[l]++, l);
        if (l <= ROOT_BITS) {
            for (uint32_t i = rev; i < (1u << ROOT_BITS); i += 1u << l) { root[i].value = (uint16_t)s; root[i].bits = (uint8_t)l; root[i].pad = 0; }
        } else {
            entry *sub = root + root[rev & ((1u << ROOT_BITS) - 1)].value;
            for (uint32_t i = rev >> ROOT_BITS; i < (1u << sub_bits); i += 1u << (l - ROOT_BITS)) {
                sub[i].value = (uint16_t)s;
                sub[i].bits = (uint8_t)(l - ROOT_BITS);
                sub[i].pad = 0;
            }
        }
    }
    return FFHIP_OK;
}

static inline uint32_t code_read(const code *c, const entry *e, bits *b)
{
    if (c->single >= 0) return (uint32_t)c->single;
    const uint64_t w = bits_peek(b);
    const entry *root = e + c->root;
    entry x = root[w & ((1u << ROOT_BITS) - 1)];
    if (x.bits > 15) {
        b->pos += ROOT_BITS;
        x = root[x.value + ((w >> ROOT_BITS) & ((1u << (x.bits - 16)) - 1))];
    }
    b->pos += x.bits;
    return x.value;
}

static const uint8_t cl_order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
#define MAX_ALPHABET (256 + 24 + (1 << 11))

/* one code of the stream over `alphabet` symbols; lengths is MAX_ALPHABET bytes of the caller's */
static int code_parse(bits *b, int alphabet, uint8_t *lengths, tables *t, code *out)
{
    memset(lengths, 0, (size_t)(alphabet > 256 ? alphabet : 256));
    if (bits_read(b, 1)) {
        const int two = (int)bits_read(b, 1);
        lengths[bits_read(b, bits_read(b, 1) ? 8 : 1)] = 1;
        if (two) lengths[bits_read(b, 8)] = 1;
    } else {
        uint8_t cl[19] = {0};
        const int n_cl = (int)bits_read(b, 4) + 4;
        for (int k = 0; k < n_cl; k++) cl[cl_order[k]] = (uint8_t)bits_read(b, 3);
        tables small = {NULL, 0, 0};
        code clc;
        int rc = code_build(cl, 19, &small, &clc);
        if (rc) { free(small.e); return rc; }
        int limit = alphabet;
        if (bits_read(b, 1)) {
            const int nb = 2 + 2 * (int)bits_read(b, 3);
            limit = 2 + (int)bits_read(b, nb);
            if (limit > alphabet) rc = FFHIP_EINVAL;
        }
        int s = 0, prev = 8;
        while (!rc && s < alphabet && limit-- > 0) {
            const uint32_t c = code_read(&clc, small.e, b);
            if (c < 16) {
                lengths[s++] = (uint8_t)c;
                if (c) prev = (int)c;
                continue;
            }
            static const uint8_t extra[3] = {2, 3, 7}, base[3] = {3, 3, 11};
            const int rep = (int)bits_read(b, extra[c - 16]) + base[c - 16];
            if (s + rep > alphabet) { rc = FFHIP_EINVAL; break; }
            memset(lengths + s, c == 16 ? prev : 0, (size_t)rep);
            s += rep;
        }
        free(small.e);
        if (rc) return rc;
    }
    if (bits_over(b)) return FFHIP_EINVAL;
    return code_build(lengths, alphabet, t, out);
}

/* ---- an entropy-coded image ---- */

static const int8_t short_codes[120][2] = {
    {0, 1}, {1, 0}, {1, 1}, {-1, 1}, {0, 2}, {2, 0}, {1, 2}, {-1, 2}, {2, 1}, {-2, 1}, {2, 2}, {-2, 2}, {0, 3}, {3, 0}, {1, 3}, {-1, 3}, {3, 1}, {-3, 1},
    {2, 3}, {-2, 3}, {3, 2}, {-3, 2}, {0, 4}, {4, 0}, {1, 4}, {-1, 4}, {4, 1}, {-4, 1}, {3, 3}, {-3, 3}, {2, 4}, {-2, 4}, {4, 2}, {-4, 2}, {0, 5}, {3, 4},
    {-3, 4}, {4, 3}, {-4, 3}, {5, 0}, {1, 5}, {-1, 5}, {5, 1}, {-5, 1}, {2, 5}, {-2, 5}, {5, 2}, {-5, 2}, {4, 4}, {-4, 4}, {3, 5}, {-3, 5}, {5, 3}, {-5, 3},
    {0, 6}, {6, 0}, {1, 6}, {-1, 6}, {6, 1}, {-6, 1}, {2, 6}, {-2, 6}, {6, 2}, {-6, 2}, {4, 5}, {-4, 5}, {5, 4}, {-5, 4}, {3, 6}, {-3, 6}, {6, 3}, {-6, 3},
    {0, 7}, {7, 0}, {1, 7}, {-1, 7}, {5, 5}, {-5, 5}, {7, 1}, {-7, 1}, {4, 6}, {-4, 6}, {6, 4}, {-6, 4}, {2, 7}, {-2, 7}, {7, 2}, {-7, 2}, {3, 7}, {-3, 7},
    {7, 3}, {-7, 3}, {5, 6}, {-5, 6}, {6, 5}, {-6, 5}, {8, 0}, {4, 7}, {-4, 7}, {7, 4}, {-7, 4}, {8, 1}, {8, 2}, {6, 6}, {-6, 6}, {8, 3}, {5, 7}, {-5, 7},
    {7, 5}, {-7, 5}, {8, 4}, {6, 7}, {-6, 7}, {7, 6}, {-7, 6}, {8, 5}, {7, 7}, {-7, 7}, {8, 6}, {8, 7}};

static inline uint32_t prefix_value(bits *b, uint32_t p)
{
    if (p < 4) return p + 1;
    const int extra = (int)(p - 2) >> 1;
    return ((2 + (p & 1)) << extra) + bits_read(b, extra) + 1;
}

/* ---- the last token of a `lenient` image that ran over the chunk's end, read again as libwebp's reader reads there ----
 * That reader keeps the chunk's last 8 bytes in a 64-bit window and a position in it; at the end the position is 64.  A fetch takes the
 * window from (position mod 64) on, zeros above it: a symbol that straddles the end gets zeros, one that begins AT the end gets the last
 * 8 bytes again.  A read of extra bits, or a refill at position >= 32, that finds the position beyond 64 sets it to 0 and marks the end;
 * from then on extra bits read as 0 and every refill sets the position to 0 again. */
typedef struct tail {
    uint64_t win;
    unsigned pos;
    int eos;
} tail;

static void tail_fill(tail *t)
{
    if (t->pos >= 32 && (t->eos || t->pos > 64)) { t->eos = 1; t->pos = 0; }
}
static uint32_t tail_bits(tail *t, int n)
{
    if (t->eos) { t->pos = 0; return 0; }
    const uint32_t v = (uint32_t)((t->win >> (t->pos & 63)) & ((1ull << n) - 1));
    t->pos += (unsigned)n;
    if (t->pos > 64) { t->eos = 1; t->pos = 0; }
    return v;
}
static uint32_t tail_symbol(tail *t, const code *c, const entry *e)
{
    if (c->single >= 0) return (uint32_t)c->single;
    const entry *root = e + c->root;
    entry x = root[(t->win >> (t->pos & 63)) & ((1u << ROOT_BITS) - 1)];
    if (x.bits > 15) {
        t->pos += ROOT_BITS;
        x = root[x.value + ((t->win >> (t->pos & 63)) & ((1u << (x.bits - 16)) - 1))];
    }
    t->pos += x.bits;
    return x.value;
}
static uint32_t tail_prefix_value(tail *t, uint32_t p)
{
    if (p < 4) return p + 1;
    const int extra = (int)(p - 2) >> 1;
    return ((2 + (p & 1)) << extra) + tail_bits(t, extra) + 1;
}

/* the image header's two fields; *meta_bits 0 without a meta prefix image */
static int image_front(bits *b, int top, int *cache_bits, int *has_meta)
{
    *cache_bits = 0;
    *has_meta = 0;
    if (bits_read(b, 1)) {
        *cache_bits = (int)bits_read(b, 4);
        if (*cache_bits < 1 || *cache_bits > 11) return FFHIP_EINVAL;
    }
    if (top) *has_meta = (int)bits_read(b, 1);
    return FFHIP_OK;
}

/* w x h ARGB words into out.  top: the picture's own image, which may have a meta prefix image.  lenient: an image without a colour
 * cache whose red, blue and alpha codes all have one symbol may take the bits of its LAST token from behind the chunk's end */
static int image_read(bits *b, uint32_t w, uint32_t h, int top, int lenient, uint32_t *out)
{
    int cache_bits, has_meta, meta_bits = 0;
    int rc = image_front(b, top, &cache_bits, &has_meta);
    if (rc) return rc;
    uint32_t *meta = NULL, meta_w = 0, n_groups = 1;
    uint32_t *cache = NULL;
    code *codes = NULL;
    uint8_t *lengths = NULL;
    tables t = {NULL, 0, 0};
    if (has_meta) {
        meta_bits = (int)bits_read(b, 3) + 2;
        meta_w = subsample(w, meta_bits);
        const uint32_t meta_h = subsample(h, meta_bits);
        meta = (uint32_t *)malloc((size_t)meta_w * meta_h * 4);
        if (!meta) return FFHIP_ENOMEM;
        rc = image_read(b, meta_w, meta_h, 0, 0, meta);
        for (size_t k = 0; !rc && k < (size_t)meta_w * meta_h; k++) {
            meta[k] = (meta[k] >> 8) & 0xffffu;
            if (meta[k] >= n_groups) n_groups = meta[k] + 1;
        }
    }
    if (!rc && (!(codes = (code *)malloc((size_t)n_groups * 5 * sizeof(code))) || !(lengths = (uint8_t *)malloc(MAX_ALPHABET)) ||
                (cache_bits && !(cache = (uint32_t *)calloc((size_t)1 << cache_bits, 4)))))
        rc = FFHIP_ENOMEM;
    const int alphabet[5] = {256 + 24 + (cache_bits ? 1 << cache_bits : 0), 256, 256, 256, 40};
    for (uint32_t g = 0; !rc && g < n_groups; g++)
        for (int a = 0; !rc && a < 5; a++) rc = code_parse(b, alphabet[a], lengths, &t, &codes[5 * g + a]);
    if (cache_bits) lenient = 0;
    for (size_t k = 0; !rc && lenient && k < (size_t)n_groups; k++)
        if (codes[5 * k + 1].single < 0 || codes[5 * k + 2].single < 0 || codes[5 * k + 3].single < 0) lenient = 0;
    const uint64_t n = (uint64_t)w * h;
    uint64_t token_at = b->pos, token_i = 0; /* where the last token read began: in the stream, in the image */
    const code *token_grp = codes;
    const int cache_shift = 32 - cache_bits;
    const uint32_t meta_mask = has_meta ? (1u << meta_bits) - 1 : ~0u;
    const code *grp = codes;
    uint64_t i = 0;
    uint32_t x = 0, y = 0;
    while (!rc && i < n) {
        if (has_meta) grp = codes + 5 * (size_t)meta[(size_t)(y >> meta_bits) * meta_w + (x >> meta_bits)];
        /* up to the end of the group's block, or of the row */
        uint32_t run_end = has_meta ? ((x | meta_mask) + 1 < w ? (x | meta_mask) + 1 : w) : w;
        while (x < run_end) {
            token_at = b->pos;
            token_i = i;
            token_grp = grp;
            const uint32_t s = code_read(&grp[0], t.e, b);
            if (s < 256) {
                const uint32_t r = code_read(&grp[1], t.e, b), bl = code_read(&grp[2], t.e, b), al = code_read(&grp[3], t.e, b);
                const uint32_t v = al << 24 | r << 16 | s << 8 | bl;
                out[i++] = v;
                if (cache) cache[(0x1e35a7bdu * v) >> cache_shift] = v;
                x++;
            } else if (s < 256 + 24) {
                const uint32_t length = prefix_value(b, s - 256);
                uint32_t d = prefix_value(b, code_read(&grp[4], t.e, b));
                if (d > 120) {
                    d -= 120;
                } else {
                    const int64_t off = (int64_t)short_codes[d - 1][0] + (int64_t)short_codes[d - 1][1] * (int64_t)w;
                    d = off < 1 ? 1u : (uint32_t)off;
                }
                if ((uint64_t)d > i || (uint64_t)length > n - i) { rc = FFHIP_EINVAL; break; }
                for (uint32_t k = 0; k < length; k++, i++) {
                    const uint32_t v = out[i - d];
                    out[i] = v;
                    if (cache) cache[(0x1e35a7bdu * v) >> cache_shift] = v;
                }
                const uint64_t col = (uint64_t)x + length;
                y += (uint32_t)(col / w);
                x = (uint32_t)(col % w);
                break; /* the position has moved: its group again */
            } else { /* a cache hit; the alphabet ends with the cache */
                const uint32_t v = cache[s - 280];
                out[i++] = v;
                cache[(0x1e35a7bdu * v) >> cache_shift] = v;
                x++;
            }
        }
        if (x == w) { x = 0; y++; }
        if (bits_over(b) && i < n) rc = FFHIP_EINVAL; /* once a row or block: a cut stream is given up early */
    }
    if (!rc && bits_over(b) && !(lenient && token_at <= 8ull * b->len)) rc = FFHIP_EINVAL;
    if (!rc && bits_over(b) && b->len >= 8) { /* a shorter stream: zeros, as read above */
        tail r = {0, 64 - (unsigned)(8ull * b->len - token_at), 0};
        memcpy(&r.win, b->p + b->len - 8, 8);
        tail_fill(&r);
        const uint32_t s = tail_symbol(&r, &token_grp[0], t.e);
        if (s < 256) {
            if (token_i + 1 != n) rc = FFHIP_EINVAL; /* the end is marked now: pixels still to come are refused */
            out[token_i] = (uint32_t)token_grp[3].single << 24 | (uint32_t)token_grp[1].single << 16 | s << 8 | (uint32_t)token_grp[2].single;
        } else { /* a copy: the alphabet of an image without a cache ends with the length prefixes */
            const uint32_t length = tail_prefix_value(&r, s - 256);
            const uint32_t dsym = tail_symbol(&r, &token_grp[4], t.e);
            tail_fill(&r);
            uint32_t d = tail_prefix_value(&r, dsym);
            if (d > 120) {
                d -= 120;
            } else {
                const int64_t off = (int64_t)short_codes[d - 1][0] + (int64_t)short_codes[d - 1][1] * (int64_t)w;
                d = off < 1 ? 1u : (uint32_t)off;
            }
            if ((uint64_t)d > token_i || (uint64_t)length != n - token_i) rc = FFHIP_EINVAL;
            for (uint64_t k = token_i; !rc && k < token_i + length; k++) out[k] = out[k - d];
        }
    }
    free(meta);
    free(cache);
    free(codes);
    free(lengths);
    free(t.e);
    return rc;
}

/* ---- a file ---- */

void ffhip_vp8l_close(ffhip_vp8l_file *pf)
{
    if (!pf) return;
    free(pf->predictor_image);
    free(pf->cross_image);
    pf->predictor_image = pf->cross_image = NULL;
}

static int vp8l_bundle_bits(int colours) { return colours > 16 ? 0 : colours > 4 ? 1 : colours > 2 ? 2 : 3; }

int ffhip_vp8l_open(const uint8_t *file, size_t len, ffhip_vp8l_file *pf)
{
    if (!file || !pf) return FFHIP_EINVAL;
    memset(pf, 0, sizeof(*pf));
    const uint8_t *body;
    size_t body_len;
    ffhip_vp8l_info head;
    memset(&head, 0, sizeof(head));
    const int rc = vp8l_header(file, len, &body, &body_len, &head);
    if (rc) return rc;
    return ffhip_vp8l_open_stream(body + 5, body_len - 5, head.width, head.height, head.has_alpha, 0, pf);
}

int ffhip_vp8l_open_stream(const uint8_t *stream, size_t len, int32_t width, int32_t height, int32_t has_alpha, int alpha_plane, ffhip_vp8l_file *pf)
{
    if (!stream || !pf || width < 1 || height < 1 || width > 16384 || height > 16384) return FFHIP_EINVAL;
    memset(pf, 0, sizeof(*pf));
    ffhip_vp8l_info *info = &pf->info;
    info->width = width;
    info->height = height;
    info->has_alpha = has_alpha;
    int rc = FFHIP_OK;
    pf->stream = stream;
    pf->stream_len = len;
    bits b = {pf->stream, pf->stream_len, 0};
    const uint32_t h = (uint32_t)info->height;
    uint32_t xs = (uint32_t)info->width;
    unsigned seen = 0;
    info->pixels_per_word = 1;
    while (!rc && bits_read(&b, 1)) {
        const int type = (int)bits_read(&b, 2);
        if (seen & (1u << type)) { rc = FFHIP_EINVAL; break; }
        seen |= 1u << type;
        const int k = info->n_transforms++;
        info->transforms[k] = type;
        pf->xsize[k] = xs;
        if (type == FFHIP_VP8L_PREDICTOR || type == FFHIP_VP8L_CROSS_COLOR) {
            const int bb = (int)bits_read(&b, 3) + 2;
            const uint32_t bx = subsample(xs, bb), by = subsample(h, bb);
            uint32_t *img = (uint32_t *)malloc((size_t)bx * by * 4);
            if (!img) { rc = FFHIP_ENOMEM; break; }
            if (type == FFHIP_VP8L_PREDICTOR) {
                pf->predictor_image = img; pf->predictor_words = bx * by; info->predictor_bits = bb;
                pf->steps.predictor_bits = (uint8_t)bb; pf->steps.predictor_bx = bx;
            } else {
                pf->cross_image = img; pf->cross_words = bx * by; info->cross_bits = bb;
                pf->steps.cross_bits = (uint8_t)bb; pf->steps.cross_bx = bx;
            }
            rc = image_read(&b, bx, by, 0, 0, img);
        } else if (type == FFHIP_VP8L_COLOR_INDEXING) {
            const int colours = (int)bits_read(&b, 8) + 1;
            const int bb = vp8l_bundle_bits(colours);
            rc = image_read(&b, (uint32_t)colours, 1, 0, 0, pf->palette);
            for (int c = 1; !rc && c < colours; c++) pf->palette[c] = ffhip_vp8l_add(pf->palette[c], pf->palette[c - 1]);
            info->palette_size = colours;
            info->pixels_per_word = 1 << bb;
            pf->steps.has_index = 1;
            pf->steps.index_bits = (uint8_t)bb;
            xs = subsample(xs, bb);
        }
    }
    if (!rc && bits_over(&b)) rc = FFHIP_EINVAL;
    if (!rc) {
        pf->image_bit = b.pos;
        info->residual_width = (int32_t)xs;
        rc = image_front(&b, 1, &info->cache_bits, &info->has_meta);
        if (!rc && bits_over(&b)) rc = FFHIP_EINVAL;
    }
    if (rc) {
        ffhip_vp8l_close(pf);
        memset(info, 0, sizeof(*info));
        return rc;
    }
    pf->lenient_end = alpha_plane && info->n_transforms == 1 && info->transforms[0] == FFHIP_VP8L_COLOR_INDEXING;
    /* the device form: the steps in the order they are undone, last transform first, colour indexing behind them all */
    ffhip_vp8l_steps *s = &pf->steps;
    s->has_alpha = (uint8_t)info->has_alpha;
    pf->device_form = 1;
    for (int k = info->n_transforms - 1; k >= 0; k--) {
        const int type = info->transforms[k];
        if (type == FFHIP_VP8L_COLOR_INDEXING) { if (k != 0) pf->device_form = 0; }
        else if (type == FFHIP_VP8L_PREDICTOR) s->has_predictor = 1;
        else if (s->has_predictor) s->post[s->n_post++] = (uint8_t)type;
        else s->pre[s->n_pre++] = (uint8_t)type;
    }
    if (!s->has_predictor) { /* without a predictor k_vp8l_finish undoes them all */
        for (int k = 0; k < s->n_pre; k++) s->post[k] = s->pre[k];
        s->n_post = s->n_pre;
        s->n_pre = 0;
    }
    return FFHIP_OK;
}

int ffhip_vp8l_read_info(const uint8_t *file, size_t len, ffhip_vp8l_info *info)
{
    if (!file || !info) return FFHIP_EINVAL;
    ffhip_vp8l_file *pf = (ffhip_vp8l_file *)malloc(sizeof(*pf));
    if (!pf) return FFHIP_ENOMEM;
    const int rc = ffhip_vp8l_open(file, len, pf);
    *info = pf->info;
    ffhip_vp8l_close(pf);
    free(pf);
    return rc;
}

int ffhip_vp8l_read_residual(const ffhip_vp8l_file *pf, uint32_t *residual)
{
    bits b = {pf->stream, pf->stream_len, pf->image_bit};
    return image_read(&b, (uint32_t)pf->info.residual_width, (uint32_t)pf->info.height, 1, pf->lenient_end, residual);
}

int ffhip_vp8l_invert_host(const ffhip_vp8l_file *pf, uint32_t *residual, uint32_t *argb)
{
    const ffhip_vp8l_info *info = &pf->info;
    const uint32_t h = (uint32_t)info->height;
    uint32_t *cur = residual, *own = NULL; /* own: an expansion's buffer, this function's to free */
    uint32_t cur_w = (uint32_t)info->residual_width;
    for (int k = info->n_transforms - 1; k >= 0; k--) {
        const int type = info->transforms[k];
        const uint32_t w = pf->xsize[k];
        if (type == FFHIP_VP8L_PREDICTOR) {
            ffhip_vp8l_predict_rows(cur, w, h, info->predictor_bits, pf->predictor_image, pf->steps.predictor_bx);
        } else if (type == FFHIP_VP8L_COLOR_INDEXING) {
            uint32_t *wide = (uint32_t *)malloc((size_t)w * h * 4);
            if (!wide) { free(own); return FFHIP_ENOMEM; }
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++)
                    wide[(size_t)y * w + x] = ffhip_vp8l_index(cur[(size_t)y * cur_w + (x >> pf->steps.index_bits)], x, pf->steps.index_bits, pf->palette);
            free(own);
            cur = own = wide;
        } else {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) cur[(size_t)y * w + x] = ffhip_vp8l_pointwise(type, cur[(size_t)y * w + x], x, y, &pf->steps, pf->cross_image);
        }
        cur_w = w;
    }
    memcpy(argb, cur, (size_t)info->width * h * 4);
    free(own);
    return FFHIP_OK;
}

int ffhip_vp8l_picture(const uint8_t *file, size_t len, uint8_t *bgra, int64_t pitch)
{
    if (!file || !bgra) return FFHIP_EINVAL;
    ffhip_vp8l_file *pf = (ffhip_vp8l_file *)malloc(sizeof(*pf));
    if (!pf) return FFHIP_ENOMEM;
    int rc = ffhip_vp8l_open(file, len, pf);
    if (rc) { free(pf); return rc; }
    const uint32_t w = (uint32_t)pf->info.width, h = (uint32_t)pf->info.height;
    uint32_t *res = NULL, *argb = NULL;
    if (pitch < 4LL * w) rc = FFHIP_EINVAL;
    if (!rc && (!(res = (uint32_t *)malloc((size_t)pf->info.residual_width * h * 4)) || !(argb = (uint32_t *)malloc((size_t)w * h * 4)))) rc = FFHIP_ENOMEM;
    if (!rc) rc = ffhip_vp8l_read_residual(pf, res);
    if (!rc) rc = ffhip_vp8l_invert_host(pf, res, argb);
    if (!rc) {
        const uint32_t opaque = pf->info.has_alpha ? 0 : 0xff000000u;
        for (uint32_t y = 0; y < h; y++) {
            uint8_t *out = bgra + (int64_t)y * pitch;
            for (uint32_t x = 0; x < w; x++) {
                const uint32_t v = argb[(size_t)y * w + x] | opaque;
                out[4 * x] = (uint8_t)v;
                out[4 * x + 1] = (uint8_t)(v >> 8);
                out[4 * x + 2] = (uint8_t)(v >> 16);
                out[4 * x + 3] = (uint8_t)(v >> 24);
            }
        }
    }
    free(res);
    free(argb);
    ffhip_vp8l_close(pf);
    free(pf);
    return rc;
}
