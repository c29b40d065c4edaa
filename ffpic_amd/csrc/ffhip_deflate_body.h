/* ffhip_deflate_body.h -- the deflate rule of include/ffpic_hip.h "PNG encoding"  as ONE body for the host entries
 * (ffhip_deflate.c, gcc) and k_deflate_chunks (ffhip_deflate_gpu.hip, hipcc): one chunk of FFHIP_DEFLATE_CHUNK bytes becomes one deflate
 * block, by 64 lanes.
 *
 * The body is written in LANE FORM.  Code between FFHIP_DEF_LANES_BEGIN and FFHIP_DEF_LANES_END is what lane `lane` does: the kernel runs
 * it once with lane = threadIdx.x and a workgroup barrier behind it, the host runs it for lane = 0 .. 63 in turn.  Code outside such a
 * section is wave-uniform: every lane of the kernel computes the same values from the store, the host computes them once.  A section
 * never reads what another lane writes in the same section, except through FFHIP_DEF_MAX / _ADD / _OR, whose results do not depend on
 * the order of the lanes; so both runs give the same bytes.  The store is LDS in the kernel and a heap object on the host.
 *
 * The four stages of ffhip_def_chunk:
 *   candidates  a step is 64 positions.  A lane reads its candidates -- distances 1, 2, 3, 4 (any position of the stream, earlier chunks
 *               included) and the head of its 4-byte hash (the latest position of EARLIER steps of this chunk with that hash) -- and keeps
 *               the longest match, the first of equal ones; then the step's positions go into the table by FFHIP_DEF_MAX.
 *   parse       greedy: the walk over the step's lanes from the first position no token covers, uniform, at most 64 turns.
 *   codes       frequencies by FFHIP_DEF_ADD; ffhip_def_code_lengths; the run-length coding of the lengths; canonical codes.
 *   emission    a token's bits at the position a prefix sum over the step's lanes gives, by FFHIP_DEF_OR into zeroed words.
 * Every loop runs to a bound known at its entry. */
#ifndef FFHIP_DEFLATE_BODY_H
#define FFHIP_DEFLATE_BODY_H

#include "ffhip_inflate_body.h" /* the length and distance tables, the code-length order, the Adler pieces */

#define FFHIP_DEF_CHUNK 16384u /* FFHIP_DEFLATE_CHUNK of the public header */
#define FFHIP_DEF_LANES 64
#define FFHIP_DEF_HASH_BITS 12
#define FFHIP_DEF_MAXSYM 288
#define FFHIP_DEF_OUT_BYTES (FFHIP_DEF_CHUNK + 32u) /* a chunk's output: stored form 5 + CHUNK, the empty stored block 5, three words of slack for the last token's FFHIP_DEF_OR */
#define FFHIP_DEF_TOK_LIT 0x80000000u   /* | byte */
#define FFHIP_DEF_TOK_MATCH 0x40000000u /* | length << 16 | distance - 1 */

#ifdef __HIPCC__
#define FFHIP_DEF_FN __device__ static inline
#define FFHIP_DEF_NOINLINE __device__ static __attribute__((noinline)) /* called three times a chunk: one copy of its code */
#define FFHIP_DEF_HD __host__ __device__ static inline /* the pieces without lanes */
#define FFHIP_DEF_LANES_BEGIN { const int lane = (int)threadIdx.x;
#define FFHIP_DEF_LANES_END } __syncthreads();
#define FFHIP_DEF_BARRIER() __syncthreads()
#define FFHIP_DEF_ROLLED _Pragma("nounroll") /* the loops stay loops: unrolled, the chunk's one long function runs out of scalar registers */
#define FFHIP_DEF_MAX(p, v) atomicMax((p), (v))
#define FFHIP_DEF_ADD(p, v) atomicAdd((p), (v))
#define FFHIP_DEF_OR(p, v) atomicOr((p), (v))
#define FFHIP_DEF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x))) /* a value every lane holds, for the scalar unit */
#else
#define FFHIP_DEF_FN static inline
#define FFHIP_DEF_NOINLINE static
#define FFHIP_DEF_HD static inline
#define FFHIP_DEF_LANES_BEGIN for (int lane = 0; lane < FFHIP_DEF_LANES; lane++) {
#define FFHIP_DEF_LANES_END }
#define FFHIP_DEF_BARRIER() ((void)0)
#define FFHIP_DEF_ROLLED
#define FFHIP_DEF_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define FFHIP_DEF_ADD(p, v) (*(p) += (v))
#define FFHIP_DEF_OR(p, v) (*(p) |= (v))
#define FFHIP_DEF_UNIFORM(x) ((uint32_t)(x))
#endif

typedef struct ffhip_def_store {
    uint32_t head[1 << FFHIP_DEF_HASH_BITS]; /* position in the chunk + 1 of the hash's latest position of the earlier steps; 0: none */
    uint32_t freq_ll[FFHIP_DEF_MAXSYM], freq_d[32], freq_cl[20];
    uint32_t w[FFHIP_DEF_MAXSYM];            /* the length rule: the frequencies of the round */
    uint32_t node_w[2 * FFHIP_DEF_MAXSYM];
    uint16_t order[FFHIP_DEF_MAXSYM], parent[2 * FFHIP_DEF_MAXSYM], depth[2 * FFHIP_DEF_MAXSYM];
    uint16_t code_ll[FFHIP_DEF_MAXSYM], code_d[32], code_cl[20]; /* bit-reversed: the first bit of the code is bit 0 */
    uint8_t len_ll[FFHIP_DEF_MAXSYM], len_d[32], len_cl[20];
    uint8_t seq_sym[320], seq_ext[320];      /* the lengths of both alphabets, run-length coded: symbol 0..18 and the value of its extra bits */
    uint32_t lane_a[FFHIP_DEF_LANES], lane_b[FFHIP_DEF_LANES]; /* a step's (length, distance), a step's bit counts, an Adler block's sums, the CRC segments */
    uint32_t used, maxd, n_seq, hlit, hdist, hclen, stored;
    uint32_t bits_lo, bits_hi;               /* of the dynamic block, end-of-block code included */
} ffhip_def_store;

/* one chunk's result */
typedef struct ffhip_def_result {
    uint32_t out_len;          /* bytes of the chunk's output, the empty stored block behind a chunk that is not the last included */
    uint32_t adler_a, adler_b; /* Adler-32 of the chunk's input from (1, 0) */
    uint32_t crc;              /* CRC-32 of the chunk's output */
} ffhip_def_result;

/* ---- CRC-32 (reflected 0xEDB88320): bytes, and the join of two finished values ---- */
FFHIP_DEF_HD uint32_t ffhip_def_crc_bytes(uint32_t crc, const uint8_t *p, uint32_t n)
{
    crc = ~crc;
    FFHIP_DEF_ROLLED
    for (uint32_t i = 0; i < n; i++) {
        crc ^= p[i];
        FFHIP_DEF_ROLLED
        for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}
/* a x b mod the polynomial; x^k is bit 31 - k */
FFHIP_DEF_HD uint32_t ffhip_def_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    FFHIP_DEF_ROLLED
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
/* x^(8 n) */
FFHIP_DEF_HD uint32_t ffhip_def_crc_x8n(uint64_t n)
{
    uint32_t r = 0x80000000u, q = 0x00800000u; /* 1, x^8 */
    FFHIP_DEF_ROLLED
    for (int k = 0; k < 64; k++) {
        if ((n >> k) & 1) r = ffhip_def_crc_mul(r, q);
        q = ffhip_def_crc_mul(q, q);
    }
    return r;
}
/* CRC-32 of A || B from the CRC-32 of A, the CRC-32 of B and x^(8 |B|) */
FFHIP_DEF_HD uint32_t ffhip_def_crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t x8n_b) { return ffhip_def_crc_mul(x8n_b, crc_a) ^ crc_b; }

/* Adler-32 of A || B from the parts' values, each from (1, 0) */
FFHIP_DEF_HD void ffhip_def_adler_join(uint32_t *a, uint32_t *b, uint32_t a2, uint32_t b2, uint64_t len2)
{
    const uint64_t a1 = *a;
    *b = (uint32_t)((*b + b2 + (len2 % 65521u) * ((a1 + 65520u) % 65521u)) % 65521u);
    *a = (uint32_t)((a1 + a2 + 65520u) % 65521u);
}

FFHIP_DEF_HD uint64_t ffhip_def_chunks(uint64_t len) { return len ? (len + FFHIP_DEF_CHUNK - 1) / FFHIP_DEF_CHUNK : 1; }

/* ---- the length rule ----
 * lengths[0 .. n) of a complete prefix code of at most `limit` bits for the symbols with freq > 0; n <= FFHIP_DEF_MAXSYM, 2^limit >= n,
 * the frequencies' sum below 2^32.  Huffman's algorithm on the symbols sorted by (frequency, symbol): two queues, the leaf before the inner
 * node at equal weight.  While the deepest leaf lies beyond the limit, every used frequency becomes (f + 1) / 2 and the tree is built
 * again; after 32 rounds all are 1 and the tree is balanced.  One used symbol gets one bit, none gets nothing. */
FFHIP_DEF_NOINLINE void ffhip_def_code_lengths(ffhip_def_store *m, const uint32_t *freq, int n, int limit, uint8_t *lengths)
{
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int s = lane; s < n; s += FFHIP_DEF_LANES) {
            m->w[s] = freq[s];
            lengths[s] = 0;
        }
    FFHIP_DEF_LANES_END
    FFHIP_DEF_ROLLED
    for (int round = 0; round < 33; round++) {
        FFHIP_DEF_LANES_BEGIN
            FFHIP_DEF_ROLLED
            for (int s = lane; s < n; s += FFHIP_DEF_LANES) {
                const uint32_t ws = m->w[s];
                if (!ws) continue;
                int r = 0;
                FFHIP_DEF_ROLLED
                for (int t = 0; t < n; t++) {
                    const uint32_t wt = m->w[t];
                    r += wt && (wt < ws || (wt == ws && t < s));
                }
                m->order[r] = (uint16_t)s;
            }
            if (lane == 0) {
                uint32_t k = 0;
                FFHIP_DEF_ROLLED
                for (int t = 0; t < n; t++) k += m->w[t] != 0;
                m->used = k;
            }
        FFHIP_DEF_LANES_END
        const int k = (int)FFHIP_DEF_UNIFORM(m->used);
        if (k == 0) return;
        if (k == 1) {
            FFHIP_DEF_LANES_BEGIN
                if (lane == 0) lengths[m->order[0]] = 1;
            FFHIP_DEF_LANES_END
            return;
        }
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) {
                FFHIP_DEF_ROLLED
                for (int i = 0; i < k; i++) m->node_w[i] = m->w[m->order[i]];
                int li = 0, ii = k;
                FFHIP_DEF_ROLLED
                for (int c = k; c < 2 * k - 1; c++) {
                    uint32_t sum = 0;
                    FFHIP_DEF_ROLLED
                    for (int pick = 0; pick < 2; pick++) {
                        const int a = (li < k && (ii >= c || m->node_w[li] <= m->node_w[ii])) ? li++ : ii++;
                        sum += m->node_w[a];
                        m->parent[a] = (uint16_t)c;
                    }
                    m->node_w[c] = sum;
                }
                m->depth[2 * k - 2] = 0;
                FFHIP_DEF_ROLLED
                for (int i = 2 * k - 3; i >= 0; i--) m->depth[i] = (uint16_t)(m->depth[m->parent[i]] + 1);
                m->maxd = m->depth[0]; /* the lightest leaf is a deepest one */
            }
        FFHIP_DEF_LANES_END
        if ((int)FFHIP_DEF_UNIFORM(m->maxd) <= limit) {
            FFHIP_DEF_LANES_BEGIN
                FFHIP_DEF_ROLLED
                for (int i = lane; i < k; i += FFHIP_DEF_LANES) lengths[m->order[i]] = (uint8_t)m->depth[i];
            FFHIP_DEF_LANES_END
            return;
        }
        FFHIP_DEF_LANES_BEGIN
            FFHIP_DEF_ROLLED
            for (int s = lane; s < n; s += FFHIP_DEF_LANES)
                if (m->w[s]) m->w[s] = (m->w[s] + 1) >> 1;
        FFHIP_DEF_LANES_END
    }
}

/* canonical codes of lengths[0 .. n), bit-reversed (one lane's work) */
FFHIP_DEF_FN void ffhip_def_codes(const uint8_t *lengths, int n, uint16_t *codes)
{
    uint32_t code = 0;
    FFHIP_DEF_ROLLED
    for (int l = 1; l <= 15; l++) {
        FFHIP_DEF_ROLLED
        for (int s = 0; s < n; s++) {
            if (lengths[s] != l) continue;
            uint32_t rev = 0;
            FFHIP_DEF_ROLLED
            for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
            codes[s] = (uint16_t)rev;
            code++;
        }
        code <<= 1;
    }
}

FFHIP_DEF_FN int ffhip_def_len_symbol(uint32_t len)
{
    int s = 28;
    FFHIP_DEF_ROLLED
    for (; s > 0; s--)
        if (len >= ffhip_inf_len_base(s)) break;
    return s;
}
FFHIP_DEF_FN int ffhip_def_dist_symbol(uint32_t dist)
{
    int s = 29;
    FFHIP_DEF_ROLLED
    for (; s > 0; s--)
        if (dist >= ffhip_inf_dist_base(s)) break;
    return s;
}

/* nbits <= 48 bits of v at bit `pos` of the zeroed words */
FFHIP_DEF_FN void ffhip_def_put(uint32_t *words, uint64_t pos, uint64_t v, int nbits)
{
    if (!nbits) return;
    uint32_t *w = words + (pos >> 5);
    const int sh = (int)(pos & 31);
    const uint32_t w0 = (uint32_t)(v << sh);
    const uint64_t rest = sh ? v >> (32 - sh) : v >> 32;
    if (w0) FFHIP_DEF_OR(w, w0);
    if ((uint32_t)rest) FFHIP_DEF_OR(w + 1, (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) FFHIP_DEF_OR(w + 2, (uint32_t)(rest >> 32));
}

/* a token's bits under the store's codes: *v, the count returned; 0 for no token */
FFHIP_DEF_FN int ffhip_def_token_bits(const ffhip_def_store *m, uint32_t tok, uint64_t *v)
{
    *v = 0;
    if (tok & FFHIP_DEF_TOK_LIT) {
        *v = m->code_ll[tok & 255u];
        return m->len_ll[tok & 255u];
    }
    if (!(tok & FFHIP_DEF_TOK_MATCH)) return 0;
    const uint32_t len = (tok >> 16) & 0x1ffu, dist = (tok & 0xffffu) + 1;
    const int ls = ffhip_def_len_symbol(len), ds = ffhip_def_dist_symbol(dist);
    int n = m->len_ll[257 + ls];
    uint64_t b = m->code_ll[257 + ls];
    b |= (uint64_t)(len - ffhip_inf_len_base(ls)) << n;
    n += (int)ffhip_inf_len_extra(ls);
    b |= (uint64_t)m->code_d[ds] << n;
    n += m->len_d[ds];
    b |= (uint64_t)(dist - ffhip_inf_dist_base(ds)) << n;
    n += (int)ffhip_inf_dist_extra(ds);
    *v = b;
    return n;
}

FFHIP_DEF_FN uint32_t ffhip_def_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return (v * 2654435761u) >> (32 - FFHIP_DEF_HASH_BITS);
}

/* exclusive prefix sum of lane_a over the lanes in front of `lane`, and the sum of all */
FFHIP_DEF_FN uint32_t ffhip_def_prefix(const ffhip_def_store *m, int lane, uint32_t *total)
{
#ifdef __HIPCC__
    const uint32_t own = m->lane_a[lane];
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
    FFHIP_DEF_ROLLED
    for (int k = 0; k < FFHIP_DEF_LANES; k++) {
        if (k < lane) before += m->lane_a[k];
        all += m->lane_a[k];
    }
    *total = all;
    return before;
#endif
}

/* Chunk [at, at + n) of the stream src[0 .. len): n <= FFHIP_DEF_CHUNK, n > 0 unless the stream is empty; final: the stream's last.
 * tok: n words of scratch (a position's token, 0 where none starts); out: FFHIP_DEF_OUT_BYTES / 4 words, ZEROED by the caller. */
FFHIP_DEF_FN void ffhip_def_chunk(ffhip_def_store *m, const uint8_t *src, uint64_t at, uint32_t n, int final, uint32_t *tok, uint32_t *out,
                                  ffhip_def_result *res)
{
    const uint8_t *in = src + at;
    FFHIP_DEF_LANES_BEGIN
        FFHIP_DEF_ROLLED
        for (int k = lane; k < (1 << FFHIP_DEF_HASH_BITS); k += FFHIP_DEF_LANES) m->head[k] = 0;
        FFHIP_DEF_ROLLED
        for (int k = lane; k < FFHIP_DEF_MAXSYM; k += FFHIP_DEF_LANES) m->freq_ll[k] = k == 256;
        if (lane < 32) m->freq_d[lane] = 0;
        if (lane < 20) m->freq_cl[lane] = 0;
    FFHIP_DEF_LANES_END

    /* ---- candidates and parse ---- */
    uint32_t next = 0; /* the first position no token covers yet */
    FFHIP_DEF_ROLLED
    for (uint32_t base = 0; base < n; base += FFHIP_DEF_LANES) {
        FFHIP_DEF_LANES_BEGIN
            const uint32_t p = base + (uint32_t)lane;
            uint32_t best = 0, best_dist = 0;
            if (p < n && p >= next) {
                const uint32_t room = n - p, maxlen = room < 258u ? room : 258u;
                FFHIP_DEF_ROLLED
                for (uint32_t d = 1; d <= 5 && best < maxlen; d++) {
                    uint32_t dist = d, need = 3;
                    if (d == 5) {
                        const uint32_t h = p + 4 <= n ? m->head[ffhip_def_hash(in + p)] : 0u;
                        if (!h) break;
                        dist = p - (h - 1);
                        need = 4;
                    } else if (at + p < d) continue;
                    const uint8_t *q = in + p - dist;
                    uint32_t l = 0;
                    FFHIP_DEF_ROLLED
                    while (l < maxlen && q[l] == in[p + l]) l++;
                    if (l >= need && l > best) {
                        best = l;
                        best_dist = dist;
                    }
                }
            }
            m->lane_a[lane] = best;
            m->lane_b[lane] = best_dist;
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
                    const uint32_t len = m->lane_a[lane], dist = m->lane_b[lane];
                    if (len) {
                        t = FFHIP_DEF_TOK_MATCH | (len << 16) | (dist - 1);
                        FFHIP_DEF_ADD(&m->freq_ll[257 + ffhip_def_len_symbol(len)], 1u);
                        FFHIP_DEF_ADD(&m->freq_d[ffhip_def_dist_symbol(dist)], 1u);
                    } else {
                        t = FFHIP_DEF_TOK_LIT | in[p];
                        FFHIP_DEF_ADD(&m->freq_ll[in[p]], 1u);
                    }
                }
                tok[p] = t;
                if (p + 4 <= n) FFHIP_DEF_MAX(&m->head[ffhip_def_hash(in + p)], p + 1);
            }
        FFHIP_DEF_LANES_END
    }

    /* ---- codes ---- */
    ffhip_def_code_lengths(m, m->freq_ll, 286, 15, m->len_ll);
    ffhip_def_code_lengths(m, m->freq_d, 30, 15, m->len_d);
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) {
            int hlit = 286, hdist = 30;
            FFHIP_DEF_ROLLED
            while (hlit > 257 && !m->len_ll[hlit - 1]) hlit--;
            FFHIP_DEF_ROLLED
            while (hdist > 1 && !m->len_d[hdist - 1]) hdist--;
            if (hdist == 1 && !m->len_d[0]) m->len_d[0] = 1; /* no match in the block: one distance code of one bit */
            m->hlit = (uint32_t)hlit;
            m->hdist = (uint32_t)hdist;
            /* the lengths of both alphabets as one sequence, run-length coded */
            const int total = hlit + hdist;
            uint32_t k = 0;
            FFHIP_DEF_ROLLED
            for (int i = 0; i < total;) {
                const int v = i < hlit ? m->len_ll[i] : m->len_d[i - hlit];
                int run = 1;
                FFHIP_DEF_ROLLED
                while (i + run < total && (i + run < hlit ? m->len_ll[i + run] : m->len_d[i + run - hlit]) == v) run++;
                i += run;
                if (v) {
                    m->seq_sym[k] = (uint8_t)v; m->seq_ext[k++] = 0;
                    run--;
                }
                FFHIP_DEF_ROLLED
                while (run >= 3) {
                    const int take = v ? (run > 6 ? 6 : run) : (run > 138 ? 138 : run);
                    if (v) { m->seq_sym[k] = 16; m->seq_ext[k++] = (uint8_t)(take - 3); }
                    else if (take >= 11) { m->seq_sym[k] = 18; m->seq_ext[k++] = (uint8_t)(take - 11); }
                    else { m->seq_sym[k] = 17; m->seq_ext[k++] = (uint8_t)(take - 3); }
                    run -= take;
                }
                FFHIP_DEF_ROLLED
                for (; run > 0; run--) { m->seq_sym[k] = (uint8_t)v; m->seq_ext[k++] = 0; }
            }
            m->n_seq = k;
            FFHIP_DEF_ROLLED
            for (uint32_t i = 0; i < k; i++) m->freq_cl[m->seq_sym[i]]++;
        }
    FFHIP_DEF_LANES_END
    ffhip_def_code_lengths(m, m->freq_cl, 19, 7, m->len_cl);
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) {
            ffhip_def_codes(m->len_ll, 286, m->code_ll);
            ffhip_def_codes(m->len_d, 30, m->code_d);
            ffhip_def_codes(m->len_cl, 19, m->code_cl);
            int hclen = 19;
            FFHIP_DEF_ROLLED
            while (hclen > 4 && !m->len_cl[ffhip_inf_clen_order(hclen - 1)]) hclen--;
            m->hclen = (uint32_t)hclen;
            uint64_t bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
            FFHIP_DEF_ROLLED
            for (uint32_t i = 0; i < m->n_seq; i++) {
                const int s = m->seq_sym[i];
                bits += (uint64_t)m->len_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
            }
            FFHIP_DEF_ROLLED
            for (int s = 0; s < 286; s++) bits += (uint64_t)m->freq_ll[s] * (m->len_ll[s] + (s > 256 ? ffhip_inf_len_extra(s - 257) : 0u));
            FFHIP_DEF_ROLLED
            for (int s = 0; s < 30; s++) bits += (uint64_t)m->freq_d[s] * (m->len_d[s] + ffhip_inf_dist_extra(s));
            m->bits_lo = (uint32_t)bits;
            m->bits_hi = (uint32_t)(bits >> 32);
            m->stored = n == 0 || (uint64_t)n + 5 <= (bits + 7) / 8; /* stored when the dynamic block is not shorter */
        }
    FFHIP_DEF_LANES_END

    /* ---- emission ---- */
    uint64_t end_bits; /* of the block */
    if (FFHIP_DEF_UNIFORM(m->stored)) {
        FFHIP_DEF_LANES_BEGIN
            uint8_t *o = (uint8_t *)out;
            if (lane == 0) {
                o[0] = (uint8_t)(final ? 1 : 0);
                o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8);
            }
            FFHIP_DEF_ROLLED
            for (uint32_t i = (uint32_t)lane; i < n; i += FFHIP_DEF_LANES) o[5 + i] = in[i];
        FFHIP_DEF_LANES_END
        end_bits = 8 * ((uint64_t)n + 5);
    } else {
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) {
                uint64_t pos = 0;
                ffhip_def_put(out, pos, (uint64_t)(final ? 1 : 0) | 4u, 3); pos += 3; /* BFINAL, BTYPE 10 */
                ffhip_def_put(out, pos, m->hlit - 257, 5); pos += 5;
                ffhip_def_put(out, pos, m->hdist - 1, 5); pos += 5;
                ffhip_def_put(out, pos, m->hclen - 4, 4); pos += 4;
                FFHIP_DEF_ROLLED
                for (uint32_t i = 0; i < m->hclen; i++) { ffhip_def_put(out, pos, m->len_cl[ffhip_inf_clen_order((int)i)], 3); pos += 3; }
                FFHIP_DEF_ROLLED
                for (uint32_t i = 0; i < m->n_seq; i++) {
                    const int s = m->seq_sym[i], e = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
                    ffhip_def_put(out, pos, (uint64_t)m->code_cl[s] | ((uint64_t)m->seq_ext[i] << m->len_cl[s]), m->len_cl[s] + e);
                    pos += (uint64_t)(m->len_cl[s] + e);
                }
                m->lane_b[0] = (uint32_t)pos; /* the header's bits: below 2^12 */
            }
        FFHIP_DEF_LANES_END
        uint64_t pos = FFHIP_DEF_UNIFORM(m->lane_b[0]);
        FFHIP_DEF_ROLLED
        for (uint32_t base = 0; base < n; base += FFHIP_DEF_LANES) {
            FFHIP_DEF_LANES_BEGIN
                const uint32_t p = base + (uint32_t)lane;
                uint64_t v;
                m->lane_a[lane] = p < n ? (uint32_t)ffhip_def_token_bits(m, tok[p], &v) : 0u;
            FFHIP_DEF_LANES_END
            FFHIP_DEF_LANES_BEGIN
                const uint32_t p = base + (uint32_t)lane;
                uint32_t all;
                const uint32_t before = ffhip_def_prefix(m, lane, &all);
                if (p < n) {
                    uint64_t v;
                    const int nb = ffhip_def_token_bits(m, tok[p], &v);
                    ffhip_def_put(out, pos + before, v, nb);
                }
                if (lane == 0) m->lane_b[0] = all;
            FFHIP_DEF_LANES_END
            pos += FFHIP_DEF_UNIFORM(m->lane_b[0]); /* written again only behind the next step's first barrier */
        }
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) ffhip_def_put(out, pos, m->code_ll[256], m->len_ll[256]);
        FFHIP_DEF_LANES_END
        end_bits = pos + FFHIP_DEF_UNIFORM(m->len_ll[256]);
    }
    /* behind a chunk that is not the last: the empty stored block -- its three header bits are zeros of the zeroed words, then to the byte
     * boundary, then 00 00 FF FF */
    uint32_t out_len = (uint32_t)((end_bits + 7) >> 3);
    if (!final) {
        out_len = (uint32_t)((end_bits + 3 + 7) >> 3) + 4;
        FFHIP_DEF_LANES_BEGIN
            if (lane == 0) ffhip_def_put(out, 8 * (uint64_t)(out_len - 2), 0xffffu, 16);
        FFHIP_DEF_LANES_END
    }

    /* ---- the check values: Adler-32 of the input, CRC-32 of the output ---- */
    uint32_t a = 1, b = 0;
    FFHIP_DEF_ROLLED
    for (uint32_t blk = 0; blk < n; blk += FFHIP_INF_ADLER_BLOCK) {
        const uint32_t cnt = n - blk < FFHIP_INF_ADLER_BLOCK ? n - blk : FFHIP_INF_ADLER_BLOCK;
        FFHIP_DEF_LANES_BEGIN
            ffhip_inf_adler_lane(in + blk, cnt, lane, &m->lane_a[lane], &m->lane_b[lane]);
        FFHIP_DEF_LANES_END
        uint32_t s1 = 0, s2 = 0;
        FFHIP_DEF_ROLLED
        for (int k = 0; k < FFHIP_DEF_LANES; k++) {
            s1 += m->lane_a[k];
            s2 += m->lane_b[k];
        }
        ffhip_inf_adler_fold(&a, &b, cnt, s1, s2);
        FFHIP_DEF_BARRIER(); /* the sums are read before the next block's are written */
    }
    const uint32_t seg = (out_len + FFHIP_DEF_LANES - 1) / FFHIP_DEF_LANES; /* a lane's bytes of the output */
    FFHIP_DEF_LANES_BEGIN
        const uint32_t from = (uint32_t)lane * seg, cnt = from >= out_len ? 0u : (out_len - from < seg ? out_len - from : seg);
        m->lane_a[lane] = ffhip_def_crc_bytes(0, (const uint8_t *)out + from, cnt);
        m->lane_b[lane] = cnt;
    FFHIP_DEF_LANES_END
    FFHIP_DEF_LANES_BEGIN
        if (lane == 0) {
            uint32_t crc = 0;
            const uint32_t xs = ffhip_def_crc_x8n(seg);
            FFHIP_DEF_ROLLED
            for (int k = 0; k < FFHIP_DEF_LANES; k++) {
                const uint32_t cnt = m->lane_b[k];
                if (cnt) crc = ffhip_def_crc_join(crc, m->lane_a[k], cnt == seg ? xs : ffhip_def_crc_x8n(cnt));
            }
            res->out_len = out_len;
            res->adler_a = a;
            res->adler_b = b;
            res->crc = crc;
        }
    FFHIP_DEF_LANES_END
}

#endif
