/* ffhip_deflate.c -- the host side of the deflate rule (include/ffpic_hip.h "PNG encoding"): a zlib stream from host bytes,
 * the bound, the length rule alone.  Plain C, no device; every chunk goes through ffhip_deflate_body.h's ffhip_def_chunk, the body
 * k_deflate_chunks compiles, with the 64 lanes run in turn. */
#include "ffhip_deflate_internal.h"

#include <stdlib.h>
#include <string.h>

size_t ffhip_deflate_bound(size_t len)
{
    const uint64_t chunks = ffhip_def_chunks(len);
    return (size_t)(2 + len + 5 * chunks + 5 * (chunks - 1) + 4);
}

int ffhip_deflate_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *lengths)
{
    if (!freq || !lengths || n < 1 || n > FFHIP_DEF_MAXSYM || limit < 1 || limit > 15 || (1 << limit) < n) return FFHIP_EINVAL;
    uint64_t sum = 0;
    for (int s = 0; s < n; s++) sum += freq[s];
    if (sum >> 32) return FFHIP_EINVAL;
    ffhip_def_store *m = (ffhip_def_store *)malloc(sizeof(*m));
    if (!m) return FFHIP_ENOMEM;
    ffhip_def_code_lengths(m, freq, n, limit, lengths);
    free(m);
    return FFHIP_OK;
}

int ffhip_deflate_chunks_host(const uint8_t *src, size_t len, uint8_t **out, ffhip_def_result **res, uint64_t *n_chunks)
{
    const uint64_t chunks = ffhip_def_chunks(len);
    ffhip_def_store *m = (ffhip_def_store *)malloc(sizeof(*m));
    uint32_t *tok = (uint32_t *)malloc(FFHIP_DEF_CHUNK * sizeof(uint32_t));
    *out = (uint8_t *)calloc((size_t)chunks, FFHIP_DEF_OUT_BYTES);
    *res = (ffhip_def_result *)calloc((size_t)chunks, sizeof(ffhip_def_result));
    *n_chunks = chunks;
    if (!m || !tok || !*out || !*res) {
        free(m); free(tok); free(*out); free(*res);
        *out = NULL; *res = NULL;
        return FFHIP_ENOMEM;
    }
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t at = c * FFHIP_DEF_CHUNK, left = len - at;
        ffhip_def_chunk(m, src, at, (uint32_t)(left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK), c == chunks - 1, tok,
                        (uint32_t *)(*out + c * FFHIP_DEF_OUT_BYTES), *res + c);
    }
    free(m); free(tok);
    return FFHIP_OK;
}

int ffhip_deflate(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len)
{
    if ((len && !src) || (cap && !dst) || !out_len) return FFHIP_EINVAL;
    uint8_t *out;
    ffhip_def_result *res;
    uint64_t chunks;
    const int rc = ffhip_deflate_chunks_host(src, len, &out, &res, &chunks);
    if (rc) return rc;
    size_t o = 0;
    uint32_t a = 1, b = 0;
    const uint8_t head[2] = {0x78, 0x01};
    for (int k = 0; k < 2; k++, o++)
        if (o < cap) dst[o] = head[k];
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t at = c * FFHIP_DEF_CHUNK, left = len - at;
        for (uint32_t k = 0; k < res[c].out_len; k++, o++)
            if (o < cap) dst[o] = out[c * FFHIP_DEF_OUT_BYTES + k];
        ffhip_def_adler_join(&a, &b, res[c].adler_a, res[c].adler_b, left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK);
    }
    const uint8_t tail[4] = {(uint8_t)(b >> 8), (uint8_t)b, (uint8_t)(a >> 8), (uint8_t)a};
    for (int k = 0; k < 4; k++, o++)
        if (o < cap) dst[o] = tail[k];
    free(out); free(res);
    *out_len = o;
    return o > cap ? FFHIP_EDEFLATE_NOSPACE : FFHIP_OK;
}
