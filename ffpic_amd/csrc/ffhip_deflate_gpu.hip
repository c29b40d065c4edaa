/*
 * ffhip_deflate_gpu.hip -- deflate on the device (include/ffpic_hip.h "PNG encoding").  The rule is ffhip_deflate_body.h's,
 * shared with the host functions of ffhip_deflate.c.
 *   k_deflate_chunks  a workgroup of ONE wave per chunk of FFHIP_DEFLATE_CHUNK bytes: ffhip_def_chunk with lane = threadIdx.x -- candidates
 *                     from the LDS head table and the fixed distances, the uniform greedy walk, the histograms by LDS atomics, the length
 *                     rule, the block's header, the tokens' bits by atomicOr into the zeroed output words, Adler-32 and CRC-32 parts.
 *                     Tokens go to scratch (a word a position: 64 KiB a chunk do not fit LDS beside the table).  Also the PNG encoder's.
 *   k_deflate_scan    a workgroup per stream: the chunks' offsets (a prefix scan in a loop of its own), the Adler parts joined, the verdict
 *   k_deflate_copy    a workgroup per chunk: header, chunk and check value into the caller's buffer, every byte under cap
 * No kernel waits for another workgroup; every loop runs to a bound known at its entry.
 * The host side is the encoders' common one: ffhip_parts_run, ffhip_items_run, ffhip_lengths_read; deflate_part's offsets are its own.
 */
#include "ffhip_items.h"
#include "ffhip_parts.h"
#include "ffhip_wave.h" /* wg_scan */
#include "ffhip_deflate_internal.h"

#include <string.h>

#define DEF_WG 256

namespace {

struct DefChunkArgs {
    const ffhip_def_stream *streams;
    const u32 *wg_item;
    u32 wg_base;
};

__global__ __launch_bounds__(FFHIP_DEF_LANES) void k_deflate_chunks(DefChunkArgs a)
{
    __shared__ ffhip_def_store m;
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const ffhip_def_stream &s = a.streams[item];
    const u32 c = wg - s.first_wg;
    const unsigned long long at = (unsigned long long)c * FFHIP_DEF_CHUNK, left = s.len - at;
    ffhip_def_chunk(&m, s.src, at, (u32)(left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK), c == s.n_wgs - 1, s.tok + at,
                    s.out + (size_t)c * (FFHIP_DEF_OUT_BYTES / 4), s.res + c);
}

struct DefDst { /* per stream, behind the ffhip_def_stream records */
    uint8_t *dst;
    unsigned long long cap;
    u32 *chunk_off; /* per chunk: where its bytes start in the stream */
};
struct DefVerdict {
    unsigned long long file_len;
    int32_t status;
    u32 adler;
};

__global__ __launch_bounds__(DEF_WG) void k_deflate_scan(const ffhip_def_stream *streams, const DefDst *dsts, DefVerdict *verdict)
{
    __shared__ u32 wave_sum[DEF_WG / 64];
    const ffhip_def_stream &s = streams[blockIdx.x];
    const DefDst &d = dsts[blockIdx.x];
    unsigned long long carry = 2; /* the zlib header */
    const u32 turns = (s.n_wgs + DEF_WG - 1) / DEF_WG;
    for (u32 turn = 0; turn < turns; turn++) {
        const u32 c = turn * DEF_WG + threadIdx.x;
        const u32 v = c < s.n_wgs ? s.res[c].out_len : 0u;
        u32 total;
        const u32 before = wg_scan<DEF_WG>(v, wave_sum, &total);
        if (c < s.n_wgs) d.chunk_off[c] = (u32)carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        u32 a = 1, b = 0;
        for (u32 c = 0; c < s.n_wgs; c++) {
            const unsigned long long left = s.len - (unsigned long long)c * FFHIP_DEF_CHUNK;
            ffhip_def_adler_join(&a, &b, s.res[c].adler_a, s.res[c].adler_b, left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK);
        }
        DefVerdict &r = verdict[blockIdx.x];
        r.file_len = carry + 4;
        r.status = r.file_len > d.cap ? FFHIP_EDEFLATE_NOSPACE : FFHIP_OK;
        r.adler = (b << 16) | a;
    }
}

__global__ __launch_bounds__(DEF_WG) void k_deflate_copy(DefChunkArgs a, const DefDst *dsts, const DefVerdict *verdict)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const ffhip_def_stream &s = a.streams[item];
    const DefDst &d = dsts[item];
    const u32 c = wg - s.first_wg, n = s.res[c].out_len;
    const unsigned long long at = d.chunk_off[c];
    const uint8_t *from = (const uint8_t *)(s.out + (size_t)c * (FFHIP_DEF_OUT_BYTES / 4));
    for (u32 k = threadIdx.x; k < n; k += DEF_WG)
        if (at + k < d.cap) d.dst[at + k] = from[k];
    if (c == 0 && threadIdx.x < 2 && threadIdx.x < d.cap) d.dst[threadIdx.x] = threadIdx.x ? 0x01 : 0x78;
    if (c == s.n_wgs - 1 && threadIdx.x < 4) {
        const unsigned long long o = verdict[item].file_len - 4 + threadIdx.x;
        if (o < d.cap) d.dst[o] = (uint8_t)(verdict[item].adler >> (24 - 8 * threadIdx.x));
    }
}

/* streams [0, n) of one part: one synchronisation */
int deflate_part(const uint8_t *const *d_src, const size_t *len, int n, uint8_t *const *d_dst, const size_t *cap, size_t *out_len, int *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<ffhip_def_stream> rec((size_t)n);
    std::vector<DefDst> dst((size_t)n);
    unsigned long long total_chunks = 0, tok_words = 0;
    for (int i = 0; i < n; i++) {
        ffhip_def_stream &s = rec[(size_t)i];
        memset(&s, 0, sizeof(s));
        s.src = d_src[i]; s.len = len[i];
        s.first_wg = (u32)total_chunks; s.n_wgs = (u32)ffhip_def_chunks(len[i]);
        total_chunks += s.n_wgs;
        tok_words += ffhip_up(len[i], 4);
        dst[(size_t)i].dst = d_dst[i]; dst[(size_t)i].cap = cap[i];
    }
    if (total_chunks > 0xffffffffULL) return FFHIP_EINVAL;
    /* the scratch: stream records and destinations (uploaded), the per-chunk table, offsets, results, verdicts, the output words (zeroed), tokens */
    const size_t rec_bytes = (size_t)n * sizeof(ffhip_def_stream), up_bytes = rec_bytes + (size_t)n * sizeof(DefDst);
    const size_t off_off = up_bytes + (size_t)total_chunks * 4, res_off = off_off + (size_t)total_chunks * 4;
    const size_t ver_off = res_off + (size_t)total_chunks * sizeof(ffhip_def_result);
    const size_t out_off = ffhip_up(ver_off + (size_t)n * sizeof(DefVerdict), 256), out_bytes = (size_t)total_chunks * FFHIP_DEF_OUT_BYTES;
    const size_t tok_off = out_off + out_bytes, end = tok_off + (size_t)tok_words * 4;
    std::vector<uint8_t> up(up_bytes);
    uint8_t *dev = nullptr;
    int rc = ffhip_items_stage(SCRATCH_PNG_ENC, stream, up.data(), up_bytes, (size_t)total_chunks, end - up_bytes - (size_t)total_chunks * 4, &dev,
                               [&](uint8_t *base) {
        size_t tok_at = 0;
        for (int i = 0; i < n; i++) {
            ffhip_def_stream &s = rec[(size_t)i];
            s.tok = (u32 *)(base + tok_off) + tok_at;
            s.out = (u32 *)(base + out_off + (size_t)s.first_wg * FFHIP_DEF_OUT_BYTES);
            s.res = (ffhip_def_result *)(base + res_off) + s.first_wg;
            dst[(size_t)i].chunk_off = (u32 *)(base + off_off) + s.first_wg;
            tok_at += ffhip_up(len[i], 4);
        }
        memcpy(up.data(), rec.data(), rec_bytes);
        memcpy(up.data() + rec_bytes, dst.data(), up_bytes - rec_bytes);
    });
    if (rc) return rc;
    const ffhip_def_stream *d_rec = (const ffhip_def_stream *)dev;
    const DefDst *d_dsts = (const DefDst *)(dev + rec_bytes);
    u32 *d_table = (u32 *)(dev + up_bytes);
    DefVerdict *d_ver = (DefVerdict *)(dev + ver_off);
    FFHIP_CHECK(hipMemsetAsync(dev + out_off, 0, out_bytes, st), FFHIP_EIO);
    hipLaunchKernelGGL(k_items_table<ffhip_def_stream>, dim3((unsigned)n), dim3(256), 0, st, d_rec, d_table);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_deflate_chunks_enqueue(d_rec, d_table, total_chunks, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_deflate_scan, dim3((unsigned)n), dim3(DEF_WG), 0, st, d_rec, d_dsts, d_ver);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    DefChunkArgs a;
    a.streams = d_rec; a.wg_item = d_table; a.wg_base = 0;
    rc = ffhip_items_run(k_deflate_copy, total_chunks, DEF_WG, stream, a, d_dsts, (const DefVerdict *)d_ver);
    if (rc) return rc;
    return ffhip_lengths_read(SCRATCH_PNG_ENC + 1, stream, d_ver, n, out_len, status);
}

} // namespace

int ffhip_deflate_chunks_enqueue(const ffhip_def_stream *d_streams, const uint32_t *d_wg_item, unsigned long long total, void *stream)
{
    DefChunkArgs a;
    a.streams = d_streams; a.wg_item = d_wg_item; a.wg_base = 0;
    return ffhip_items_run(k_deflate_chunks, total, FFHIP_DEF_LANES, stream, a);
}

extern "C" int ffhip_deflate_streams_device(const uint8_t *const *d_src, const size_t *len, int n, uint8_t *const *d_dst, const size_t *cap,
                                            size_t *out_len, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!d_src || !len || !d_dst || !cap || !out_len || !status))) return FFHIP_EINVAL;
    for (int i = 0; i < n; i++) {
        if ((len[i] && !d_src[i]) || (cap[i] && !d_dst[i])) return FFHIP_EINVAL;
        if (len[i] >= ((size_t)1 << 32) || ffhip_deflate_bound(len[i]) >= ((size_t)1 << 32)) return FFHIP_EINVAL; /* sizes and offsets are held in 32 bits */
    }
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(nullptr) / 4; /* a byte of input takes six of scratch */
    return ffhip_parts_run(n, budget, FFHIP_PARTS_NO_CAP, [&](int i) { return len[i]; }, [&](int first, int cnt) {
        return deflate_part(d_src + first, len + first, cnt, d_dst + first, cap + first, out_len + first, status + first, stream);
    });
}
