/*
 * ffhip_png_enc_gpu.hip -- the PNG encoder on the device (include/ffpic_hip.h "PNG encoding").  The rule is
 * ffhip_png_enc_body.h's and ffhip_deflate_body.h's, shared with the host functions of ffhip_png_enc.c and ffhip_deflate.c.
 *   k_items_tables2   (ffhip_items.h) a workgroup per picture: its index over its rows (PeDesc) and its chunks (ffhip_def_stream) in the two
 *                     per-workgroup tables
 *   k_png_filter     a wave per row: the five sums of the adaptive choice by a wave reduction (the row above is read from the source again),
 *                     then the filtered row into the scratch, 16 bytes a store between the row's first and last 16-byte boundary
 *   k_deflate_chunks  (ffhip_deflate_gpu.hip) a wave per chunk of the filtered picture
 *   k_png_enc_scan    a workgroup per picture: the chunks' offsets in the file, every IDAT's CRC-32 from its bytes' CRC-32, the Adler parts
 *                     joined, the file's last 28 bytes, its size and the verdict
 *   k_png_enc_copy    a workgroup per chunk: its IDAT into the caller's buffer -- the first with signature and IHDR in front, the last with
 *                     the Adler IDAT and IEND behind -- every byte under cap
 * No kernel waits for another workgroup; every loop runs to a bound known at its entry.
 * The host side is the encoders' common one: ffhip_parts_run, ffhip_items_run, ffhip_lengths_read; encode_part's offsets are its own.
 */
#include "ffhip_items.h"
#include "ffhip_parts.h"
#include "ffhip_wave.h" /* wg_scan */
#include "ffhip_png_enc_internal.h"

#include <string.h>

#define PE_WG 256
#define PE_PART_ITEMS 4096 /* pictures of a part at most: the records and verdicts of a part stay small */

namespace {

struct PeDesc {
    ffhip_png_source src;
    uint8_t *filt, *d_out; /* the filtered picture in the scratch (16-byte aligned); the caller's buffer */
    unsigned long long cap, flen;
    u32 *chunk_off;        /* per chunk: where its IDAT starts in the file */
    u32 row_first, row_n;  /* its rows among the call's: k_png_filter's workgroups */
    int32_t filter;
    u32 pad;
    uint8_t header[40];    /* FFHIP_PE_HEADER bytes */
};
struct PeVerdict {
    unsigned long long file_len;
    int32_t status;
    u32 pad;
    uint8_t tail[32]; /* FFHIP_PE_TAIL bytes */
};

struct PeArgs {
    const PeDesc *desc;
    const ffhip_def_stream *streams;
    const u32 *wg_item;
    PeVerdict *verdict;
    u32 wg_base;
};

__global__ __launch_bounds__(64) void k_png_filter(PeArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const PeDesc &d = a.desc[item];
    const ffhip_png_source *s = &d.src;
    const int row = (int)(wg - d.row_first), lane = (int)threadIdx.x;
    const long long rb = (long long)s->width * s->channels;
    int type = d.filter;
    if (type == FFHIP_PNG_FILTER_ADAPTIVE) {
        u32 sums[5] = {0, 0, 0, 0, 0};
        for (long long j = lane; j < rb; j += 64) {
            int f[5];
            ffhip_pe_filter5(s, row, j, f);
#pragma unroll
            for (int t = 0; t < 5; t++) sums[t] += ffhip_pe_cost(f[t]);
        }
#pragma unroll
        for (int t = 0; t < 5; t++)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sums[t] += __shfl_xor(sums[t], off);
        type = ffhip_pe_choose(sums);
    }
    uint8_t *dst = d.filt + (long long)row * (rb + 1);
    if (lane == 0) dst[0] = (uint8_t)type;
    dst++;
    /* bytes up to the first 16-byte boundary, then 16 a store, then the rest */
    long long head = (long long)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > rb) head = rb;
    const long long groups = (rb - head) >> 4;
    for (long long j = lane; j < head; j += 64) {
        int f[5];
        ffhip_pe_filter5(s, row, j, f);
        dst[j] = (uint8_t)ffhip_pe_pick(f, type);
    }
    for (long long g = lane; g < groups; g += 64) {
        u32x4 w = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            int f[5];
            ffhip_pe_filter5(s, row, head + 16 * g + k, f);
            w[k >> 2] |= (u32)ffhip_pe_pick(f, type) << (8 * (k & 3));
        }
        *(u32x4 *)(dst + head + 16 * g) = w;
    }
    for (long long j = head + 16 * groups + lane; j < rb; j += 64) {
        int f[5];
        ffhip_pe_filter5(s, row, j, f);
        dst[j] = (uint8_t)ffhip_pe_pick(f, type);
    }
}

__global__ __launch_bounds__(PE_WG) void k_png_enc_scan(PeArgs a)
{
    __shared__ u32 wave_sum[PE_WG / 64];
    const PeDesc &d = a.desc[blockIdx.x];
    const ffhip_def_stream &s = a.streams[blockIdx.x];
    unsigned long long carry = FFHIP_PE_HEADER;
    const u32 turns = (s.n_wgs + PE_WG - 1) / PE_WG;
    for (u32 turn = 0; turn < turns; turn++) {
        const u32 c = turn * PE_WG + threadIdx.x;
        u32 v = 0;
        if (c < s.n_wgs) {
            const u32 n = s.res[c].out_len;
            v = ffhip_pe_idat_size(c == 0, n);
            s.res[c].crc = ffhip_pe_idat_crc(c == 0, n, s.res[c].crc); /* from the bytes' to the chunk's */
        }
        u32 total;
        const u32 before = wg_scan<PE_WG>(v, wave_sum, &total);
        if (c < s.n_wgs) d.chunk_off[c] = (u32)carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        u32 x = 1, y = 0;
        for (u32 c = 0; c < s.n_wgs; c++) {
            const unsigned long long left = s.len - (unsigned long long)c * FFHIP_DEF_CHUNK;
            ffhip_def_adler_join(&x, &y, s.res[c].adler_a, s.res[c].adler_b, left < FFHIP_DEF_CHUNK ? left : FFHIP_DEF_CHUNK);
        }
        PeVerdict &r = a.verdict[blockIdx.x];
        ffhip_pe_tail(x, y, r.tail);
        r.file_len = carry + FFHIP_PE_TAIL;
        r.status = r.file_len > d.cap ? FFHIP_EPNG_NOSPACE : FFHIP_OK;
    }
}

__global__ __launch_bounds__(PE_WG) void k_png_enc_copy(PeArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const PeDesc &d = a.desc[item];
    const ffhip_def_stream &s = a.streams[item];
    const u32 c = wg - s.first_wg, n = s.res[c].out_len;
    const int first = c == 0, hn = ffhip_pe_idat_head_len(first);
    const unsigned long long at = d.chunk_off[c];
    const uint8_t *from = (const uint8_t *)(s.out + (size_t)c * (FFHIP_DEF_OUT_BYTES / 4));
    uint8_t *out = d.d_out;
    if ((int)threadIdx.x < hn && at + threadIdx.x < d.cap) out[at + threadIdx.x] = ffhip_pe_idat_head_byte(first, n, (int)threadIdx.x);
    for (u32 k = threadIdx.x; k < n; k += PE_WG)
        if (at + hn + k < d.cap) out[at + hn + k] = from[k];
    if (threadIdx.x < 4 && at + hn + n + threadIdx.x < d.cap) out[at + hn + n + threadIdx.x] = (uint8_t)(s.res[c].crc >> (24 - 8 * threadIdx.x));
    if (first && threadIdx.x < FFHIP_PE_HEADER && threadIdx.x < d.cap) out[threadIdx.x] = d.header[threadIdx.x];
    if (c == s.n_wgs - 1 && threadIdx.x < FFHIP_PE_TAIL) {
        const PeVerdict &r = a.verdict[item];
        const unsigned long long o = r.file_len - FFHIP_PE_TAIL + threadIdx.x;
        if (o < d.cap) out[o] = r.tail[threadIdx.x];
    }
}

bool item_ok(const ffhip_png_encode_item &it)
{
    if (it.reserved != 0 || !ffhip_pngenc_source_ok(&it.src, it.filter) || (it.cap && !it.d_out)) return false;
    /* the stated limit: sizes and offsets within a file are held in 32 bits */
    return ffhip_png_encode_bound(it.src.width, it.src.height, it.src.channels) < ((size_t)1 << 32);
}

/* the pictures of one part: one synchronisation */
int encode_part(const ffhip_png_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<PeDesc> desc((size_t)n);
    std::vector<ffhip_def_stream> rec((size_t)n);
    std::vector<size_t> filt_at((size_t)n);
    unsigned long long total_rows = 0, total_chunks = 0;
    size_t filt_bytes = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_png_encode_item &it = items[i];
        PeDesc &d = desc[(size_t)i];
        ffhip_def_stream &s = rec[(size_t)i];
        memset(&d, 0, sizeof(d));
        memset(&s, 0, sizeof(s));
        d.src = it.src; d.filter = it.filter; d.d_out = it.d_out; d.cap = it.cap;
        d.flen = ffhip_pe_filtered_len(it.src.width, it.src.height, it.src.channels);
        d.row_first = (u32)total_rows; d.row_n = (u32)it.src.height;
        ffhip_pngenc_header(it.src.width, it.src.height, it.src.channels, d.header);
        s.len = d.flen;
        s.first_wg = (u32)total_chunks; s.n_wgs = (u32)ffhip_def_chunks(d.flen);
        total_rows += d.row_n; total_chunks += s.n_wgs;
        filt_at[(size_t)i] = filt_bytes;
        filt_bytes += ffhip_up((size_t)d.flen, 16);
    }
    if (total_rows > 0xffffffffULL || total_chunks > 0xffffffffULL) return FFHIP_EINVAL;
    /* the scratch: picture and stream records (uploaded), the two per-workgroup tables, offsets, results, verdicts, the chunks' output words
     * (zeroed), the filtered pictures, the tokens */
    const size_t desc_bytes = (size_t)n * sizeof(PeDesc), up_bytes = desc_bytes + (size_t)n * sizeof(ffhip_def_stream);
    const size_t table_words = (size_t)total_rows + (size_t)total_chunks;
    const size_t off_off = up_bytes + table_words * 4, res_off = off_off + (size_t)total_chunks * 4;
    const size_t ver_off = ffhip_up(res_off + (size_t)total_chunks * sizeof(ffhip_def_result), 8);
    const size_t out_off = ffhip_up(ver_off + (size_t)n * sizeof(PeVerdict), 256), out_bytes = (size_t)total_chunks * FFHIP_DEF_OUT_BYTES;
    const size_t filt_off = ffhip_up(out_off + out_bytes, 256), tok_off = filt_off + filt_bytes, end = tok_off + filt_bytes * 4;
    std::vector<uint8_t> up(up_bytes);
    uint8_t *dev = nullptr;
    int rc = ffhip_items_stage(SCRATCH_PNG_ENC, stream, up.data(), up_bytes, table_words, end - up_bytes - table_words * 4, &dev, [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            PeDesc &d = desc[(size_t)i];
            ffhip_def_stream &s = rec[(size_t)i];
            d.filt = base + filt_off + filt_at[(size_t)i];
            d.chunk_off = (u32 *)(base + off_off) + s.first_wg;
            s.src = d.filt;
            s.tok = (u32 *)(base + tok_off) + filt_at[(size_t)i];
            s.out = (u32 *)(base + out_off + (size_t)s.first_wg * FFHIP_DEF_OUT_BYTES);
            s.res = (ffhip_def_result *)(base + res_off) + s.first_wg;
        }
        memcpy(up.data(), desc.data(), desc_bytes);
        memcpy(up.data() + desc_bytes, rec.data(), up_bytes - desc_bytes);
    });
    if (rc) return rc;
    PeArgs a;
    a.desc = (const PeDesc *)dev; a.streams = (const ffhip_def_stream *)(dev + desc_bytes); a.verdict = (PeVerdict *)(dev + ver_off);
    u32 *d_row_item = (u32 *)(dev + up_bytes), *d_chunk_item = d_row_item + total_rows;
    FFHIP_CHECK(hipMemsetAsync(dev + out_off, 0, out_bytes, st), FFHIP_EIO);
    hipLaunchKernelGGL((k_items_tables2<PeDesc, ffhip_def_stream, &PeDesc::row_first, &PeDesc::row_n, &ffhip_def_stream::first_wg, &ffhip_def_stream::n_wgs>),
                       dim3((unsigned)n), dim3(256), 0, st, a.desc, a.streams, d_row_item, d_chunk_item);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    a.wg_item = d_row_item;
    rc = ffhip_items_run(k_png_filter, total_rows, 64, stream, a);
    if (rc) return rc;
    rc = ffhip_deflate_chunks_enqueue(a.streams, d_chunk_item, total_chunks, stream);
    if (rc) return rc;
    a.wg_item = d_chunk_item; a.wg_base = 0;
    hipLaunchKernelGGL(k_png_enc_scan, dim3((unsigned)n), dim3(PE_WG), 0, st, a);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_png_enc_copy, total_chunks, PE_WG, stream, a);
    if (rc) return rc;
    return ffhip_lengths_read(SCRATCH_PNG_ENC + 1, stream, a.verdict, n, len_out, status);
}

} // namespace

extern "C" int ffhip_png_encode_items(const ffhip_png_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!items || !len_out || !status))) return FFHIP_EINVAL;
    for (int i = 0; i < n; i++)
        if (!item_ok(items[i])) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(nullptr) / 4; /* a filtered byte takes six of scratch: itself, its token word, its chunk's output */
    /* a part: up to PE_PART_ITEMS pictures while their filtered bytes fit the budget */
    return ffhip_parts_run(n, budget, PE_PART_ITEMS,
                           [&](int i) { return (size_t)ffhip_pe_filtered_len(items[i].src.width, items[i].src.height, items[i].src.channels); },
                           [&](int first, int cnt) { return encode_part(items + first, cnt, len_out + first, status + first, stream); });
}
