/*
 * ffhip_vp8l_enc_gpu.hip -- the lossless WebP encoder on the device (include/ffpic_hip.h "Lossless WebP encoding").  The
 * rule is ffhip_vp8l_enc_body.h's, shared with the host functions of ffhip_vp8l_enc.c.
 *   k_items_tables2     (ffhip_items.h) a workgroup per picture: its index over its tiles and its chunks in the two per-workgroup tables
 *   k_vp8l_enc_predict  a wave per tile: the 14 sums of the choice by a wave reduction (neighbours are read from the source again), the mode
 *                       into the sub-image, the residual words into the scratch picture, 16 bytes a store where the row allows
 *   k_vp8l_enc_parse    a wave per chunk: candidates, the uniform greedy walk, a token word a position in scratch, the histogram in LDS and
 *                       from there by integer atomics into the picture's counters
 *   k_vp8l_enc_codes    a wave per picture: lengths and codes of both groups, the file's head as bits, the table of codes, the first chunk's bit
 *   k_vp8l_enc_count    a wave per chunk: its tokens' bits
 *   k_vp8l_enc_scan     a workgroup per picture: the chunks' bit positions (a prefix scan in a loop of its own), the sizes, the verdict
 *   k_vp8l_enc_write    a wave per chunk: its tokens' bits by atomicOr at a wave prefix sum's positions into the file's zeroed words
 *   k_vp8l_enc_copy     a workgroup per chunk: its share of the file into the caller's buffer, every byte under cap
 * No kernel waits for another workgroup; every loop runs to a bound known at its entry.
 * The host side is the encoders' common one: ffhip_parts_run, ffhip_items_run, ffhip_lengths_read; encode_part's offsets are its own.
 */
#include "ffhip_items.h"
#include "ffhip_parts.h"
#include "ffhip_wave.h" /* wg_scan */
#include "ffhip_vp8l_enc_internal.h"

#include <string.h>

#define VE_WG 256
#define VE_PART_ITEMS 4096 /* pictures of a part at most */

namespace {

struct VeDesc {
    ffhip_png_source src;
    uint8_t *d_out;
    unsigned long long cap, pixels, words_bytes; /* words_bytes: the file's zeroed words, a multiple of 16 */
    u32 *res, *tok;            /* the residual picture (16-byte aligned) and the token words */
    uint8_t *modes;            /* the sub-image: a byte a tile */
    u32 *hist, *table, *words; /* the counters (zeroed), the table of codes, the file (zeroed) */
    u32 *chunk_bits;
    unsigned long long *chunk_pos;
    u32 tile_first, tile_n, tiles_x;
    u32 first_wg, n_wgs;       /* its chunks among the call's */
    int32_t flags;
};
struct VeVerdict {
    unsigned long long file_len, head_bits;
    int32_t status;
    u32 pad;
};
struct VeArgs {
    const VeDesc *desc;
    const u32 *wg_item;
    VeVerdict *verdict;
    u32 wg_base;
};

__global__ __launch_bounds__(64) void k_vp8l_enc_predict(VeArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const VeDesc &d = a.desc[item];
    const ffhip_png_source *s = &d.src;
    const int flags = d.flags, lane = (int)threadIdx.x, w = s->width, h = s->height;
    const u32 t = wg - d.tile_first;
    const int x0 = (int)(t % d.tiles_x) << FFHIP_VP8L_ENC_TILE_BITS, y0 = (int)(t / d.tiles_x) << FFHIP_VP8L_ENC_TILE_BITS;
    const int tw = w - x0 < FFHIP_VE_TILE ? w - x0 : FFHIP_VE_TILE, th = h - y0 < FFHIP_VE_TILE ? h - y0 : FFHIP_VE_TILE;
    int mode = 0;
    if (flags & FFHIP_VP8L_ENC_PREDICT) {
        u32 sums[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = lane; i < tw * th; i += 64) ffhip_ve_costs(s, flags, x0 + i % tw, y0 + i / tw, sums);
#pragma unroll
        for (int k = 0; k < 14; k++)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sums[k] += __shfl_xor(sums[k], off);
        mode = ffhip_ve_choose(sums);
        if (lane == 0) d.modes[t] = (uint8_t)mode;
    }
    /* groups of four pixels of a row: one store where the four lie inside the row at a 16-byte boundary of the residual picture */
    const int gw = (tw + 3) >> 2;
    for (int g = lane; g < gw * th; g += 64) {
        const int y = y0 + g / gw, x = x0 + 4 * (g % gw), cnt = x0 + tw - x < 4 ? x0 + tw - x : 4;
        const long long idx = (long long)y * w + x;
        u32x4 r = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < cnt) r[k] = ffhip_ve_residual(s, flags, mode, x + k, y);
        if (cnt == 4 && !(idx & 3))
            *(u32x4 *)(d.res + idx) = r;
        else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) d.res[idx + k] = r[k];
        }
    }
}

__global__ __launch_bounds__(FFHIP_DEF_LANES) void k_vp8l_enc_parse(VeArgs a)
{
    __shared__ ffhip_ve_parse_store m;
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const VeDesc &d = a.desc[item];
    const unsigned long long at = (unsigned long long)(wg - d.first_wg) * FFHIP_VE_CHUNK, left = d.pixels - at;
    ffhip_ve_parse(&m, d.res, at, (u32)(left < FFHIP_VE_CHUNK ? left : FFHIP_VE_CHUNK), (u32)d.src.width, d.tok + at, d.hist);
}

__global__ __launch_bounds__(FFHIP_DEF_LANES) void k_vp8l_enc_codes(VeArgs a)
{
    __shared__ ffhip_ve_codes_store m;
    const VeDesc &d = a.desc[blockIdx.x];
    const unsigned long long pos = ffhip_ve_codes(&m, (u32)d.src.width, (u32)d.src.height, d.src.channels == 2 || d.src.channels == 4, d.flags, d.modes,
                                                  d.hist, d.words, d.table);
    if (threadIdx.x == 0) a.verdict[blockIdx.x].head_bits = pos;
}

/* the picture's table of codes into LDS */
__device__ static inline void load_table(u32 *table, const u32 *from)
{
    for (int k = (int)threadIdx.x; k < FFHIP_VE_NSYM; k += FFHIP_DEF_LANES) table[k] = from[k];
    __syncthreads();
}

__global__ __launch_bounds__(FFHIP_DEF_LANES) void k_vp8l_enc_count(VeArgs a)
{
    __shared__ u32 table[FFHIP_VE_NSYM], lanes[FFHIP_DEF_LANES + 4];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const VeDesc &d = a.desc[item];
    const u32 c = wg - d.first_wg;
    const unsigned long long at = (unsigned long long)c * FFHIP_VE_CHUNK, left = d.pixels - at;
    load_table(table, d.table);
    const u32 bits = ffhip_ve_count(lanes, table, d.res + at, d.tok + at, (u32)(left < FFHIP_VE_CHUNK ? left : FFHIP_VE_CHUNK), (u32)d.src.width);
    if (threadIdx.x == 0) d.chunk_bits[c] = bits;
}

__global__ __launch_bounds__(VE_WG) void k_vp8l_enc_scan(VeArgs a)
{
    __shared__ u32 wave_sum[VE_WG / 64];
    const VeDesc &d = a.desc[blockIdx.x];
    VeVerdict &r = a.verdict[blockIdx.x];
    unsigned long long carry = r.head_bits;
    const u32 turns = (d.n_wgs + VE_WG - 1) / VE_WG;
    for (u32 turn = 0; turn < turns; turn++) {
        const u32 c = turn * VE_WG + threadIdx.x;
        const u32 v = c < d.n_wgs ? d.chunk_bits[c] : 0u; /* a turn's sum: 256 x 4096 x 60 bits at most */
        u32 total;
        const u32 before = wg_scan<VE_WG>(v, wave_sum, &total);
        if (c < d.n_wgs) d.chunk_pos[c] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        r.file_len = ffhip_ve_finish(d.words, carry);
        r.status = r.file_len > d.cap ? FFHIP_EVP8L_NOSPACE : FFHIP_OK;
    }
}

__global__ __launch_bounds__(FFHIP_DEF_LANES) void k_vp8l_enc_write(VeArgs a)
{
    __shared__ u32 table[FFHIP_VE_NSYM], lanes[FFHIP_DEF_LANES + 4];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const VeDesc &d = a.desc[item];
    const u32 c = wg - d.first_wg;
    const unsigned long long at = (unsigned long long)c * FFHIP_VE_CHUNK, left = d.pixels - at;
    load_table(table, d.table);
    ffhip_ve_write(lanes, table, d.res + at, d.tok + at, (u32)(left < FFHIP_VE_CHUNK ? left : FFHIP_VE_CHUNK), (u32)d.src.width, d.words, d.chunk_pos[c]);
}

/* chunk c's share of the file: the 16-byte pieces [c x share, (c + 1) x share) of the words, below the file's size and below cap */
__global__ __launch_bounds__(VE_WG) void k_vp8l_enc_copy(VeArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const VeDesc &d = a.desc[item];
    const u32 c = wg - d.first_wg;
    const unsigned long long pieces = d.words_bytes >> 4, share = (pieces + d.n_wgs - 1) / d.n_wgs;
    const unsigned long long len = a.verdict[item].file_len, end = len < d.cap ? len : d.cap;
    const unsigned long long p1 = (c + 1ull) * share < pieces ? (c + 1ull) * share : pieces;
    const uint8_t *from = (const uint8_t *)d.words;
    for (unsigned long long p = c * share + threadIdx.x; p < p1; p += VE_WG) {
        const unsigned long long o = p << 4;
        if (o >= end) break;
        const u32x4 v = *(const u32x4 *)(from + o);
        if (o + 16 <= end && !((uintptr_t)(d.d_out + o) & 15))
            *(u32x4 *)(d.d_out + o) = v;
        else
            for (int k = 0; k < 16 && o + k < end; k++) d.d_out[o + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
}

bool item_ok(const ffhip_vp8l_encode_item &it)
{
    return it.reserved == 0 && ffhip_vp8lenc_source_ok(&it.src, it.flags) && !(it.cap && !it.d_out);
}

/* the pictures of one part: one synchronisation */
int encode_part(const ffhip_vp8l_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<VeDesc> desc((size_t)n);
    std::vector<size_t> px_at((size_t)n), words_at((size_t)n);
    unsigned long long total_tiles = 0, total_chunks = 0;
    size_t px_words = 0, words_bytes = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_vp8l_encode_item &it = items[i];
        VeDesc &d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        const u32 w = (u32)it.src.width, h = (u32)it.src.height;
        d.src = it.src; d.flags = it.flags; d.d_out = it.d_out; d.cap = it.cap;
        d.pixels = (unsigned long long)w * h;
        d.words_bytes = ffhip_up((size_t)ffhip_ve_bound(w, h) + 16, 16);
        d.tiles_x = ffhip_ve_sub_size(w);
        d.tile_first = (u32)total_tiles; d.tile_n = d.tiles_x * ffhip_ve_sub_size(h);
        d.first_wg = (u32)total_chunks; d.n_wgs = (u32)ffhip_ve_chunks(d.pixels);
        total_tiles += d.tile_n; total_chunks += d.n_wgs;
        px_at[(size_t)i] = px_words; px_words += ffhip_up((size_t)d.pixels, 4);
        words_at[(size_t)i] = words_bytes; words_bytes += (size_t)d.words_bytes;
    }
    if (total_tiles > 0xffffffffULL || total_chunks > 0xffffffffULL) return FFHIP_EINVAL;
    /* the scratch: the picture records (uploaded), the two per-workgroup tables, the chunks' bits, the tables of codes, the chunks' positions,
     * the verdicts, the modes, then -- zeroed by the call -- the counters and the files' words, then the residual pictures and the tokens */
    const size_t up_bytes = (size_t)n * sizeof(VeDesc), table_words = (size_t)total_tiles + (size_t)total_chunks;
    const size_t bits_off = up_bytes + table_words * 4, code_off = bits_off + (size_t)total_chunks * 4;
    const size_t pos_off = ffhip_up(code_off + (size_t)n * FFHIP_VE_NSYM * 4, 8), ver_off = pos_off + (size_t)total_chunks * 8;
    const size_t mode_off = ver_off + (size_t)n * sizeof(VeVerdict);
    const size_t hist_off = ffhip_up(mode_off + (size_t)total_tiles, 256), words_off = ffhip_up(hist_off + (size_t)n * FFHIP_VE_NSYM * 4, 256);
    const size_t res_off = ffhip_up(words_off + words_bytes, 256), tok_off = res_off + px_words * 4, end = tok_off + px_words * 4;
    std::vector<uint8_t> upl(up_bytes);
    uint8_t *dev = nullptr;
    int rc = ffhip_items_stage(SCRATCH_VP8L_ENC, stream, upl.data(), up_bytes, table_words, end - up_bytes - table_words * 4, &dev, [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            VeDesc &d = desc[(size_t)i];
            d.res = (u32 *)(base + res_off) + px_at[(size_t)i];
            d.tok = (u32 *)(base + tok_off) + px_at[(size_t)i];
            d.modes = base + mode_off + d.tile_first;
            d.hist = (u32 *)(base + hist_off) + (size_t)i * FFHIP_VE_NSYM;
            d.table = (u32 *)(base + code_off) + (size_t)i * FFHIP_VE_NSYM;
            d.words = (u32 *)(base + words_off + words_at[(size_t)i]);
            d.chunk_bits = (u32 *)(base + bits_off) + d.first_wg;
            d.chunk_pos = (unsigned long long *)(base + pos_off) + d.first_wg;
        }
        memcpy(upl.data(), desc.data(), up_bytes);
    });
    if (rc) return rc;
    VeArgs a;
    a.desc = (const VeDesc *)dev; a.verdict = (VeVerdict *)(dev + ver_off);
    u32 *d_tile_item = (u32 *)(dev + up_bytes), *d_chunk_item = d_tile_item + total_tiles;
    FFHIP_CHECK(hipMemsetAsync(dev + hist_off, 0, res_off - hist_off, st), FFHIP_EIO);
    hipLaunchKernelGGL((k_items_tables2<VeDesc, VeDesc, &VeDesc::tile_first, &VeDesc::tile_n, &VeDesc::first_wg, &VeDesc::n_wgs>),
                       dim3((unsigned)n), dim3(256), 0, st, a.desc, a.desc, d_tile_item, d_chunk_item);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    a.wg_item = d_tile_item;
    rc = ffhip_items_run(k_vp8l_enc_predict, total_tiles, 64, stream, a);
    if (rc) return rc;
    a.wg_item = d_chunk_item;
    rc = ffhip_items_run(k_vp8l_enc_parse, total_chunks, FFHIP_DEF_LANES, stream, a);
    if (rc) return rc;
    a.wg_base = 0;
    hipLaunchKernelGGL(k_vp8l_enc_codes, dim3((unsigned)n), dim3(FFHIP_DEF_LANES), 0, st, a);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_vp8l_enc_count, total_chunks, FFHIP_DEF_LANES, stream, a);
    if (rc) return rc;
    a.wg_base = 0;
    hipLaunchKernelGGL(k_vp8l_enc_scan, dim3((unsigned)n), dim3(VE_WG), 0, st, a);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_vp8l_enc_write, total_chunks, FFHIP_DEF_LANES, stream, a);
    if (rc) return rc;
    rc = ffhip_items_run(k_vp8l_enc_copy, total_chunks, VE_WG, stream, a);
    if (rc) return rc;
    return ffhip_lengths_read(SCRATCH_VP8L_ENC + 1, stream, a.verdict, n, len_out, status);
}

} // namespace

extern "C" int ffhip_vp8l_encode_items(const ffhip_vp8l_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!items || !len_out || !status))) return FFHIP_EINVAL;
    for (int i = 0; i < n; i++)
        if (!item_ok(items[i])) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(nullptr) / 16; /* a pixel takes sixteen bytes of scratch: its residual word, its token word, 7.5 of the file */
    /* a part: up to VE_PART_ITEMS pictures while their pixels fit the budget */
    return ffhip_parts_run(n, budget, VE_PART_ITEMS, [&](int i) { return (size_t)items[i].src.width * (size_t)items[i].src.height; },
                           [&](int first, int cnt) { return encode_part(items + first, cnt, len_out + first, status + first, stream); });
}
