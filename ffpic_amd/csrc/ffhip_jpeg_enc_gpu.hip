/*
 * ffhip_jpeg_enc_gpu.hip -- the baseline JPEG encoder on the device (include/ffpic_hip.h "JPEG encoding").  The rule is
 * ffhip_jpeg_enc_body.h's, shared with the host functions of ffhip_jpeg_enc.c.
 *
 * PIXELS TO COEFFICIENTS (ffhip_jpeg_fdct_items), ffhip_jpeg_libjpeg.hip in the other direction:
 *   k_jpeg_color_downsample  a thread takes the 8 h x v pixels over 8 chroma samples of one chroma row (grey: 8 pixels of a row): RGB to
 *                            YCbCr, the means, 8-byte stores into the padded RASTER uint8 planes; the lanes of a wave take neighbouring units
 *   k_jpeg_fdct_islow        a thread takes one block of any component, dummy blocks included: 8 x 8-byte loads, both passes and the
 *                            quantiser in registers, 8 x 16-byte stores of int16 in MCU order (a wave's stores are one run of 8 KiB)
 * COEFFICIENTS TO FILES (ffhip_jpeg_huff_encode_items):
 *   k_jenc_blocks<false>  a thread per block of the scan: its bits (the DC predecessor is read from the planes)
 *   k_jenc_positions      a workgroup per picture: the blocks' bit positions in the unstuffed stream, a prefix scan of je_span in a loop of its own
 *   (the host reads the streams' sizes and sizes the scratch)
 *   k_jenc_blocks<true>   a thread per block: its bits into the zeroed stream; an interval's last block adds padding and marker
 *   k_jenc_ff_count       a workgroup per KiB of stream: the FF bytes that get a 00
 *   k_jenc_ff_scan        a workgroup per picture: their prefix sums, the file's size, the item's verdict
 *   k_jenc_copy           a workgroup per KiB of stream: header and stuffed stream into the caller's buffer, every byte under cap
 * No kernel waits for another workgroup; every loop runs to a bound known at its entry.
 * The host side is the encoders' common one: ffhip_parts_run cuts ffhip_jpeg_encode_items into parts, k_items_tables2 writes
 * the colour and FDCT tables, ffhip_items_run launches, ffhip_records_fetch is the first synchronisation, ffhip_lengths_read the second.
 */
#include "ffhip_items.h"
#include "ffhip_parts.h"
#include "ffhip_wave.h" /* wg_scan */
#include "ffhip_jpeg_enc_internal.h"

#include <string.h>

#define JE_WG 256
#define JE_CHUNK 1024 /* bytes of unstuffed stream a workgroup of k_jenc_ff_count and k_jenc_copy takes */
#define G(T) __attribute__((address_space(1))) T

namespace {

/* ------------------------------------------------------------------------------------------------ pixels to coefficients */
struct JencDesc {
    const uint8_t *pixels;
    int64_t row_stride, pixel_stride, c0, c1, c2;
    int32_t channels, width, height, layout;
    int32_t mcu_cols, mcu_rows;
    uint8_t *plane_y, *plane_u, *plane_v; /* padded raster planes in the scratch */
    int16_t *coef_y, *coef_u, *coef_v;
    u32 color_first_wg, color_n_wgs; /* k_jpeg_color_downsample: 8 mcus units */
    u32 fdct_first_wg, fdct_n_wgs, wg_u, wg_v; /* k_jpeg_fdct_islow: luma, then Cb, then Cr */
    uint16_t quant[128];
};

struct JencArgs {
    const JencDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
};

/* pixel (col, row) of the source, both inside the picture */
__device__ __forceinline__ void load_rgb(const JencDesc &d, int col, int row, int &r, int &g, int &b)
{
    G(const uint8_t) *p = (G(const uint8_t) *)d.pixels + (long long)row * d.row_stride + (long long)col * d.pixel_stride;
    if (d.channels == 4) {
        const u32 w = *(G(const u32) *)p;
        b = (int)(w & 255u); g = (int)((w >> 8) & 255u); r = (int)((w >> 16) & 255u);
    } else {
        r = p[d.c0]; g = p[d.c1]; b = p[d.c2];
    }
}

__device__ __forceinline__ u32x2 pack8(const int *s)
{
    u32x2 w;
    w[0] = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
    w[1] = (u32)s[4] | ((u32)s[5] << 8) | ((u32)s[6] << 16) | ((u32)s[7] << 24);
    return w;
}

/* the unit (ux, cy) of a colour picture: 8 H columns from 8 H ux, the V rows under chroma row cy */
template <int H, int V> __device__ __forceinline__ void color_unit(const JencDesc &d, int ux, int cy)
{
    const long long yw = 8LL * H * d.mcu_cols, cw = 8LL * d.mcu_cols;
    int cb[V][8 * H], cr[V][8 * H];
#pragma unroll
    for (int dy = 0; dy < V; dy++) {
        const int y = cy * V + dy, row_l = je_luma_src_row(y, d.height), row_c = je_chroma_src_row(cy, dy, d.height, V);
        int lum[8 * H];
#pragma unroll
        for (int k = 0; k < 8 * H; k++) {
            int r, g, b;
            load_rgb(d, je_src_col(ux * 8 * H + k, d.width), row_l, r, g, b);
            je_ycc(r, g, b, &lum[k], &cb[dy][k], &cr[dy][k]);
        }
        if (row_c != row_l) { /* chroma rows beyond the last downsampled row repeat THAT row, not the picture's last row (step 3) */
#pragma unroll
            for (int k = 0; k < 8 * H; k++) {
                int r, g, b, unused;
                load_rgb(d, je_src_col(ux * 8 * H + k, d.width), row_c, r, g, b);
                je_ycc(r, g, b, &unused, &cb[dy][k], &cr[dy][k]);
            }
        }
        G(uint8_t) *dst = (G(uint8_t) *)d.plane_y + (long long)y * yw + (long long)ux * 8 * H;
#pragma unroll
        for (int k = 0; k < H; k++) *(G(u32x2) *)(dst + 8 * k) = pack8(lum + 8 * k);
    }
    int u[8], w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int cx = ux * 8 + k;
        if (H == 2 && V == 2) {
            u[k] = je_h2v2(cb[0][2 * k], cb[0][2 * k + 1], cb[V - 1][2 * k], cb[V - 1][2 * k + 1], cx);
            w[k] = je_h2v2(cr[0][2 * k], cr[0][2 * k + 1], cr[V - 1][2 * k], cr[V - 1][2 * k + 1], cx);
        } else if (H == 2) {
            u[k] = je_h2v1(cb[0][2 * k], cb[0][2 * k + 1], cx);
            w[k] = je_h2v1(cr[0][2 * k], cr[0][2 * k + 1], cx);
        } else {
            u[k] = cb[0][k];
            w[k] = cr[0][k];
        }
    }
    *(G(u32x2) *)((G(uint8_t) *)d.plane_u + (long long)cy * cw + (long long)ux * 8) = pack8(u);
    *(G(u32x2) *)((G(uint8_t) *)d.plane_v + (long long)cy * cw + (long long)ux * 8) = pack8(w);
}

__global__ __launch_bounds__(JE_WG) void k_jpeg_color_downsample(JencArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JencDesc &d = a.desc[item];
    const unsigned long long idx = (unsigned long long)(wg - d.color_first_wg) * JE_WG + threadIdx.x;
    const unsigned long long units = 8ULL * (unsigned long long)d.mcu_cols * (unsigned long long)d.mcu_rows;
    if (idx >= units) return; /* nothing is loaded or stored beyond the planes */
    const int cy = (int)(idx / (u32)d.mcu_cols), ux = (int)(idx - (unsigned long long)cy * (u32)d.mcu_cols);
    if (d.layout == FFHIP_JPEG_ENC_GREY) {
        int s[8];
        const int row = je_luma_src_row(cy, d.height);
#pragma unroll
        for (int k = 0; k < 8; k++)
            s[k] = ((G(const uint8_t) *)d.pixels)[(long long)row * d.row_stride + (long long)je_src_col(ux * 8 + k, d.width) * d.pixel_stride + d.c0];
        *(G(u32x2) *)((G(uint8_t) *)d.plane_y + (long long)cy * (8LL * d.mcu_cols) + (long long)ux * 8) = pack8(s);
    } else if (d.layout == FFHIP_JPEG_ENC_444) color_unit<1, 1>(d, ux, cy);
    else if (d.layout == FFHIP_JPEG_ENC_422) color_unit<2, 1>(d, ux, cy);
    else color_unit<2, 2>(d, ux, cy);
}

__global__ __launch_bounds__(JE_WG) void k_jpeg_fdct_islow(JencArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JencDesc &d = a.desc[item];
    const u32 local = wg - d.fdct_first_wg;
    const int comp = local >= d.wg_v ? 2 : (local >= d.wg_u ? 1 : 0);
    const u32 first = comp == 2 ? d.wg_v : (comp == 1 ? d.wg_u : 0u);
    const int h = comp ? 1 : je_layout_h(d.layout), v = comp ? 1 : je_layout_v(d.layout), hv = h * v;
    const unsigned long long mcus = (unsigned long long)d.mcu_cols * (unsigned long long)d.mcu_rows;
    const unsigned long long b = (unsigned long long)(local - first) * JE_WG + threadIdx.x; /* the thread's block, MCU order */
    if (b >= mcus * (unsigned)hv) return;
    const unsigned long long mcu = b / (unsigned)hv;
    const int j = (int)(b - mcu * (unsigned)hv);
    const int my = (int)(mcu / (u32)d.mcu_cols), mx = (int)(mcu - (unsigned long long)my * (u32)d.mcu_cols);
    const int sj = comp ? 0 : je_dc_source(j, mx, my, h, v, d.width, d.height); /* a dummy block takes a block in front of it (step 4) */
    const long long bx = (long long)mx * h + sj % h, by = (long long)my * v + sj / h;
    const long long stride = 8LL * h * d.mcu_cols;
    G(const uint8_t) *src = (G(const uint8_t) *)(comp == 2 ? d.plane_v : (comp == 1 ? d.plane_u : d.plane_y)) + by * 8 * stride + bx * 8;
    int32_t s[64];
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const u32x2 w = *(G(const u32x2) *)(src + y * stride);
#pragma unroll
        for (int k = 0; k < 8; k++) s[8 * y + k] = (int32_t)((w[k >> 2] >> (8 * (k & 3))) & 255u);
    }
    je_fdct_quant(s, d.quant + (comp ? 64 : 0));
    if (sj != j) {
#pragma unroll
        for (int k = 1; k < 64; k++) s[k] = 0;
    }
    G(int16_t) *dst = (G(int16_t) *)(comp == 2 ? d.coef_v : (comp == 1 ? d.coef_u : d.coef_y)) + (long long)b * 64;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        u32x4 w;
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = ((u32)s[8 * y + 2 * k] & 0xffffu) | ((u32)s[8 * y + 2 * k + 1] << 16);
        *(G(u32x4) *)(dst + 8 * y) = w;
    }
}

bool fdct_item_ok(const ffhip_jpeg_fdct_item &it)
{
    if (!ffhip_jenc_source_ok(&it.src, it.layout)) return false;
    if (!it.d_coef_y || ((uintptr_t)it.d_coef_y & 15)) return false;
    if (it.layout == FFHIP_JPEG_ENC_GREY) return !it.d_coef_u && !it.d_coef_v;
    return it.d_coef_u && it.d_coef_v && !((uintptr_t)it.d_coef_u & 15) && !((uintptr_t)it.d_coef_v & 15);
}

int fdct_items_impl(const ffhip_jpeg_fdct_item *items, int n, void *stream, bool checked)
{
    if (n < 0 || (n > 0 && !items)) return FFHIP_EINVAL;
    std::vector<JencDesc> desc((size_t)n);
    std::vector<size_t> plane_at((size_t)n);
    unsigned long long total_color = 0, total_fdct = 0;
    size_t plane_bytes = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_fdct_item &it = items[i];
        if (!checked && !fdct_item_ok(it)) return FFHIP_EINVAL;
        ffhip_jenc_geometry g;
        ffhip_jenc_geom(it.src.width, it.src.height, it.layout, &g);
        JencDesc &d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.pixels = it.src.pixels; d.row_stride = it.src.row_stride; d.pixel_stride = it.src.pixel_stride;
        d.c0 = it.src.chan[0]; d.c1 = it.src.chan[1]; d.c2 = it.src.chan[2];
        d.channels = it.src.channels; d.width = it.src.width; d.height = it.src.height; d.layout = it.layout;
        d.mcu_cols = g.mcu_cols; d.mcu_rows = g.mcu_rows;
        d.coef_y = it.d_coef_y; d.coef_u = it.d_coef_u; d.coef_v = it.d_coef_v;
        ffhip_jpeg_encode_tables(it.quality, d.quant);
        const unsigned long long mcus = (unsigned long long)g.mcus, yblocks = mcus * (unsigned)(g.h * g.v);
        const u32 wy = (u32)((yblocks + JE_WG - 1) / JE_WG), wc = g.ncomp == 3 ? (u32)((mcus + JE_WG - 1) / JE_WG) : 0u;
        d.color_first_wg = (u32)total_color; d.color_n_wgs = (u32)((8 * mcus + JE_WG - 1) / JE_WG);
        d.fdct_first_wg = (u32)total_fdct; d.fdct_n_wgs = wy + 2 * wc; d.wg_u = wy; d.wg_v = wy + wc;
        total_color += d.color_n_wgs; total_fdct += d.fdct_n_wgs;
        plane_at[(size_t)i] = plane_bytes; /* multiples of 64 bytes */
        plane_bytes += (size_t)(yblocks + (g.ncomp == 3 ? 2 * mcus : 0)) * 64;
    }
    if (total_color > 0xffffffffULL || total_fdct > 0xffffffffULL) return FFHIP_EINVAL; /* the tables' entries are 32-bit workgroup indices */
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    if (n == 0) return FFHIP_OK;
    const size_t desc_bytes = (size_t)n * sizeof(JencDesc);
    const size_t table_words = (size_t)total_color + (size_t)total_fdct;
    const size_t planes_off = ffhip_up(desc_bytes + table_words * 4, 256);
    uint8_t *dev = nullptr;
    const int rc = ffhip_items_stage(SCRATCH_JPEG_ENC, stream, desc.data(), desc_bytes, table_words, planes_off + plane_bytes - desc_bytes - table_words * 4, &dev,
                                     [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            JencDesc &d = desc[(size_t)i];
            const size_t mcus = (size_t)d.mcu_cols * d.mcu_rows, hv = (size_t)(je_layout_h(d.layout) * je_layout_v(d.layout));
            d.plane_y = base + planes_off + plane_at[(size_t)i];
            d.plane_u = d.layout != FFHIP_JPEG_ENC_GREY ? d.plane_y + mcus * hv * 64 : nullptr;
            d.plane_v = d.layout != FFHIP_JPEG_ENC_GREY ? d.plane_u + mcus * 64 : nullptr;
        }
    });
    if (rc) return rc;
    const JencDesc *d_desc = (const JencDesc *)dev;
    u32 *d_color = (u32 *)(dev + desc_bytes), *d_fdct = d_color + total_color;
    hipLaunchKernelGGL((k_items_tables2<JencDesc, JencDesc, &JencDesc::color_first_wg, &JencDesc::color_n_wgs, &JencDesc::fdct_first_wg, &JencDesc::fdct_n_wgs>),
                       dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, d_desc, d_desc, d_color, d_fdct);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    JencArgs a;
    a.desc = d_desc; a.wg_item = d_color; a.wg_base = 0;
    const int lrc = ffhip_items_run(k_jpeg_color_downsample, total_color, JE_WG, stream, a);
    if (lrc) return lrc;
    a.wg_item = d_fdct;
    return ffhip_items_run(k_jpeg_fdct_islow, total_fdct, JE_WG, stream, a);
}

/* ------------------------------------------------------------------------------------------------ coefficients to files */
struct JhuffDesc {
    const int16_t *coef_y, *coef_u, *coef_v;
    uint8_t *out;
    unsigned long long cap, blocks, mcus;
    unsigned long long *pos; /* per block of the scan: its bits, then (k_jenc_positions) where they start */
    int32_t hv, bpm, ncomp, restart;
    u32 first_wg, n_wgs;     /* of the kernels that take a thread per block */
    u32 header_len, pad;
    uint8_t header[FFHIP_JPEG_ENC_HEADER_MAX];
};
struct JhuffStream { /* known once the positions are: the second upload */
    u32 *words, *mask;   /* the unstuffed stream (chunks x JE_CHUNK bytes) and one bit per byte of it */
    u32 *chunk_ff;       /* per chunk: its FF bytes to stuff, then (k_jenc_ff_scan) those in front of it */
    unsigned long long bytes; /* of the unstuffed stream, EOI included */
    u32 first_wg, n_wgs; /* chunks */
};
struct JhuffResult {
    unsigned long long stream_bytes, file_len;
    int32_t bad, status;
};

struct JhuffArgs {
    const JhuffDesc *desc;
    const JhuffStream *str;
    const u32 *tab;      /* [2][JE_TAB_WORDS] */
    const u32 *wg_item;
    JhuffResult *res;
    u32 wg_base;
};

/* count (EMIT = false) and write (EMIT = true): block g of the item's scan */
template <bool EMIT> __global__ __launch_bounds__(JE_WG) void k_jenc_blocks(JhuffArgs a)
{
    __shared__ u32 tab[2 * JE_TAB_WORDS];
    for (u32 k = threadIdx.x; k < 2 * JE_TAB_WORDS; k += JE_WG) tab[k] = a.tab[k];
    __syncthreads();
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JhuffDesc &d = a.desc[item];
    const unsigned long long g = (unsigned long long)(wg - d.first_wg) * JE_WG + threadIdx.x;
    if (g >= d.blocks) return;
    const long long mcu = (long long)(g / (unsigned)d.bpm);
    const int j = (int)(g - (unsigned long long)mcu * (unsigned)d.bpm);
    const int16_t *blk = je_scan_block(d.coef_y, d.coef_u, d.coef_v, d.hv, mcu, j);
    const int pred = je_scan_pred(d.coef_y, d.coef_u, d.coef_v, d.hv, mcu, j, d.restart);
    const u32 *t = tab + (j >= d.hv && d.ncomp == 3 ? JE_TAB_WORDS : 0);
    int bad = 0;
    if (!EMIT) {
        d.pos[g] = (unsigned long long)je_block_code(blk, pred, t, nullptr, &bad);
        if (bad) atomicOr(&a.res[item].bad, 1);
    } else {
        const JhuffStream &s = a.str[item];
        const unsigned long long start = d.pos[g];
        je_sink sink;
        je_sink_open(&sink, s.words, start);
        const int bits = je_block_code(blk, pred, t, &sink, &bad);
        const bool last_mcu = (unsigned long long)mcu == d.mcus - 1;
        if (j == d.bpm - 1 && (last_mcu || (d.restart && (mcu + 1) % d.restart == 0)))
            je_interval_end(&sink, start + (unsigned long long)bits, last_mcu ? 0xD9 : 0xD0 + (int)(((mcu + 1) / d.restart - 1) & 7), s.mask);
        je_sink_close(&sink);
    }
}

__device__ __forceinline__ je_span span_shfl_up(je_span v, int off)
{
    je_span o;
    o.a = __shfl_up((unsigned long long)v.a, off);
    o.c = __shfl_up((unsigned long long)v.c, off);
    o.starts = __shfl_up(v.starts, off);
    return o;
}

/* a workgroup per picture: pos[g] from the block's bits to where they start; the stream's size */
__global__ __launch_bounds__(JE_WG) void k_jenc_positions(const JhuffDesc *desc, JhuffResult *res)
{
    __shared__ je_span wave_sum[JE_WG / 64];
    const JhuffDesc &d = desc[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0; /* the position behind the blocks of the turns so far */
    const unsigned long long turns = (d.blocks + JE_WG - 1) / JE_WG;
    for (unsigned long long turn = 0; turn < turns; turn++) {
        const unsigned long long g = turn * JE_WG + threadIdx.x;
        je_span own = je_span_block(0, 0);
        int starts = 0;
        if (g < d.blocks) {
            const unsigned long long mcu = g / (unsigned)d.bpm;
            starts = g == mcu * (unsigned)d.bpm && mcu > 0 && d.restart && mcu % (unsigned)d.restart == 0;
            own = je_span_block((int)d.pos[g], starts);
        }
        je_span incl = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const je_span o = span_shfl_up(incl, off);
            if (lane >= off) incl = je_span_join(o, incl);
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        je_span before = je_span_block(0, 0); /* of the waves in front of this one */
        for (int w = 0; w < JE_WG / 64; w++)
            if (w < wave) before = je_span_join(before, wave_sum[w]);
        je_span all = wave_sum[0];
        for (int w = 1; w < JE_WG / 64; w++) all = je_span_join(all, wave_sum[w]);
        const unsigned long long end = je_span_apply(je_span_join(before, incl), carry); /* behind this block */
        if (g < d.blocks) d.pos[g] = end - (unsigned long long)(starts ? own.c - 16 : own.a);
        carry = je_span_apply(all, carry);
        __syncthreads();
    }
    if (threadIdx.x == 0) res[blockIdx.x].stream_bytes = (je_up8(carry) >> 3) + 2;
}

/* byte k of a stream word is an FF of entropy data */
__device__ __forceinline__ int stuffed(u32 w, u32 m, int k) { return ((w >> (8 * k)) & 255u) == 255u && !((m >> k) & 1u); }

/* the FF bytes of the thread's word (4 bytes from `at`) that get a 00, as a mask of 4 bits; nothing beyond the stream counts */
__device__ __forceinline__ u32 word_ff(const JhuffStream &s, unsigned long long at, u32 &w)
{
    w = s.words[at >> 2];
    const u32 m = (s.mask[at >> 5] >> (at & 31)) & 15u;
    u32 ff = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (at + k < s.bytes && stuffed(w, m, k)) ff |= 1u << k;
    return ff;
}

__global__ __launch_bounds__(JE_WG) void k_jenc_ff_count(JhuffArgs a)
{
    __shared__ u32 wave_sum[JE_WG / 64];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JhuffStream &s = a.str[item];
    const u32 chunk = wg - s.first_wg;
    u32 w, total;
    const u32 ff = word_ff(s, (unsigned long long)chunk * JE_CHUNK + 4u * threadIdx.x, w);
    wg_scan<JE_WG>((u32)__builtin_popcount(ff), wave_sum, &total);
    if (threadIdx.x == 0) s.chunk_ff[chunk] = total;
}

/* a workgroup per picture: chunk_ff to exclusive prefix sums; the file's size and the verdict */
__global__ __launch_bounds__(JE_WG) void k_jenc_ff_scan(const JhuffDesc *desc, const JhuffStream *str, JhuffResult *res)
{
    __shared__ u32 wave_sum[JE_WG / 64];
    const JhuffDesc &d = desc[blockIdx.x];
    const JhuffStream &s = str[blockIdx.x];
    unsigned long long carry = 0;
    const u32 turns = (s.n_wgs + JE_WG - 1) / JE_WG;
    for (u32 turn = 0; turn < turns; turn++) {
        const u32 c = turn * JE_WG + threadIdx.x;
        const u32 v = c < s.n_wgs ? s.chunk_ff[c] : 0u;
        u32 total;
        const u32 before = wg_scan<JE_WG>(v, wave_sum, &total);
        if (c < s.n_wgs) s.chunk_ff[c] = (u32)carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        JhuffResult &r = res[blockIdx.x];
        r.file_len = d.header_len + s.bytes + carry;
        r.status = r.bad ? FFHIP_EJPEG_RANGE : (r.file_len > d.cap ? FFHIP_EJPEG_NOSPACE : FFHIP_OK);
    }
}

__global__ __launch_bounds__(JE_WG) void k_jenc_copy(JhuffArgs a)
{
    __shared__ u32 wave_sum[JE_WG / 64];
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const JhuffDesc &d = a.desc[item];
    const JhuffStream &s = a.str[item];
    const u32 chunk = wg - s.first_wg;
    G(uint8_t) *out = (G(uint8_t) *)d.out;
    if (chunk == 0)
        for (u32 k = threadIdx.x; k < FFHIP_JPEG_ENC_HEADER_MAX; k += JE_WG)
            if (k < d.header_len && k < d.cap) out[k] = d.header[k];
    const unsigned long long at = (unsigned long long)chunk * JE_CHUNK + 4u * threadIdx.x;
    u32 w, total;
    const u32 ff = word_ff(s, at, w);
    const u32 before = wg_scan<JE_WG>((u32)__builtin_popcount(ff), wave_sum, &total);
    unsigned long long o = d.header_len + at + s.chunk_ff[chunk] + before;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (at + k >= s.bytes) break;
        if (o < d.cap) out[o] = (uint8_t)(w >> (8 * k));
        o++;
        if ((ff >> k) & 1u) {
            if (o < d.cap) out[o] = 0;
            o++;
        }
    }
}

bool huff_item_ok(const ffhip_jpeg_huff_item &it)
{
    if (!ffhip_jenc_params_ok(it.width, it.height, it.layout, it.restart)) return false;
    if (!it.d_coef_y || ((uintptr_t)it.d_coef_y & 15) || (it.cap && !it.d_out)) return false;
    if (it.layout == FFHIP_JPEG_ENC_GREY) { if (it.d_coef_u || it.d_coef_v) return false; }
    else if (!it.d_coef_u || !it.d_coef_v || ((uintptr_t)it.d_coef_u & 15) || ((uintptr_t)it.d_coef_v & 15)) return false;
    /* the stated limit of the two calls: chunk indices, FF counts and the offsets within a file's chunks are held in 32 bits */
    return ffhip_jpeg_encode_bound(it.width, it.height, it.layout, it.restart) < ((size_t)1 << 32);
}

int huff_items_impl(const ffhip_jpeg_huff_item *items, int n, size_t *len_out, int *status, void *stream, bool checked)
{
    if (n < 0 || (n > 0 && (!items || !len_out || !status))) return FFHIP_EINVAL;
    std::vector<JhuffDesc> desc((size_t)n);
    unsigned long long total_wgs = 0, total_blocks = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_huff_item &it = items[i];
        if (!checked && !huff_item_ok(it)) return FFHIP_EINVAL;
        ffhip_jenc_geometry g;
        ffhip_jenc_geom(it.width, it.height, it.layout, &g);
        JhuffDesc &d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.coef_y = it.d_coef_y; d.coef_u = it.d_coef_u; d.coef_v = it.d_coef_v;
        d.out = it.d_out; d.cap = it.cap; d.blocks = (unsigned long long)g.blocks; d.mcus = (unsigned long long)g.mcus;
        d.hv = g.h * g.v; d.bpm = g.bpm; d.ncomp = g.ncomp; d.restart = it.restart;
        d.first_wg = (u32)total_wgs; d.n_wgs = (u32)((d.blocks + JE_WG - 1) / JE_WG);
        d.header_len = (u32)ffhip_jenc_header(it.width, it.height, it.layout, it.quality, it.restart, d.header);
        total_wgs += d.n_wgs; total_blocks += d.blocks;
    }
    if (total_wgs > 0xffffffffULL) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    if (n == 0) return FFHIP_OK;
    hipStream_t st = (hipStream_t)stream;

    /* first scratch: the records and the code tables (uploaded), the per-workgroup table, the positions, the results */
    const size_t desc_bytes = (size_t)n * sizeof(JhuffDesc), tab_bytes = 2 * JE_TAB_WORDS * sizeof(u32);
    std::vector<uint8_t> rec(desc_bytes + tab_bytes);
    ffhip_jenc_code_tables((uint32_t *)(rec.data() + desc_bytes));
    const size_t pos_off = ffhip_up(rec.size() + (size_t)total_wgs * 4, 256);
    const size_t res_off = pos_off + (size_t)total_blocks * 8, res_bytes = (size_t)n * sizeof(JhuffResult);
    uint8_t *dev = nullptr;
    int rc = ffhip_items_stage(SCRATCH_JPEG_ENC + 1, stream, rec.data(), rec.size(), (size_t)total_wgs, res_off + res_bytes - rec.size() - (size_t)total_wgs * 4, &dev,
                               [&](uint8_t *base) {
        unsigned long long at = 0;
        for (int i = 0; i < n; i++) {
            desc[(size_t)i].pos = (unsigned long long *)(base + pos_off) + at;
            at += desc[(size_t)i].blocks;
        }
        memcpy(rec.data(), desc.data(), desc_bytes);
    });
    if (rc) return rc;
    JhuffArgs a;
    a.desc = (const JhuffDesc *)dev; a.str = nullptr; a.tab = (const u32 *)(dev + desc_bytes); a.res = (JhuffResult *)(dev + res_off);
    u32 *d_block_item = (u32 *)(dev + rec.size());
    a.wg_item = d_block_item; a.wg_base = 0;
    FFHIP_CHECK(hipMemsetAsync(a.res, 0, res_bytes, st), FFHIP_EIO);
    hipLaunchKernelGGL(k_items_table<JhuffDesc>, dim3((unsigned)n), dim3(256), 0, st, a.desc, d_block_item);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_jenc_blocks<false>, total_wgs, JE_WG, stream, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_jenc_positions, dim3((unsigned)n), dim3(JE_WG), 0, st, a.desc, a.res);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    /* the streams' sizes: the first of the call's two synchronisations */
    const JhuffResult *h_res = nullptr;
    rc = ffhip_records_fetch(SCRATCH_JPEG_ENC + 3, stream, a.res, n, &h_res);
    if (rc) return rc;

    /* second scratch, sized by the counted totals: the stream records (uploaded), the per-chunk table, chunk_ff, then words and masks (zeroed) */
    std::vector<JhuffStream> str((size_t)n);
    std::vector<size_t> words_at((size_t)n), mask_at((size_t)n);
    unsigned long long total_chunks = 0;
    size_t zero_bytes = 0;
    for (int i = 0; i < n; i++) {
        JhuffStream &s = str[(size_t)i];
        s.bytes = h_res[i].stream_bytes;
        s.first_wg = (u32)total_chunks; s.n_wgs = (u32)((s.bytes + JE_CHUNK - 1) / JE_CHUNK);
        total_chunks += s.n_wgs;
        words_at[(size_t)i] = zero_bytes;
        zero_bytes += (size_t)s.n_wgs * JE_CHUNK + 64; /* a block's closing word may lie in the four bytes behind the stream */
        mask_at[(size_t)i] = zero_bytes;
        zero_bytes += ffhip_up((size_t)s.n_wgs * JE_CHUNK / 8 + 1, 64);
    }
    if (total_chunks > 0xffffffffULL) return FFHIP_EINVAL;
    const size_t str_bytes = (size_t)n * sizeof(JhuffStream);
    const size_t ff_off = str_bytes + (size_t)total_chunks * 4, zero_off = ffhip_up(ff_off + (size_t)total_chunks * 4, 256);
    uint8_t *dev2 = nullptr;
    rc = ffhip_items_stage(SCRATCH_JPEG_ENC + 2, stream, str.data(), str_bytes, (size_t)total_chunks, zero_off + zero_bytes - str_bytes - (size_t)total_chunks * 4, &dev2,
                           [&](uint8_t *base) {
        for (int i = 0; i < n; i++) {
            JhuffStream &s = str[(size_t)i];
            s.words = (u32 *)(base + zero_off + words_at[(size_t)i]);
            s.mask = (u32 *)(base + zero_off + mask_at[(size_t)i]);
            s.chunk_ff = (u32 *)(base + ff_off) + s.first_wg;
        }
    });
    if (rc) return rc;
    a.str = (const JhuffStream *)dev2;
    u32 *d_chunk_item = (u32 *)(dev2 + str_bytes);
    FFHIP_CHECK(hipMemsetAsync(dev2 + zero_off, 0, zero_bytes, st), FFHIP_EIO);
    hipLaunchKernelGGL(k_items_table<JhuffStream>, dim3((unsigned)n), dim3(256), 0, st, a.str, d_chunk_item);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_jenc_blocks<true>, total_wgs, JE_WG, stream, a);
    if (rc) return rc;
    a.wg_item = d_chunk_item;
    rc = ffhip_items_run(k_jenc_ff_count, total_chunks, JE_WG, stream, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_jenc_ff_scan, dim3((unsigned)n), dim3(JE_WG), 0, st, a.desc, a.str, a.res);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    rc = ffhip_items_run(k_jenc_copy, total_chunks, JE_WG, stream, a);
    if (rc) return rc;
    /* lengths and verdicts: the second synchronisation */
    return ffhip_lengths_read(SCRATCH_JPEG_ENC + 3, stream, (const JhuffResult *)a.res, n, len_out, status);
}

} // namespace

extern "C" int ffhip_jpeg_fdct_items(const ffhip_jpeg_fdct_item *items, int n, void *stream) { return fdct_items_impl(items, n, stream, false); }

extern "C" int ffhip_jpeg_huff_encode_items(const ffhip_jpeg_huff_item *items, int n, size_t *len_out, int *status, void *stream)
{
    return huff_items_impl(items, n, len_out, status, stream, false);
}

extern "C" int ffhip_jpeg_encode_items(const ffhip_jpeg_encode_item *items, int n, size_t *len_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!items || !len_out || !status))) return FFHIP_EINVAL;
    std::vector<ffhip_jpeg_fdct_item> fd((size_t)n);
    std::vector<ffhip_jpeg_huff_item> hf((size_t)n);
    std::vector<size_t> coef_bytes((size_t)n);
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_encode_item &it = items[i];
        if (it.reserved != 0 || !ffhip_jenc_source_ok(&it.src, it.layout)) return FFHIP_EINVAL;
        ffhip_jenc_geometry g;
        ffhip_jenc_geom(it.src.width, it.src.height, it.layout, &g);
        coef_bytes[(size_t)i] = (size_t)g.blocks * 128;
        ffhip_jpeg_fdct_item &f = fd[(size_t)i];
        f.src = it.src; f.layout = it.layout; f.quality = it.quality;
        f.d_coef_y = (int16_t *)16; f.d_coef_u = f.d_coef_v = it.layout == FFHIP_JPEG_ENC_GREY ? nullptr : (int16_t *)16; /* placeholders for the check */
        ffhip_jpeg_huff_item &h = hf[(size_t)i];
        h.width = it.src.width; h.height = it.src.height; h.layout = it.layout; h.quality = it.quality; h.restart = it.restart;
        h.d_coef_y = f.d_coef_y; h.d_coef_u = f.d_coef_u; h.d_coef_v = f.d_coef_v; h.d_out = it.d_out; h.cap = it.cap;
        if (!huff_item_ok(h)) return FFHIP_EINVAL;
    }
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(nullptr);
    /* a part: pictures while their coefficient planes fit the budget */
    return ffhip_parts_run(n, budget, FFHIP_PARTS_NO_CAP, [&](int i) { return coef_bytes[(size_t)i]; }, [&](int first, int cnt) -> int {
        size_t bytes = 0;
        for (int i = first; i < first + cnt; i++) bytes += coef_bytes[(size_t)i];
        int16_t *planes = (int16_t *)ffhip_scratch(SCRATCH_JPEG_ENC + 4, stream, bytes / 4 + 16);
        if (!planes) return FFHIP_ENOMEM;
        size_t at = 0;
        for (int i = first; i < first + cnt; i++) {
            ffhip_jenc_geometry g;
            ffhip_jenc_geom(fd[(size_t)i].src.width, fd[(size_t)i].src.height, fd[(size_t)i].layout, &g);
            int16_t *y = planes + at, *u = g.ncomp == 3 ? y + g.mcus * g.h * g.v * 64 : nullptr, *v = g.ncomp == 3 ? u + g.mcus * 64 : nullptr;
            fd[(size_t)i].d_coef_y = y; fd[(size_t)i].d_coef_u = u; fd[(size_t)i].d_coef_v = v;
            hf[(size_t)i].d_coef_y = y; hf[(size_t)i].d_coef_u = u; hf[(size_t)i].d_coef_v = v;
            at += coef_bytes[(size_t)i] / 2;
        }
        const int rc = fdct_items_impl(fd.data() + first, cnt, stream, true);
        if (rc) return rc; /* the call's own codes only: every one of them ends the call */
        return huff_items_impl(hf.data() + first, cnt, len_out + first, status + first, stream, true);
    });
}
