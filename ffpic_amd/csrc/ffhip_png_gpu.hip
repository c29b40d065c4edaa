/* ffhip_png_gpu.hip -- PNG files to BGRA pictures on the device (include/ffpic_hip.h, "PNG").  Host threads walk the chunks,
 * check the CRCs and inflate (ffhip_png.c, ffhip_inflate.c) straight into a part's pinned staging; one upload; k_png_unfilter undoes the
 * row filters in place, k_png_expand writes the pictures.  Both kernels compile the functions of ffhip_png_body.h, as ffhip_png_picture
 * does on the host, and neither has an error path: what a file can be refused for is seen on the host.  How a part is driven -- the
 * launch per band level, the gather launch, the end of a part, the stage clock -- is ffhip_staged.h's; the cut into parts is here.
 * With FFHIP_PNG_INFLATE_DEVICE the host threads copy the streams instead and k_inflate (ffhip_inflate_gpu.hip)
 * inflates them in front of the two kernels: png_front_device beside png_front_host.
 *
 * k_png_unfilter.  An item is one (file, pass) sub-image, cut into bands of 64 rows; a wave takes one band, lane r its row r.  A row is
 * walked in CHUNKS of four filter units (4 x bpp bytes = bpp dwords), and the lanes are skewed by one chunk: at step t lane r
 * reconstructs chunk t - r of its row.  Then `a` and `c` of a chunk's first unit are the lane's own registers from the step before, and
 * `b` -- the chunk above -- is what lane r - 1 produced one step earlier: bpp cross-lane moves (DPP wave_shr:1) per step, no LDS and no
 * memory round trip.  Lane 0 reads `b` from the last row of the band above, in global memory, which the launch before has written: bands
 * of an item depend on each other top to bottom, and level l of every item is one launch.  No spin-waits, no counters.
 *   The loads: a lane reads its own row, so a wave's loads are 64 short runs at the row pitch, at arbitrary byte addresses.  The choice
 * is wide unaligned loads consumed over several steps -- a chunk is one unaligned load of bpp dwords, consumed over four units -- rather
 * than a staged tile: a tile would put the rows' bytes through LDS only to hand every lane its own row back, and the cross-lane traffic
 * this kernel has (b) goes through DPP.  What the chunk buys is one load and one store per four units instead of per unit; what it
 * costs is a skew of 63 chunks, not units, per band (13 % of a 1920-unit row's steps).
 *
 * k_png_expand.  The gather form: a lane owns four consecutive output pixels of a row and makes one 16-byte store.  Of an Adam7 file the
 * lane finds each pixel's pass and index by the map, so stores stay full rows whatever the interlace.  A picture's last partial group of
 * four is stored pixel by pixel. */
#include "ffhip_staged.h"
#include "ffhip_inflate_gpu.h"
#include "ffhip_png_internal.h"

#include <chrono>

namespace {

constexpr int PNG_BAND = 64;
constexpr int PNG_EXPAND_THREADS = FFHIP_GATHER_THREADS;

/* one (file, pass) sub-image: `rows` rows of 1 + row_bytes bytes at `sub` */
struct PngUnfDesc {
    uint8_t *sub;
    u32 rows, row_bytes, bpp, n_bands;
};
struct PngUnfArgs {
    const PngUnfDesc *desc; /* sorted by n_bands, largest first: the items with a band `level` are the first of them */
    u32 level, wg_base;
};

/* one file's picture */
struct PngExpDesc {
    const uint8_t *rows;  /* the file's unfiltered sub-images, one behind the other */
    uint8_t *dst;
    int64_t pitch;
    const u32 *palette;   /* 256 BGRA dwords, colour type 3 only */
    unsigned long long pass_off[7]; /* by Adam7 pass ([0] alone: not interlaced) */
    u32 pass_pitch[7];    /* 1 + row bytes */
    u32 width, height, groups_x;
    u32 first_wg, n_wgs;
    ffhip_png_expand_rule rule;
};
struct PngExpArgs {
    const PngExpDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
};

template <int N> struct __attribute__((packed)) PngRun { u32 w[N]; }; /* N dwords at any byte address */

/* nb <= 4 * N bytes at p -> w, zero behind them; nb == 4 * N is one unaligned load */
template <int N> __device__ __forceinline__ void png_load_run(const uint8_t *p, u32 nb, u32 (&w)[N])
{
    if (nb == 4 * N) {
        const PngRun<N> v = *(const PngRun<N> *)p;
#pragma unroll
        for (int k = 0; k < N; k++) w[k] = v.w[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = 0;
#pragma unroll
    for (int i = 0; i < 4 * N; i++)
        if ((u32)i < nb) w[i >> 2] |= (u32)p[i] << (8 * (i & 3));
}

template <int N> __device__ __forceinline__ void png_store_run(uint8_t *p, u32 nb, const u32 (&w)[N])
{
    if (nb == 4 * N) {
        PngRun<N> v;
#pragma unroll
        for (int k = 0; k < N; k++) v.w[k] = w[k];
        *(PngRun<N> *)p = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4 * N; i++)
        if ((u32)i < nb) p[i] = (uint8_t)byte_of(w, i);
}

/* One band.  Every lane runs every step, whatever its row: the cross-lane move wants the whole wave */
template <int BPP> __device__ __forceinline__ void png_unfilter_band(const PngUnfDesc &d, u32 band, int lane)
{
    constexpr int CB = 4 * BPP; /* a chunk: four units, BPP dwords */
    const unsigned long long pitch = (unsigned long long)d.row_bytes + 1;
    const u32 row = band * PNG_BAND + (u32)lane;
    const bool live = row < d.rows;
    uint8_t *cur = d.sub + (live ? row : 0) * pitch + 1;
    const int ft = live ? cur[-1] : 0;
    const u32 n_chunks = (d.row_bytes + CB - 1) / CB;
    const uint8_t *above = band ? d.sub + ((unsigned long long)band * PNG_BAND - 1) * pitch + 1 : nullptr; /* lane 0's b */
    u32 out[BPP], corner[BPP]; /* the lane's last chunk; of it and of the chunk above it, the last unit (bytes 3 BPP ..) */
#pragma unroll
    for (int k = 0; k < BPP; k++) out[k] = corner[k] = 0;
    for (u32 t = 0; t < n_chunks + PNG_BAND - 1; t++) {
        u32 up[BPP];
#pragma unroll
        for (int k = 0; k < BPP; k++) up[k] = wave_shr1(out[k]); /* lane r - 1's; lane 0: 0 */
        const u32 q = t - (u32)lane;
        if (!live || t < (u32)lane || q >= n_chunks) continue;
        const u32 nb = min((u32)CB, d.row_bytes - q * CB);
        if (lane == 0 && above) png_load_run(above + (unsigned long long)q * CB, nb, up);
        u32 raw[BPP];
        png_load_run(cur + (unsigned long long)q * CB, nb, raw);
        int o[CB];
#pragma unroll
        for (int i = 0; i < CB; i++) {
            const int a = i >= BPP ? o[i - BPP] : byte_of(out, 3 * BPP + i);
            const int c = i >= BPP ? byte_of(up, i - BPP) : byte_of(corner, 3 * BPP + i);
            o[i] = ffhip_png_unfilter_byte(ft, byte_of(raw, i), a, byte_of(up, i), c);
        }
#pragma unroll
        for (int k = 0; k < BPP; k++) {
            out[k] = (u32)o[4 * k] | (u32)o[4 * k + 1] << 8 | (u32)o[4 * k + 2] << 16 | (u32)o[4 * k + 3] << 24;
            corner[k] = up[k];
        }
        png_store_run(cur + (unsigned long long)q * CB, nb, out);
    }
}

__global__ __launch_bounds__(PNG_BAND) void k_png_unfilter(PngUnfArgs a)
{
    const PngUnfDesc d = a.desc[a.wg_base + blockIdx.x];
    const int lane = (int)threadIdx.x;
    switch (d.bpp) {
    case 1: png_unfilter_band<1>(d, a.level, lane); break;
    case 2: png_unfilter_band<2>(d, a.level, lane); break;
    case 3: png_unfilter_band<3>(d, a.level, lane); break;
    case 4: png_unfilter_band<4>(d, a.level, lane); break;
    case 6: png_unfilter_band<6>(d, a.level, lane); break;
    default: png_unfilter_band<8>(d, a.level, lane); break;
    }
}

__global__ __launch_bounds__(PNG_EXPAND_THREADS) void k_png_expand(PngExpArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const PngExpDesc *d = a.desc + item;
    const u32 width = d->width, gx = d->groups_x;
    const u32 g = (wg - d->first_wg) * PNG_EXPAND_THREADS + threadIdx.x; /* groups_x x height < 2^30 */
    if (g >= gx * d->height) return;
    const u32 y = g / gx, x0 = 4 * (g - y * gx);
    const u32 n = min(4u, width - x0);
    const ffhip_png_expand_rule rule = d->rule;
    const u32 *pal = d->palette;
    u32 v[4] = {0, 0, 0, 0};
    if (!rule.interlace && rule.depth == 8 && n == 4 && (rule.ctype == 6 || (rule.ctype == 2 && !rule.has_trns))) {
        /* the two common kinds, a whole group: one run of 16 or 12 bytes */
        const uint8_t *row = d->rows + (unsigned long long)y * d->pass_pitch[0] + 1;
        if (rule.ctype == 6) {
            u32 w[4];
            png_load_run(row + 4ull * x0, 16, w);
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (w[j] & 0xff00ff00u) | ((w[j] & 0xffu) << 16) | ((w[j] >> 16) & 0xffu);
        } else {
            u32 w[3];
            png_load_run(row + 3ull * x0, 12, w);
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = ffhip_png_bgra((u32)byte_of(w, 3 * j + 2), (u32)byte_of(w, 3 * j + 1), (u32)byte_of(w, 3 * j), 255u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if ((u32)j >= n) break;
            u32 px = x0 + (u32)j, py = y;
            const int p = rule.interlace ? ffhip_png_adam7_of(x0 + (u32)j, y, &px, &py) : 0;
            v[j] = ffhip_png_pixel(&rule, d->rows + d->pass_off[p] + (unsigned long long)py * d->pass_pitch[p] + 1, px, pal);
        }
    }
    uint8_t *out = d->dst + (long long)y * d->pitch + 4ll * x0;
    if (n == 4) {
        *(u32x4 *)out = u32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (u32 j = 0; j < n; j++) ((u32 *)out)[j] = v[j];
    }
}

thread_local int t_png_last[2];       /* ffhip_debug_png_last */
thread_local double t_png_times[4];   /* ffhip_debug_png_times */
thread_local double t_png_inflate[4]; /* ffhip_debug_png_inflate */

struct PngPartFile { int idx; size_t rows_off, palette_off; };
/* where the stages behind the front end find a part's file on the device */
struct PngPartPlace { uint8_t *rows; const u32 *palette; };

/* three events of the device front end's own, made only under FFHIP_PNG_TIMES */
struct PngInflateClock {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on;
    explicit PngInflateClock(bool want) : on(want)
    {
        for (int k = 0; on && k < 3; k++)
            if (hipEventCreate(&ev[k]) != hipSuccess) on = false;
    }
    PngInflateClock(const PngInflateClock &) = delete;
    ~PngInflateClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t st) { if (on) (void)hipEventRecord(ev[k], st); }
    double ms(int k) /* from mark k to mark k + 1, behind a synchronisation */
    {
        float v = 0;
        return on && hipEventElapsedTime(&v, ev[k], ev[k + 1]) == hipSuccess ? v : 0.0;
    }
};

/* A part's front end, the host way: the host threads inflate into the pinned staging (the filtered pictures, then the palettes), one
 * upload */
int png_front_host(const std::vector<PngPartFile> &part, size_t bytes, const std::vector<ffhip_png_file> &pf, const uint8_t *const *files, const size_t *lens,
                   int n_threads, int *status, void *stream, StageClock &clock, std::vector<PngPartPlace> &place)
{
    hipStream_t st = (hipStream_t)stream;
    clock.mark_from(0, st);
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_PNG, stream, bytes + 64);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_PNG, stream, bytes / 4 + 16);
    if (!pin || !dev) return FFHIP_ENOMEM;
    const auto t0 = std::chrono::steady_clock::now();
    ffhip_parallel_for((int)part.size(), n_threads, [&](int k) {
        const PngPartFile &p = part[(size_t)k];
        const ffhip_png_file &f = pf[(size_t)p.idx];
        status[p.idx] = ffhip_png_read_filtered(files[p.idx], lens[p.idx], &f, pin + p.rows_off);
        if (f.info.color_type == 3) memcpy(pin + p.palette_off, f.palette, 1024);
    });
    t_png_times[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t_png_inflate[1] += (double)part.size();
    clock.mark_from(0, st);
    FFHIP_CHECK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
    clock.mark_from(1, st);
    for (size_t k = 0; k < part.size(); k++) place[k] = {dev + part[k].rows_off, (const u32 *)(dev + part[k].palette_off)};
    return FFHIP_OK;
}

/* The same with FFHIP_PNG_INFLATE_DEVICE.  The device scratch holds the filtered pictures at their places of the host way (`rows_bytes`
 * of them) and behind them the TAIL, which alone has a pinned copy and is the one upload: the palettes, the filtered bytes of the files
 * the host threads inflate after all (a palette shorter than its depth's range: ffhip_png_read_filtered checks the indices on unfiltered
 * rows), every other file's IDAT payloads joined, and k_inflate's records.  k_inflate writes the pictures and its verdicts, one copy
 * brings the records back, one synchronisation.  The upload's time goes where the host way's goes; the launch and the copy back are
 * ffhip_debug_png_inflate's alone: the part's clock starts again behind them */
int png_front_device(const std::vector<PngPartFile> &part, size_t rows_bytes, const std::vector<ffhip_png_file> &pf, const uint8_t *const *files,
                     const size_t *lens, int n_threads, int *status, void *stream, StageClock &clock, std::vector<PngPartPlace> &place)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t n = part.size();
    std::vector<size_t> pal_off(n, 0), own_off(n, 0);
    std::vector<char> host_way(n, 0);
    size_t tail = 0, n_dev = 0, z_bytes = 0;
    for (size_t k = 0; k < n; k++)
        if (pf[(size_t)part[k].idx].info.color_type == 3) { pal_off[k] = tail; tail += 1024; }
    for (size_t k = 0; k < n; k++) {
        const ffhip_png_file &f = pf[(size_t)part[k].idx];
        host_way[k] = (char)ffhip_png_short_palette(&f.info);
        own_off[k] = tail; /* filtered bytes, or the stream */
        tail += ffhip_up(host_way[k] ? (size_t)f.info.filtered_bytes : f.idat_bytes, 16);
        if (!host_way[k]) { n_dev++; z_bytes += f.idat_bytes; }
    }
    const size_t rec_off = tail, rec_bytes = n_dev * sizeof(FfhipInflateRec);
    tail += rec_bytes;
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_PNG, stream, tail + 64);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_PNG, stream, (rows_bytes + tail) / 4 + 16);
    if (!pin || !dev) return FFHIP_ENOMEM;
    uint8_t *dev_tail = dev + rows_bytes;
    const auto t0 = std::chrono::steady_clock::now();
    ffhip_parallel_for((int)n, n_threads, [&](int k) {
        const PngPartFile &p = part[(size_t)k];
        const ffhip_png_file &f = pf[(size_t)p.idx];
        if (host_way[(size_t)k]) status[p.idx] = ffhip_png_read_filtered(files[p.idx], lens[p.idx], &f, pin + own_off[(size_t)k]);
        else ffhip_png_join_idat(files[p.idx], &f, pin + own_off[(size_t)k]);
        if (f.info.color_type == 3) memcpy(pin + pal_off[(size_t)k], f.palette, 1024);
    });
    t_png_times[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<FfhipInflateRec> rec;
    rec.reserve(n_dev);
    for (size_t k = 0; k < n; k++) {
        const ffhip_png_info &info = pf[(size_t)part[k].idx].info;
        place[k] = {host_way[k] ? dev_tail + own_off[k] : dev + part[k].rows_off, (const u32 *)(dev_tail + pal_off[k])};
        if (host_way[k]) continue;
        FfhipInflateRec r;
        memset(&r, 0, sizeof(r));
        r.src = dev_tail + own_off[k];
        r.dst = place[k].rows;
        r.len = pf[(size_t)part[k].idx].idat_bytes;
        r.cap = info.filtered_bytes;
        r.partial = 1; /* PNG's "extra bytes are ignored" */
        r.index = (u32)k;
        r.png = 1;
        for (int q = 0; q < 7; q++) {
            r.rows[q] = (u32)info.pass_rows[q];
            r.pitch[q] = (u32)info.pass_row_bytes[q] + 1;
        }
        rec.push_back(r);
    }
    ffhip_inflate_sort(rec);
    if (rec_bytes) memcpy(pin + rec_off, rec.data(), rec_bytes);
    t_png_inflate[0] += (double)n_dev;
    t_png_inflate[1] += (double)(n - n_dev);
    t_png_inflate[2] += (double)z_bytes;
    PngInflateClock own(clock.on);
    own.mark(0, st);
    FFHIP_CHECK(hipMemcpyAsync(dev_tail, pin, tail, hipMemcpyHostToDevice, st), FFHIP_EIO);
    own.mark(1, st);
    if (n_dev) {
        const int rc = ffhip_inflate_launch((FfhipInflateRec *)(dev_tail + rec_off), n_dev, stream);
        if (rc) return rc;
        FFHIP_CHECK(hipMemcpyAsync(pin + rec_off, dev_tail + rec_off, rec_bytes, hipMemcpyDeviceToHost, st), FFHIP_EIO);
    }
    own.mark(2, st);
    FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO);
    t_png_times[1] += own.ms(0);
    t_png_inflate[3] += own.ms(1);
    const FfhipInflateRec *back = (const FfhipInflateRec *)(pin + rec_off);
    for (size_t k = 0; k < n_dev; k++) status[part[back[k].index].idx] = back[k].status;
    clock.mark_from(0, st);
    return FFHIP_OK;
}

/* One part: files pf[] of the call, `rows_bytes` of filtered pictures and `palette_bytes` of palettes behind them.  The clock
 * (FFHIP_PNG_TIMES) stands around the upload, the unfilter launches and the expand launch */
int png_run_part(const std::vector<PngPartFile> &part, size_t rows_bytes, size_t palette_bytes, const std::vector<ffhip_png_file> &pf,
                 const uint8_t *const *files, const size_t *lens, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch, int *status,
                 unsigned png_flags, void *stream, StageClock &clock)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<PngPartPlace> place(part.size());
    int rc = png_flags & FFHIP_PNG_INFLATE_DEVICE
                 ? png_front_device(part, rows_bytes, pf, files, lens, n_threads, status, stream, clock, place)
                 : png_front_host(part, rows_bytes + palette_bytes, pf, files, lens, n_threads, status, stream, clock, place);
    if (rc) return rc;
    std::vector<PngUnfDesc> unf;
    std::vector<PngExpDesc> exp;
    unsigned long long total = 0;
    for (size_t k = 0; k < part.size(); k++) {
        const PngPartFile &p = part[k];
        if (status[p.idx]) continue;
        const ffhip_png_file &f = pf[(size_t)p.idx];
        const ffhip_png_info &info = f.info;
        PngExpDesc e;
        memset(&e, 0, sizeof(e));
        e.rows = place[k].rows;
        e.dst = d_bgra[p.idx];
        e.pitch = pitch[p.idx];
        e.palette = info.color_type == 3 ? place[k].palette : nullptr;
        e.width = (u32)info.width;
        e.height = (u32)info.height;
        e.rule = f.rule;
        unsigned long long at = 0;
        for (int q = 0; q < 7; q++) {
            e.pass_off[q] = at;
            e.pass_pitch[q] = (u32)info.pass_row_bytes[q] + 1;
            if (!info.pass_rows[q]) continue;
            PngUnfDesc u;
            u.sub = place[k].rows + at;
            u.rows = (u32)info.pass_rows[q];
            u.row_bytes = (u32)info.pass_row_bytes[q];
            u.bpp = (u32)ffhip_png_bpp(info.color_type, info.bit_depth);
            u.n_bands = (u.rows + PNG_BAND - 1) / PNG_BAND;
            unf.push_back(u);
            at += (unsigned long long)e.pass_pitch[q] * u.rows;
        }
        ffhip_gather_place(e, &total); /* n_wgs < 2^22: both sides below 2^16 */
        exp.push_back(e);
    }
    if (exp.empty()) return FFHIP_OK;
    rc = ffhip_banded_launches(SCRATCH_PNG + 1, stream, unf, &t_png_last[1], [&](u32 level, const PngUnfDesc *d_unf, unsigned grid_x, u32 wg_base) {
        PngUnfArgs a;
        a.desc = d_unf; a.level = level; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_png_unfilter, dim3(grid_x), dim3(PNG_BAND), 0, st, a);
    });
    if (rc) return rc;
    clock.mark_from(2, st);
    rc = ffhip_gather_launch(SCRATCH_PNG + 2, stream, exp, total, [&](const PngExpDesc *d_exp, const u32 *d_table, unsigned grid_x, u32 wg_base) {
        PngExpArgs a;
        a.desc = d_exp; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_png_expand, dim3(grid_x), dim3(PNG_EXPAND_THREADS), 0, st, a);
    });
    clock.mark_from(3, st);
    return rc;
}

} // namespace

extern "C" int ffhip_png_decode_files_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                                const int64_t *pitch, ffhip_png_info *info_out, int *status, unsigned png_flags, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status)) || (png_flags & ~FFHIP_PNG_INFLATE_DEVICE)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    const char *sw = FFHIP_ENV("FFHIP_PNG_INFLATE_GPU"); /* the unedited tools and suites over the device front end */
    if (sw && sw[0] && sw[0] != '0') png_flags |= FFHIP_PNG_INFLATE_DEVICE;
    n_threads = ffhip_host_threads(n_threads);
    std::vector<ffhip_png_file> pf((size_t)n);
    ffhip_parallel_for(n, n_threads, [&](int i) {
        ffhip_png_file &f = pf[(size_t)i];
        status[i] = files[i] && lens[i] ? ffhip_png_open(files[i], lens[i], &f) : FFHIP_EINVAL;
        if (status[i]) memset(&f.info, 0, sizeof(f.info));
        if (info_out) info_out[i] = f.info;
        if (status[i]) return;
        if (!ffhip_bgra_takes_stores16(d_bgra[i], pitch[i], f.info.width)) status[i] = FFHIP_EINVAL; /* k_png_expand's */
    });
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    t_png_last[0] = t_png_last[1] = 0;
    for (double &t : t_png_times) t = 0;
    for (double &t : t_png_inflate) t = 0;
    StageClock clock(FFHIP_ENV("FFHIP_PNG_TIMES"), t_png_times);
    const size_t budget = ffhip_part_budget(FFHIP_ENV("FFHIP_PNG_PART_BYTES"));
    int rc = FFHIP_OK;
    for (int i = 0; i < n && rc == FFHIP_OK;) {
        std::vector<PngPartFile> part;
        size_t rows = 0, palettes = 0;
        for (; i < n; i++) {
            if (status[i]) continue;
            const size_t need = ffhip_up((size_t)pf[(size_t)i].info.filtered_bytes, 16);
            if (!part.empty() && rows + need > budget) break;
            part.push_back({i, rows, palettes});
            rows += need;
            if (pf[(size_t)i].info.color_type == 3) palettes += 1024;
        }
        if (part.empty()) break;
        for (PngPartFile &p : part) p.palette_off += rows;
        t_png_last[0]++;
        rc = ffhip_part_end(png_run_part(part, rows, palettes, pf, files, lens, n_threads, d_bgra, pitch, status, png_flags, stream, clock), stream, clock);
    }
    if (rc) return rc;
    for (int k = 0; k < n; k++)
        if (status[k]) return status[k];
    return FFHIP_OK;
}

extern "C" int ffhip_png_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                             const int64_t *pitch, ffhip_png_info *info_out, int *status, void *stream)
{
    return ffhip_png_decode_files_device_ex(files, lens, n, n_threads, d_bgra, pitch, info_out, status, 0u, stream);
}

extern "C" int ffhip_debug_png_inflate(double out[4]) { return ffhip_copy_out(out, t_png_inflate); }

extern "C" int ffhip_debug_png_last(int out[2]) { return ffhip_copy_out(out, t_png_last); }

extern "C" int ffhip_debug_png_times(double out[4]) { return ffhip_copy_out(out, t_png_times); }
