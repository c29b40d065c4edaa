/* ffhip_png_gpu.hip -- PNG files to BGRA pictures on the device (include/ffpic_hip.h, "PNG").  Host threads walk the chunks,
 * check the CRCs and inflate (ffhip_png.c, ffhip_inflate.c) straight into a part's pinned staging; one upload; k_png_unfilter undoes the
 * row filters in place, k_png_expand writes the pictures.  Both kernels compile the functions of ffhip_png_body.h, as ffhip_png_picture
 * does on the host, and neither has an error path: what a file can be refused for is seen on the host.
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
#include "ffhip_items.h"
#include "ffhip_png_internal.h"

#include <algorithm>
#include <chrono>
#include <stdlib.h>

namespace {

constexpr int PNG_BAND = 64;
constexpr int PNG_EXPAND_THREADS = 256;

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

/* byte i (static) of a run of dwords */
template <int N> __device__ __forceinline__ int png_byte(const u32 (&w)[N], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

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
        if ((u32)i < nb) p[i] = (uint8_t)png_byte(w, i);
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
        for (int k = 0; k < BPP; k++) up[k] = (u32)__builtin_amdgcn_update_dpp(0, (int)out[k], 0x138, 0xf, 0xf, false); /* wave_shr:1 -- lane r - 1; lane 0: 0 */
        const u32 q = t - (u32)lane;
        if (!live || t < (u32)lane || q >= n_chunks) continue;
        const u32 nb = min((u32)CB, d.row_bytes - q * CB);
        if (lane == 0 && above) png_load_run(above + (unsigned long long)q * CB, nb, up);
        u32 raw[BPP];
        png_load_run(cur + (unsigned long long)q * CB, nb, raw);
        int o[CB];
#pragma unroll
        for (int i = 0; i < CB; i++) {
            const int a = i >= BPP ? o[i - BPP] : png_byte(out, 3 * BPP + i);
            const int c = i >= BPP ? png_byte(up, i - BPP) : png_byte(corner, 3 * BPP + i);
            o[i] = ffhip_png_unfilter_byte(ft, png_byte(raw, i), a, png_byte(up, i), c);
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
            for (int j = 0; j < 4; j++) v[j] = ffhip_png_bgra((u32)png_byte(w, 3 * j + 2), (u32)png_byte(w, 3 * j + 1), (u32)png_byte(w, 3 * j), 255u);
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

thread_local int t_png_last[2];     /* ffhip_debug_png_last */
thread_local double t_png_times[4]; /* ffhip_debug_png_times */

/* FFHIP_PNG_TIMES: events around a part's upload, unfilter launches and expand launch; off, nothing is recorded */
struct PngClock {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    PngClock()
    {
        const char *v = FFHIP_ENV("FFHIP_PNG_TIMES");
        on = v && v[0] && v[0] != '0';
        for (int k = 0; on && k < 4; k++)
            if (hipEventCreate(&ev[k]) != hipSuccess) on = false;
    }
    ~PngClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t st) { if (on) (void)hipEventRecord(ev[k], st); }
    void add() /* behind the part's synchronisation */
    {
        for (int k = 0; on && k < 3; k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) t_png_times[k + 1] += ms;
        }
    }
};

size_t png_place(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

size_t png_part_budget()
{
    const char *v = FFHIP_ENV("FFHIP_PNG_PART_BYTES");
    const long long b = v ? atoll(v) : 0;
    return b > 0 ? (size_t)b : (size_t)1 << 30;
}

struct PngPartFile { int idx; size_t rows_off, palette_off; };

/* One part: files pf[] of the call, `bytes` of staging (their filtered pictures, then the palettes) */
int png_run_part(const std::vector<PngPartFile> &part, size_t bytes, const std::vector<ffhip_png_file> &pf, const uint8_t *const *files, const size_t *lens,
                 int n_threads, uint8_t *const *d_bgra, const int64_t *pitch, int *status, void *stream, PngClock &clock)
{
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 4; k++) clock.mark(k, st); /* a part that launches nothing has empty intervals */
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
    clock.mark(0, st);
    FFHIP_CHECK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
    for (int k = 1; k < 4; k++) clock.mark(k, st);
    std::vector<PngUnfDesc> unf;
    std::vector<PngExpDesc> exp;
    unsigned long long total = 0;
    for (const PngPartFile &p : part) {
        if (status[p.idx]) continue;
        const ffhip_png_file &f = pf[(size_t)p.idx];
        const ffhip_png_info &info = f.info;
        PngExpDesc e;
        memset(&e, 0, sizeof(e));
        e.rows = dev + p.rows_off;
        e.dst = d_bgra[p.idx];
        e.pitch = pitch[p.idx];
        e.palette = info.color_type == 3 ? (const u32 *)(dev + p.palette_off) : nullptr;
        e.width = (u32)info.width;
        e.height = (u32)info.height;
        e.groups_x = (e.width + 3) / 4;
        e.rule = f.rule;
        unsigned long long at = 0;
        for (int q = 0; q < 7; q++) {
            e.pass_off[q] = at;
            e.pass_pitch[q] = (u32)info.pass_row_bytes[q] + 1;
            if (!info.pass_rows[q]) continue;
            PngUnfDesc u;
            u.sub = dev + p.rows_off + at;
            u.rows = (u32)info.pass_rows[q];
            u.row_bytes = (u32)info.pass_row_bytes[q];
            u.bpp = (u32)ffhip_png_bpp(info.color_type, info.bit_depth);
            u.n_bands = (u.rows + PNG_BAND - 1) / PNG_BAND;
            unf.push_back(u);
            at += (unsigned long long)e.pass_pitch[q] * u.rows;
        }
        e.first_wg = (u32)total;
        e.n_wgs = (u32)(((unsigned long long)e.groups_x * e.height + PNG_EXPAND_THREADS - 1) / PNG_EXPAND_THREADS); /* < 2^22: both sides below 2^16 */
        total += e.n_wgs;
        exp.push_back(e);
    }
    if (exp.empty()) return FFHIP_OK;
    if (total > 0xffffffffULL) return FFHIP_EINVAL;
    /* the sub-images with the most bands first: the items that have a band l are then the first cnt(l) records, and level l is the
     * workgroups [0, cnt(l)) of the records themselves -- a workgroup's item is its index, so this table needs no second one */
    std::stable_sort(unf.begin(), unf.end(), [](const PngUnfDesc &x, const PngUnfDesc &y) { return x.n_bands > y.n_bands; });
    uint8_t *d_unf = nullptr;
    int rc = ffhip_items_stage(SCRATCH_PNG + 1, stream, unf.data(), unf.size() * sizeof(PngUnfDesc), 0, 0, &d_unf);
    if (rc) return rc;
    size_t cnt = unf.size();
    for (u32 level = 0; level < unf[0].n_bands; level++) {
        while (unf[cnt - 1].n_bands <= level) cnt--;
        rc = ffhip_items_launch(0, cnt, [&](unsigned grid_x, u32 wg_base) {
            PngUnfArgs a;
            a.desc = (const PngUnfDesc *)d_unf; a.level = level; a.wg_base = wg_base;
            hipLaunchKernelGGL(k_png_unfilter, dim3(grid_x), dim3(PNG_BAND), 0, st, a);
        });
        if (rc) return rc;
        t_png_last[1]++;
    }
    for (int k = 2; k < 4; k++) clock.mark(k, st);
    const PngExpDesc *d_exp = nullptr;
    u32 *d_table = nullptr;
    rc = ffhip_items_upload(SCRATCH_PNG + 2, stream, exp, total, &d_exp, &d_table);
    if (rc) return rc;
    rc = ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        PngExpArgs a;
        a.desc = d_exp; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_png_expand, dim3(grid_x), dim3(PNG_EXPAND_THREADS), 0, st, a);
    });
    clock.mark(3, st);
    return rc;
}

} // namespace

extern "C" int ffhip_png_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                             const int64_t *pitch, ffhip_png_info *info_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    std::vector<ffhip_png_file> pf((size_t)n);
    ffhip_parallel_for(n, n_threads, [&](int i) {
        ffhip_png_file &f = pf[(size_t)i];
        status[i] = files[i] && lens[i] ? ffhip_png_open(files[i], lens[i], &f) : FFHIP_EINVAL;
        if (status[i]) memset(&f.info, 0, sizeof(f.info));
        if (info_out) info_out[i] = f.info;
        if (status[i]) return;
        /* what k_png_expand asks of an output: whole 16-byte stores */
        if (!d_bgra[i] || ((uintptr_t)d_bgra[i] & 15) || pitch[i] < 4LL * f.info.width || (pitch[i] & 15) || pitch[i] > 0x7fffffffLL) status[i] = FFHIP_EINVAL;
    });
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    t_png_last[0] = t_png_last[1] = 0;
    for (double &t : t_png_times) t = 0;
    PngClock clock;
    const size_t budget = png_part_budget();
    int rc = FFHIP_OK;
    for (int i = 0; i < n && rc == FFHIP_OK;) {
        std::vector<PngPartFile> part;
        size_t rows = 0, palettes = 0;
        for (; i < n; i++) {
            if (status[i]) continue;
            const size_t need = png_place((size_t)pf[(size_t)i].info.filtered_bytes);
            if (!part.empty() && rows + need > budget) break;
            part.push_back({i, rows, palettes});
            rows += need;
            if (pf[(size_t)i].info.color_type == 3) palettes += 1024;
        }
        if (part.empty()) break;
        for (PngPartFile &p : part) p.palette_off += rows;
        t_png_last[0]++;
        rc = png_run_part(part, rows + palettes, pf, files, lens, n_threads, d_bgra, pitch, status, stream, clock);
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream); /* the next part, and the next call, refill the staging */
        if (e != hipSuccess) {
            ffhip_note_hip_error((int)e, "hipStreamSynchronize");
            if (rc == FFHIP_OK) rc = FFHIP_EIO;
        } else {
            clock.add();
        }
    }
    if (rc) return rc;
    for (int k = 0; k < n; k++)
        if (status[k]) return status[k];
    return FFHIP_OK;
}

extern "C" int ffhip_debug_png_last(int out[2])
{
    if (!out) return FFHIP_EINVAL;
    out[0] = t_png_last[0];
    out[1] = t_png_last[1];
    return FFHIP_OK;
}

extern "C" int ffhip_debug_png_times(double out[4])
{
    if (!out) return FFHIP_EINVAL;
    for (int k = 0; k < 4; k++) out[k] = t_png_times[k];
    return FFHIP_OK;
}
