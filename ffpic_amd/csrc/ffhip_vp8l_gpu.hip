/* ffhip_vp8l_gpu.hip -- lossless WebP files to BGRA pictures on the device (include/ffpic_hip.h, "lossless WebP").  Host
 * threads decode the prefix codes, copies and colour cache (ffhip_vp8l.c) straight into a part's pinned staging: a file's RESIDUAL image,
 * its predictor and cross-colour block images and its palette; one upload; k_vp8l_predict undoes the predictor in place, k_vp8l_finish
 * undoes what is left and writes the pictures.  Both kernels compile the functions of ffhip_vp8l_body.h, as ffhip_vp8l_picture does on the
 * host, and neither has an error path: what a file can be refused for is seen on the host.  How a part is driven -- the launch per band
 * level, the gather launch, the end of a part, the stage clock -- is ffhip_staged.h's; the cut into parts is here, and so is the block of
 * functions that ffhip_webp_alpha_gpu.hip borrows (ffhip_vp8l_internal.h).
 *
 * k_vp8l_predict, in the form of k_png_unfilter.  An item is a file, cut into bands of 64 rows; a wave takes one band, lane r its row r.
 * A row is walked in CHUNKS of four pixels (16 bytes), and the lanes are skewed by TWO chunks: at step t lane r reconstructs chunk t - 2r.
 * A chunk's last pixel has the first pixel of the NEXT chunk above as its TR, so the lane above must have finished chunk q + 1 when this
 * lane starts chunk q.  A lane keeps its last two chunks and hands them down by DPP wave_shr:1 -- the older one whole (T of the four
 * pixels), of the newer one the first pixel (TR of the last): five moves per step; TL of the first pixel is the older chunk's last pixel
 * of the step before, kept in a register.  The first pixel of the lane's own row is kept too: it is the TR of the row's last pixel.  Lane 0
 * reads the row above from memory, where the launch before has written it: bands depend on each other top to bottom, and level l of
 * every file is one launch.  No spin-waits, no counters.
 *   The mode is constant over a chunk and differs between lanes.  Chosen by instruction count: ONE switch per chunk
 * (ffhip_vp8l_predict_chunk), the lanes of a wave walking the arms their modes name one after the other.  The kernel is 1 784
 * instructions, about 1 500 of them the thirteen arms of four pixels each (mode 13's clamps and Select's two v_sad_u8 a pixel the longest);
 * the select form -- every mode computed, the lane's own picked -- would issue all of them at every step of every wave, where the switch
 * issues the arms of the modes PRESENT among the 64 lanes and two branch instructions an arm, so it is never more and mostly far less:
 * encoded pictures hold runs of one mode down a column of blocks.  Families by whether the mode reads L would save nothing, since the four
 * pixels of a chunk hang on each other through L in ten of the thirteen arms, and it is that chain, not the issue rate, that an arm costs.
 *   The pointwise transforms undone BEFORE the predictor (cross-colour, in the order libwebp's encoder writes) are applied to the residual
 * as it is loaded.
 *
 * k_vp8l_finish.  The gather form of k_png_expand: a lane owns four consecutive output pixels of a row, applies the pointwise transforms
 * behind the predictor in the file's order, looks a colour-indexed file's pixels up in the palette (2, 4 or 8 to a word), applies the
 * alpha rule and makes one 16-byte store.  A picture's last partial group of four is stored pixel by pixel. */
#include "ffhip_staged.h"
#include "ffhip_vp8l_internal.h"

#include <chrono>
#include <stdlib.h>

namespace {

constexpr int VP8L_BAND = 64;
constexpr int VP8L_SKEW = 2; /* chunks between a lane and the lane above it */
constexpr int VP8L_FINISH_THREADS = FFHIP_GATHER_THREADS;

/* one file's residual image, to be predicted in place */
struct Vp8lPredDesc {
    u32 *res;            /* rows x width words */
    const u32 *modes;    /* the predictor's block image */
    const u32 *cross;    /* the cross-colour block image, where a step before the predictor reads it */
    u32 width, rows, n_bands;
    ffhip_vp8l_steps steps;
};
struct Vp8lPredArgs {
    const Vp8lPredDesc *desc; /* sorted by n_bands, largest first: the items with a band `level` are the first of them */
    u32 level, wg_base;
};

/* one file's picture */
struct Vp8lFinDesc {
    const u32 *res;      /* the residual image with the predictor undone: rows of res_width words */
    uint8_t *dst;
    int64_t pitch;
    const u32 *cross, *palette;
    u32 width, height, res_width, groups_x;
    u32 first_wg, n_wgs;
    ffhip_vp8l_steps steps;
};
struct Vp8lFinArgs {
    const Vp8lFinDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
};

struct __attribute__((packed, aligned(4))) Vp8lQuad { u32 w[4]; }; /* four words at any word address */

/* n <= 4 words at p -> w, zero behind them */
__device__ __forceinline__ void vp8l_load(const u32 *p, int n, u32 (&w)[4])
{
    if (n == 4) {
        const Vp8lQuad v = *(const Vp8lQuad *)p;
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = v.w[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = k < n ? p[k] : 0u;
}

/* One band.  Every lane runs every step, whatever its row: the cross-lane moves want the whole wave */
__global__ __launch_bounds__(VP8L_BAND) void k_vp8l_predict(Vp8lPredArgs a)
{
    const Vp8lPredDesc d = a.desc[a.wg_base + blockIdx.x];
    const int lane = (int)threadIdx.x;
    const u32 band = a.level, width = d.width;
    const u32 row = band * VP8L_BAND + (u32)lane;
    const bool live = row < d.rows;
    u32 *cur = d.res + (unsigned long long)(live ? row : 0) * width;
    const u32 *above = band ? d.res + ((unsigned long long)band * VP8L_BAND - 1) * width : nullptr; /* lane 0's row above */
    const u32 n_chunks = (width + 3) / 4;
    const int pbits = d.steps.predictor_bits, cbits = d.steps.cross_bits;
    const u32 *mode_row = d.modes + (unsigned long long)(row >> pbits) * d.steps.predictor_bx;
    const u32 *cross_row = d.cross ? d.cross + (unsigned long long)(row >> cbits) * d.steps.cross_bx : nullptr;
    u32 older[4] = {0, 0, 0, 0}, newer[4] = {0, 0, 0, 0}; /* the lane's last two chunks */
    u32 corner = 0, first = 0;                            /* above left of the next chunk; the row's first pixel */
    const u32 start = (u32)(VP8L_SKEW * lane);
    for (u32 t = 0; t < n_chunks + VP8L_SKEW * (VP8L_BAND - 1); t++) {
        u32 up[6];
#pragma unroll
        for (int k = 0; k < 4; k++) up[1 + k] = wave_shr1(older[k]);
        up[5] = wave_shr1(newer[0]);
        if (t < start) continue;
        const u32 q = t - start;
#pragma unroll
        for (int k = 0; k < 4; k++) older[k] = newer[k]; /* a finished lane goes on shifting: the lane below still reads its last chunks */
        if (!live || q >= n_chunks) continue;
        const u32 x0 = 4 * q;
        const int n = (int)min(4u, width - x0);
        if (lane == 0 && above) {
            u32 w4[4];
            vp8l_load(above + x0, n, w4);
#pragma unroll
            for (int k = 0; k < 4; k++) up[1 + k] = w4[k];
            up[5] = x0 + 4 < width ? above[x0 + 4] : 0u;
        }
        up[0] = corner;
        corner = up[4];
        u32 res[4], out[4] = {0, 0, 0, 0};
        vp8l_load(cur + x0, n, res);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s >= (int)d.steps.n_pre) break;
            const int type = d.steps.pre[s];
            const u32 m = type == FFHIP_VP8L_CROSS_COLOR ? cross_row[x0 >> cbits] : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) res[j] = type == FFHIP_VP8L_CROSS_COLOR ? ffhip_vp8l_cross(res[j], m) : ffhip_vp8l_add_green(res[j]);
        }
        const bool last = q + 1 == n_chunks;
        if (last && q) { /* the row's last pixel: its TR is the row's own first pixel.  A row of one chunk: tr_own */
#pragma unroll
            for (int k = 2; k < 6; k++)
                if (k == n + 1) up[k] = first;
        }
        const int block = row ? ffhip_vp8l_mode_of(mode_row[x0 >> pbits]) : 1;
        ffhip_vp8l_predict_chunk(q ? block : row ? 2 : 0, block, n, n_chunks == 1 ? n - 1 : 0, res, newer[3], up, out);
        if (q == 0) first = out[0];
#pragma unroll
        for (int k = 0; k < 4; k++) newer[k] = out[k];
        if (n == 4) {
            Vp8lQuad v;
#pragma unroll
            for (int k = 0; k < 4; k++) v.w[k] = out[k];
            *(Vp8lQuad *)(cur + x0) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < n) cur[x0 + (u32)k] = out[k];
        }
    }
}

__global__ __launch_bounds__(VP8L_FINISH_THREADS) void k_vp8l_finish(Vp8lFinArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const Vp8lFinDesc *d = a.desc + item;
    const u32 width = d->width, gx = d->groups_x, rw = d->res_width;
    const u32 g = (wg - d->first_wg) * VP8L_FINISH_THREADS + threadIdx.x; /* groups_x x height < 2^28 */
    if (g >= gx * d->height) return;
    const u32 y = g / gx, x0 = 4 * (g - y * gx);
    const int n = (int)min(4u, width - x0);
    const ffhip_vp8l_steps steps = d->steps;
    const u32 *row = d->res + (unsigned long long)y * rw;
    const u32 opaque = steps.has_alpha ? 0u : 0xff000000u;
    u32 v[4] = {0, 0, 0, 0};
    if (!steps.has_index) {
        vp8l_load(row + x0, n, v);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s >= (int)steps.n_post) break;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = ffhip_vp8l_pointwise(steps.post[s], v[j], min(x0 + (u32)j, width - 1), y, &steps, d->cross);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 x = min(x0 + (u32)j, width - 1), xp = x >> steps.index_bits;
            u32 word = row[xp];
#pragma unroll
            for (int s = 0; s < 2; s++)
                if (s < (int)steps.n_post) word = ffhip_vp8l_pointwise(steps.post[s], word, xp, y, &steps, d->cross);
            v[j] = ffhip_vp8l_index(word, x, steps.index_bits, d->palette);
        }
    }
    uint8_t *out = d->dst + (long long)y * d->pitch + 4ll * x0;
    if (n == 4) {
        *(u32x4 *)out = u32x4{v[0] | opaque, v[1] | opaque, v[2] | opaque, v[3] | opaque};
    } else {
        for (int j = 0; j < n; j++) ((u32 *)out)[j] = v[j] | opaque;
    }
}

thread_local int t_vp8l_last[3];     /* ffhip_debug_vp8l_last */
thread_local double t_vp8l_times[4]; /* ffhip_debug_vp8l_times */

size_t vp8l_res_bytes(const ffhip_vp8l_file &f)
{
    return 4 * (size_t)(f.device_form ? f.info.residual_width : f.info.width) * (size_t)f.info.height;
}
size_t vp8l_side_bytes(const ffhip_vp8l_file &f)
{
    if (!f.device_form) return 0;
    return ffhip_up(4 * (size_t)f.predictor_words, 16) + ffhip_up(4 * (size_t)f.cross_words, 16) + (f.steps.has_index ? 1024 : 0);
}

/* One part: files pf[] of the call, `bytes` of staging.  The clock (FFHIP_VP8L_TIMES) stands around the upload, the predict launches and
 * the finish launch */
int vp8l_run_part(const std::vector<Vp8lPartFile> &part, size_t bytes, const std::vector<ffhip_vp8l_file> &pf, int n_threads, uint8_t *const *d_bgra,
                  const int64_t *pitch, int *status, void *stream, StageClock &clock)
{
    hipStream_t st = (hipStream_t)stream;
    clock.mark_from(0, st);
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_VP8L, stream, bytes + 64);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_VP8L, stream, bytes / 4 + 16);
    if (!pin || !dev) return FFHIP_ENOMEM;
    const auto t0 = std::chrono::steady_clock::now();
    ffhip_parallel_for((int)part.size(), n_threads, [&](int k) { status[part[(size_t)k].idx] = vp8l_stage_file(pf[(size_t)part[(size_t)k].idx], part[(size_t)k], pin); });
    t_vp8l_times[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    clock.mark_from(0, st);
    FFHIP_CHECK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
    clock.mark_from(1, st);
    return vp8l_enqueue_part(part, dev, pf.data(), d_bgra, pitch, status, stream, SCRATCH_VP8L, t_vp8l_last + 1, &clock);
}

} // namespace

/* ---- lent to ffhip_webp_alpha_gpu.hip, as ffhip_vp8l_internal.h describes: from here to the mark below ---- */

size_t vp8l_part_add(std::vector<Vp8lPartFile> &part, const ffhip_vp8l_file &f, int idx, size_t *res, size_t *side)
{
    Vp8lPartFile p{idx, *res, *side, 0, 0};
    p.cross_off = p.modes_off + (f.device_form ? ffhip_up(4 * (size_t)f.predictor_words, 16) : 0);
    p.palette_off = p.cross_off + (f.device_form ? ffhip_up(4 * (size_t)f.cross_words, 16) : 0);
    part.push_back(p);
    *res += ffhip_up(vp8l_res_bytes(f), 16);
    *side += vp8l_side_bytes(f);
    return *res + *side;
}

void vp8l_part_seal(std::vector<Vp8lPartFile> &part, size_t res)
{
    for (Vp8lPartFile &p : part) { p.modes_off += res; p.cross_off += res; p.palette_off += res; }
}

int vp8l_stage_file(const ffhip_vp8l_file &f, const Vp8lPartFile &p, uint8_t *pin)
{
    if (f.device_form) {
        const int rc = ffhip_vp8l_read_residual(&f, (uint32_t *)(pin + p.res_off));
        if (f.predictor_words) memcpy(pin + p.modes_off, f.predictor_image, 4 * (size_t)f.predictor_words);
        if (f.cross_words) memcpy(pin + p.cross_off, f.cross_image, 4 * (size_t)f.cross_words);
        if (f.steps.has_index) memcpy(pin + p.palette_off, f.palette, 1024);
        return rc;
    }
    /* colour indexing behind another transform: every step on the host, the pixels uploaded */
    uint32_t *res = (uint32_t *)malloc(4 * (size_t)f.info.residual_width * (size_t)f.info.height);
    int rc = res ? ffhip_vp8l_read_residual(&f, res) : FFHIP_ENOMEM;
    if (!rc) rc = ffhip_vp8l_invert_host(&f, res, (uint32_t *)(pin + p.res_off));
    free(res);
    return rc;
}

int vp8l_enqueue_part(const std::vector<Vp8lPartFile> &part, uint8_t *dev, const ffhip_vp8l_file *pf, uint8_t *const *d_bgra, const int64_t *pitch,
                      const int *status, void *stream, int kind, int counts[2], StageClock *clock)
{
    hipStream_t st = (hipStream_t)stream;
    std::vector<Vp8lPredDesc> pred;
    std::vector<Vp8lFinDesc> fin;
    unsigned long long total = 0;
    for (const Vp8lPartFile &p : part) {
        if (status[p.idx]) continue;
        const ffhip_vp8l_file &f = pf[p.idx];
        Vp8lFinDesc e;
        memset(&e, 0, sizeof(e));
        e.res = (const u32 *)(dev + p.res_off);
        e.dst = d_bgra[p.idx];
        e.pitch = pitch[p.idx];
        e.width = (u32)f.info.width;
        e.height = (u32)f.info.height;
        e.res_width = e.width;
        e.steps.has_alpha = (uint8_t)f.info.has_alpha;
        if (f.device_form) {
            e.res_width = (u32)f.info.residual_width;
            e.steps = f.steps;
            e.cross = f.cross_words ? (const u32 *)(dev + p.cross_off) : nullptr;
            e.palette = f.steps.has_index ? (const u32 *)(dev + p.palette_off) : nullptr;
            if (f.steps.has_predictor) {
                Vp8lPredDesc u;
                memset(&u, 0, sizeof(u));
                u.res = (u32 *)(dev + p.res_off);
                u.modes = (const u32 *)(dev + p.modes_off);
                u.cross = e.cross;
                u.width = e.res_width;
                u.rows = e.height;
                u.n_bands = (u.rows + VP8L_BAND - 1) / VP8L_BAND;
                u.steps = f.steps;
                pred.push_back(u);
            }
        } else {
            counts[1]++;
        }
        ffhip_gather_place(e, &total); /* n_wgs < 2^20: both sides at most 2^14 */
        fin.push_back(e);
    }
    if (fin.empty()) return FFHIP_OK;
    int rc = ffhip_banded_launches(kind + 1, stream, pred, &counts[0], [&](u32 level, const Vp8lPredDesc *d_pred, unsigned grid_x, u32 wg_base) {
        Vp8lPredArgs a;
        a.desc = d_pred; a.level = level; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_vp8l_predict, dim3(grid_x), dim3(VP8L_BAND), 0, st, a);
    });
    if (rc) return rc;
    if (clock) clock->mark_from(2, st);
    rc = ffhip_gather_launch(kind + 2, stream, fin, total, [&](const Vp8lFinDesc *d_fin, const u32 *d_table, unsigned grid_x, u32 wg_base) {
        Vp8lFinArgs a;
        a.desc = d_fin; a.wg_item = d_table; a.wg_base = wg_base;
        hipLaunchKernelGGL(k_vp8l_finish, dim3(grid_x), dim3(VP8L_FINISH_THREADS), 0, st, a);
    });
    if (clock) clock->mark_from(3, st);
    return rc;
}

/* ---- the end of what is lent ---- */

extern "C" int ffhip_vp8l_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                              const int64_t *pitch, ffhip_vp8l_info *info_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    n_threads = ffhip_host_threads(n_threads);
    Vp8lFiles opened((size_t)n);
    std::vector<ffhip_vp8l_file> &pf = opened.v;
    const auto t_open = std::chrono::steady_clock::now();
    ffhip_parallel_for(n, n_threads, [&](int i) {
        ffhip_vp8l_file &f = pf[(size_t)i];
        memset(&f, 0, sizeof(f));
        status[i] = files[i] && lens[i] ? ffhip_vp8l_open(files[i], lens[i], &f) : FFHIP_EINVAL;
        if (info_out) info_out[i] = f.info;
        if (status[i]) return;
        if (!ffhip_bgra_takes_stores16(d_bgra[i], pitch[i], f.info.width)) status[i] = FFHIP_EINVAL; /* k_vp8l_finish's */
    });
    const double open_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_open).count();
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    t_vp8l_last[0] = t_vp8l_last[1] = t_vp8l_last[2] = 0;
    for (double &t : t_vp8l_times) t = 0;
    t_vp8l_times[0] = open_ms; /* the headers, transform lists and their sub-images */
    StageClock clock(FFHIP_ENV("FFHIP_VP8L_TIMES"), t_vp8l_times);
    const size_t budget = ffhip_part_budget(FFHIP_ENV("FFHIP_VP8L_PART_BYTES"));
    int rc = FFHIP_OK;
    for (int i = 0; i < n && rc == FFHIP_OK;) {
        std::vector<Vp8lPartFile> part;
        size_t res = 0, side = 0;
        for (; i < n; i++) {
            if (status[i]) continue;
            const ffhip_vp8l_file &f = pf[(size_t)i];
            if (!part.empty() && res + ffhip_up(vp8l_res_bytes(f), 16) > budget) break;
            vp8l_part_add(part, f, i, &res, &side);
        }
        if (part.empty()) break;
        vp8l_part_seal(part, res);
        t_vp8l_last[0]++;
        rc = ffhip_part_end(vp8l_run_part(part, res + side, pf, n_threads, d_bgra, pitch, status, stream, clock), stream, clock);
    }
    if (rc) return rc;
    for (int k = 0; k < n; k++)
        if (status[k]) return status[k];
    return FFHIP_OK;
}

extern "C" int ffhip_debug_vp8l_last(int out[3]) { return ffhip_copy_out(out, t_vp8l_last); }

extern "C" int ffhip_debug_vp8l_times(double out[4]) { return ffhip_copy_out(out, t_vp8l_times); }
