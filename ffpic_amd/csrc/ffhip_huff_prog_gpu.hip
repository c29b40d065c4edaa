/*
 * ffhip_huff_prog_gpu.hip -- the progressive JPEG entropy front end ON the GPU.
 *
 * The host parses every file (ffhip_prog_parse: scan list, a table snapshot per scan), stages the bytes of every scan that is kept
 * (ffhip_prog_stage_scan: unstuffed, cut at the RSTn markers) into pinned memory and sorts the scans into dependency levels.  The device
 * runs k_jpeg_huff_prog once per level over all the files of the call: ONE LANE per (picture, scan, restart interval) -- a scan without
 * DRI is one lane.  The subsequence decoder of the baseline path does not carry over: a lane entering an AC refinement mid-stream cannot
 * know how many correction bits a block takes without that block's history, so refinement scans do not self-synchronise.  Parallelism
 * comes from the batch, from restart intervals and from the independent scans of a level.
 *
 * The lane's work is ffhip_prog_interval of ffhip_jpeg_prog_body.h, the function the host decoder runs: same bit reader, same block
 * addressing, same verdicts.  Optimised files carry their own tables per scan, so the lanes of a wave mostly hold different tables and
 * read them from global memory (struct huff: the 9-bit look-up, then the canonical-code walk); the distinct tables of the batch are
 * uploaded once each.
 */
#include "ffhip_internal.h"
#include "ffhip_jpeg_prog_internal.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <unordered_map>
#include <vector>

struct ProgArgs {
    const uint8_t *clean;          /* the staged bytes of every kept scan of the call */
    const uint32_t *seg;           /* interval bounds, per scan n_seg + 1 of them, relative to the scan's bytes */
    const struct huff *tabs;       /* the distinct tables of the call */
    const struct prog_scan *scans;
    const struct prog_pic *pics;
    const u32x2 *work;             /* (scan, interval) per lane, this level's */
    int16_t *plane[3];
    int *status;                   /* per picture: non-zero if some interval was malformed */
    uint32_t n_work;
    uint32_t lanes;                /* work items per 64-thread workgroup, 1..64 */
};

/* Scans of one level store to different int16 elements of the same block from different lanes (the DC scan and an AC band of a component,
 * two bands of it): distinct 2-byte locations written by byte-enabled vector stores, so no ordering is needed among them.  An AC
 * refinement reads and rewrites only its own band of its own blocks, a DC refinement only element 0; what they read was stored by an
 * earlier level = an earlier launch on the stream.  The verdict is an ordinary vector store of the same value from every lane that has one. */
__global__ __launch_bounds__(64) void k_jpeg_huff_prog(ProgArgs a)
{
    /* The lanes of a wave walk different scans with different tables, and the body is ordinary branching code, not the flat state machine of
     * k_jpeg_huff: lanes that sit in one wave run one after the other wherever they part ways.  So a level's work items are spread over as many
     * waves as the device holds before they share one: a.lanes items a wave (the host's choice by the length of the work list), the other
     * lanes of the wave idle. */
    const uint32_t gid = blockIdx.x * a.lanes + threadIdx.x;
    if (threadIdx.x >= a.lanes || gid >= a.n_work) return;
    const u32x2 w = a.work[gid];
    const struct prog_scan sc = a.scans[w.x];
    const struct prog_pic pc = a.pics[sc.pic];
    int16_t *const plane[3] = {a.plane[0], a.plane[1], a.plane[2]};
    if (ffhip_prog_interval(&sc, &pc, w.y, a.clean, a.seg, a.tabs, plane)) a.status[sc.pic] = FFHIP_EINVAL;
}

namespace {
struct ProgLayout { size_t o_seg, o_tabs, o_scans, o_pics, o_work, o_status, o_quant, total; };

uint64_t table_hash(const struct huff &t)
{
    const uint8_t *p = (const uint8_t *)&t.maxcode;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < offsetof(struct huff, present) - offsetof(struct huff, maxcode); i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
bool table_same(const struct huff &a, const struct huff &b)
{
    return !memcmp(&a.maxcode, &b.maxcode, offsetof(struct huff, present) - offsetof(struct huff, maxcode)); /* (look[] follows from the rest) */
}
} // namespace

/* k_max: per picture (k_maxes) or one for all.  counts[4]: progressive files, scans decoded, scans skipped, levels launched.  FFHIP_OK when the
 * batch ran, whatever the single files' verdicts in status[]; FFHIP_EINVAL: the call refuses the batch (nothing enqueued). */
int jpeg_progressive_batch_gpu_impl(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_jpeg_geom *geom,
                                    const ffhip_jpeg_geom *geoms, int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant,
                                    int k_max, const int *k_maxes, int *status, void *stream, const FfhipHuffThen *then, int counts[4])
{
    if (n < 0 || !geom || (n > 0 && (!files || !lens || !d_coef_y || !d_quant || !status)) || k_max < 0 || k_max > 63) return FFHIP_EINVAL;
    if (geom->ncomp == 3 && (!d_coef_u || !d_coef_v)) return FFHIP_EINVAL;
    if (geom->mcu_cols <= 0 || geom->mcu_rows <= 0 || geom->h < 1 || geom->v < 1 || geom->h * geom->v > 4 || (geom->ncomp != 1 && geom->ncomp != 3) ||
        (geom->ncomp == 1 && geom->h * geom->v != 1)) return FFHIP_EINVAL;
    std::vector<uint32_t> mcu_base((size_t)n + 1, 0u);
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_geom *gi = geoms ? &geoms[i] : geom;
        if (gi->ncomp != geom->ncomp || gi->h != geom->h || gi->v != geom->v || gi->mcu_cols <= 0 || gi->mcu_rows <= 0) return FFHIP_EINVAL;
        if (k_maxes && (k_maxes[i] < 0 || k_maxes[i] > 63)) return FFHIP_EINVAL;
        const size_t sum = (size_t)mcu_base[(size_t)i] + (size_t)gi->mcu_cols * gi->mcu_rows;
        if (sum * (size_t)(geom->h * geom->v) > 0x3fffffffu) return FFHIP_EINVAL; /* block indices stay in 32 bits */
        mcu_base[(size_t)i + 1] = (uint32_t)sum;
    }
    if (n == 0) return FFHIP_OK;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    n_threads = n_threads < 1 ? 1 : n_threads > 64 ? 64 : n_threads;
    hipStream_t st = (hipStream_t)stream;

    /* ---- host: parse, choose the scans, lay the upload out ---- */
    std::unique_ptr<struct prog_file[]> pf(new (std::nothrow) struct prog_file[(size_t)n]);
    if (!pf) return FFHIP_ENOMEM;
    struct Free { struct prog_file *p; int n; ~Free() { for (int i = 0; i < n; i++) ffhip_prog_free(&p[i]); } } free_tabs = {pf.get(), n};
    (void)free_tabs;
    std::vector<int> k_eff((size_t)n, 0);
    ffhip_parallel_for(n, n_threads, [&](int i) {
        status[i] = files[i] && lens[i] ? ffhip_prog_parse(files[i], lens[i], &pf[(size_t)i]) : FFHIP_EINVAL;
        if (status[i]) { memset(&pf[(size_t)i], 0, sizeof(struct prog_file)); return; }
        ffhip_jpeg_geom g;
        ffhip_jpeg_frame_geom(&pf[(size_t)i].fr, &g);
        if (!ffhip_jpeg_geom_same(&g, geoms ? &geoms[i] : geom)) {
            status[i] = FFHIP_EINVAL; /* another geometry */
            ffhip_prog_free(&pf[(size_t)i]);
            pf[(size_t)i].n_scans = 0;
            return;
        }
        k_eff[(size_t)i] = ffhip_prog_k_eff(&pf[(size_t)i], k_maxes ? k_maxes[i] : k_max);
    });
    std::vector<struct prog_scan> scans;
    std::vector<struct prog_pic> pics((size_t)n);
    std::vector<const struct huff *> uniq;
    std::unordered_map<uint64_t, std::vector<uint32_t>> by_hash;
    struct Src { int file, scan; };
    std::vector<Src> src;
    size_t clean_total = 0, seg_total = 0, work_total = 0;
    uint32_t max_level = 0;
    for (int i = 0; i < n; i++) {
        const ffhip_jpeg_geom *gi = geoms ? &geoms[i] : geom;
        pics[(size_t)i] = {(uint32_t)gi->ncomp, (uint32_t)gi->h, (uint32_t)gi->v, (uint32_t)gi->mcu_cols, (uint32_t)gi->mcu_rows, mcu_base[(size_t)i]};
        if (status[i]) continue;
        counts[0]++;
        struct prog_file &f = pf[(size_t)i];
        std::vector<uint32_t> tab_id((size_t)f.n_tabs, 0xffffffffu);
        for (int s = 0; s < f.n_scans; s++) {
            struct prog_scan sc = f.scan[s];
            if ((int)sc.ss > k_eff[(size_t)i]) { counts[2]++; continue; }
            counts[1]++;
            sc.pic = (uint32_t)i;
            sc.data = (uint32_t)clean_total;
            sc.seg_base = (uint32_t)seg_total;
            const bool reads_tables = !(sc.ss == 0 && sc.ah != 0);
            for (uint32_t k = 0; k < sc.ncomp && reads_tables; k++) { /* the distinct tables of the batch, by content */
                uint32_t &id = tab_id[sc.tab[k]];
                if (id == 0xffffffffu) {
                    const struct huff &t = f.tabs[sc.tab[k]];
                    std::vector<uint32_t> &same = by_hash[table_hash(t)];
                    for (uint32_t u : same)
                        if (table_same(*uniq[u], t)) id = u;
                    if (id == 0xffffffffu) {
                        id = (uint32_t)uniq.size();
                        uniq.push_back(&t);
                        same.push_back(id);
                    }
                }
                sc.tab[k] = id;
            }
            clean_total += (f.raw_len[s] + 15) & ~(size_t)15;
            seg_total += (size_t)sc.n_seg + 1;
            work_total += sc.n_seg;
            max_level = std::max(max_level, sc.level);
            if (clean_total > 0x7fffffffu || seg_total > 0x7fffffffu) return FFHIP_EINVAL;
            scans.push_back(sc);
            src.push_back({i, s});
        }
    }
    ProgLayout L;
    {
        size_t at = clean_total + 16;
        auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15) & ~(size_t)15; return o; };
        L.o_seg = take(seg_total * 4);
        L.o_tabs = take(uniq.size() * sizeof(struct huff));
        L.o_scans = take(scans.size() * sizeof(struct prog_scan));
        L.o_pics = take((size_t)n * sizeof(struct prog_pic));
        L.o_work = take(work_total * 8);
        L.o_status = take((size_t)n * 4);
        L.o_quant = take((size_t)n * 512);
        L.total = at;
    }
    FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO); /* the pinned stage may still be read by what `stream` holds */
    uint8_t *stage = ffhip_pinned_scratch(SCRATCH_HUFF_PROG, stream, L.total + 64);
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_HUFF_PROG, stream, (L.total + 3) / 4 + 16);
    if (!stage || !dev) return FFHIP_ENOMEM;

    /* ---- host: stage the scans; a scan with fewer restart intervals than it needs fails its file ---- */
    uint32_t *h_seg = (uint32_t *)(stage + L.o_seg);
    std::vector<char> scan_bad(scans.size(), 0); /* per scan: every thread writes flags of its own */
    ffhip_parallel_for((int)scans.size(), n_threads, [&](int q) {
        const struct prog_scan &sc = scans[(size_t)q];
        const struct prog_file &f = pf[(size_t)src[(size_t)q].file];
        const int s = src[(size_t)q].scan;
        if (ffhip_prog_stage_scan(stage + sc.data, f.raw[s], f.raw_len[s], h_seg + sc.seg_base, sc.n_seg) != sc.n_seg) scan_bad[(size_t)q] = 1;
    });
    for (size_t q = 0; q < scans.size(); q++)
        if (scan_bad[q]) status[scans[q].pic] = FFHIP_EINVAL;
    for (size_t u = 0; u < uniq.size(); u++) ((struct huff *)(stage + L.o_tabs))[u] = *uniq[u];
    if (!scans.empty()) memcpy(stage + L.o_scans, scans.data(), scans.size() * sizeof(struct prog_scan));
    memcpy(stage + L.o_pics, pics.data(), (size_t)n * sizeof(struct prog_pic));
    memset(stage + L.o_status, 0, (size_t)n * 4);
    for (int i = 0; i < n; i++) {
        uint16_t *q = (uint16_t *)(stage + L.o_quant) + (size_t)i * 256;
        if (status[i]) for (int k = 0; k < 256; k++) q[k] = 1;
        else memcpy(q, pf[(size_t)i].fr.quant, 512);
    }
    /* the work lists, level by level: the lanes of a level are independent of each other */
    std::vector<uint32_t> level_first((size_t)max_level + 2, 0u);
    {
        u32x2 *wk = (u32x2 *)(stage + L.o_work);
        uint32_t at = 0;
        for (uint32_t lv = 1; lv <= max_level; lv++) {
            level_first[lv] = at;
            for (size_t q = 0; q < scans.size(); q++) {
                if (scans[q].level != lv || status[scans[q].pic]) continue;
                for (uint32_t iv = 0; iv < scans[q].n_seg; iv++) { wk[at].x = (uint32_t)q; wk[at].y = iv; at++; }
            }
        }
        level_first[(size_t)max_level + 1] = at;
    }

    /* ---- device: one clear, one upload, a launch per level ---- */
    const size_t total_mcus = mcu_base[(size_t)n];
    FFHIP_CHECK(hipMemsetAsync(d_coef_y, 0, total_mcus * geom->h * geom->v * 128, st), FFHIP_EIO);
    if (geom->ncomp == 3) {
        FFHIP_CHECK(hipMemsetAsync(d_coef_u, 0, total_mcus * 128, st), FFHIP_EIO);
        FFHIP_CHECK(hipMemsetAsync(d_coef_v, 0, total_mcus * 128, st), FFHIP_EIO);
    }
    FFHIP_CHECK(hipMemcpyAsync(dev, stage, L.total, hipMemcpyHostToDevice, st), FFHIP_EIO);
    FFHIP_CHECK(hipMemcpyAsync(d_quant, dev + L.o_quant, (size_t)n * 512, hipMemcpyDeviceToDevice, st), FFHIP_EIO);
    ProgArgs a;
    a.clean = dev;
    a.seg = (const uint32_t *)(dev + L.o_seg);
    a.tabs = (const struct huff *)(dev + L.o_tabs);
    a.scans = (const struct prog_scan *)(dev + L.o_scans);
    a.pics = (const struct prog_pic *)(dev + L.o_pics);
    a.plane[0] = d_coef_y; a.plane[1] = d_coef_u; a.plane[2] = d_coef_v;
    a.status = (int *)(dev + L.o_status);
    const uint32_t resident = (uint32_t)std::max(1, ffhip_resident_waves((const void *)k_jpeg_huff_prog, 64)); /* waves the device holds at once */
    /* FFHIP_JPEG_PROG_LANES=1..64: that many work items a wave whatever the length of the work list (the tests' way to several items in one
     * wave without a batch of ten thousand scans) */
    const char *fl = FFHIP_ENV("FFHIP_JPEG_PROG_LANES");
    const uint32_t forced = fl && atoi(fl) >= 1 && atoi(fl) <= 64 ? (uint32_t)atoi(fl) : 0u;
    for (uint32_t lv = 1; lv <= max_level; lv++) {
        a.n_work = level_first[lv + 1] - level_first[lv];
        if (!a.n_work) continue;
        a.work = (const u32x2 *)(dev + L.o_work) + level_first[lv];
        a.lanes = forced ? forced : std::min(64u, std::max(1u, (a.n_work + resident - 1) / resident));
        hipLaunchKernelGGL(k_jpeg_huff_prog, dim3((a.n_work + a.lanes - 1) / a.lanes), dim3(64), 0, st, a);
        FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
        counts[3]++;
    }
    if (then) {
        std::vector<ffhip_jpeg_item> items(then->items, then->items + n);
        for (int i = 0; i < n; i++) jpeg_item_planes(&items[(size_t)i], d_coef_y, d_coef_u, d_coef_v, d_quant, mcu_base[(size_t)i], (size_t)i);
        const int rrc = jpeg_recon_items_by_rule(items.data(), then->rule, n, stream, 0);
        if (rrc) return rrc;
    }
    FFHIP_CHECK(hipMemcpyAsync(stage + L.o_status, dev + L.o_status, (size_t)n * 4, hipMemcpyDeviceToHost, st), FFHIP_EIO);
    FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO);
    for (int i = 0; i < n; i++)
        if (!status[i]) status[i] = ((const int *)(stage + L.o_status))[i];
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_progressive_batch_gpu(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_jpeg_geom *geom,
                                                int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant, int k_max, int *status,
                                                void *stream)
{
    int counts[4] = {0, 0, 0, 0};
    const int rc = jpeg_progressive_batch_gpu_impl(files, lens, n, n_threads, geom, nullptr, d_coef_y, d_coef_u, d_coef_v, d_quant, k_max, nullptr, status,
                                                   stream, nullptr, counts);
    const int last[5] = {counts[0], counts[1], counts[2], counts[3], 1};
    ffhip_prog_note_last(last);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}
