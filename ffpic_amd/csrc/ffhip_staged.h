/* ffhip_staged.h -- the host drive of the staged file decoders (ffhip_png_gpu.hip, ffhip_vp8l_gpu.hip, ffhip_webp_alpha_gpu.hip; DESIGN.md
 * 4.28).  Such a call cuts its files into PARTS under a byte budget; of a part, host threads fill the pinned staging, one copy uploads it,
 * a BANDED kernel walks every item in bands of rows, one launch per band level, a GATHER kernel writes the pictures, four pixels to a
 * lane, and the stream is synchronised before the next part refills the staging.  Four stage times are taken by events.  What differs
 * between the decoders -- what a part's budget sums, what the host threads do, the records -- stays in their files. */
#ifndef FFHIP_STAGED_H
#define FFHIP_STAGED_H

#include "ffhip_items.h"
#include "ffhip_parts.h" /* ffhip_part_budget */
#include "ffhip_wave.h"

#include <algorithm>
#include <stdlib.h>

/* A *_TIMES switch: events around a part's upload, banded launches and gather launch, their intervals added into times[1..3]; off,
 * nothing is created or recorded.  `v` is the switch's value: FFHIP_ENV keeps a static per call site, so the caller reads it */
struct StageClock {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on;
    double *times;
    StageClock(const char *v, double *times4) : on(v && v[0] && v[0] != '0'), times(times4)
    {
        for (int k = 0; on && k < 4; k++)
            if (hipEventCreate(&ev[k]) != hipSuccess) on = false;
    }
    StageClock(const StageClock &) = delete;
    ~StageClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark_from(int k, hipStream_t st) /* the marks from k on: a part that launches nothing more has empty intervals */
    {
        for (; on && k < 4; k++) (void)hipEventRecord(ev[k], st);
    }
    void add() /* behind the part's synchronisation */
    {
        for (int k = 0; on && k < 3; k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) times[k + 1] += ms;
        }
    }
};

/* behind a part's last enqueue; rc is the part's so far -> the call's */
inline int ffhip_part_end(int rc, void *stream, StageClock &clock)
{
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream); /* the next part, and the next call, refill the staging */
    if (e != hipSuccess) {
        ffhip_note_hip_error((int)e, "hipStreamSynchronize");
        return rc == FFHIP_OK ? FFHIP_EIO : rc;
    }
    clock.add();
    return rc;
}

/* The banded kernel over rec[], each with n_bands bands that depend on each other top to bottom.  The items with the most bands go
 * first: the items that have a band l are then the first cnt(l) records, and level l is the workgroups [0, cnt(l)) of the records
 * themselves -- a workgroup's item is its index, so the records need no per-workgroup table.  The records go up through scratch `kind`;
 * launch(level, d_records, grid_x, wg_base) enqueues one launch; *levels counts the levels launched */
template <class Rec, class Launch> int ffhip_banded_launches(int kind, void *stream, std::vector<Rec> &rec, int *levels, Launch launch)
{
    if (rec.empty()) return FFHIP_OK;
    std::stable_sort(rec.begin(), rec.end(), [](const Rec &x, const Rec &y) { return x.n_bands > y.n_bands; });
    uint8_t *d_rec = nullptr;
    int rc = ffhip_items_stage(kind, stream, rec.data(), rec.size() * sizeof(Rec), 0, 0, &d_rec);
    if (rc) return rc;
    size_t cnt = rec.size();
    for (u32 level = 0; level < rec[0].n_bands; level++) {
        while (rec[cnt - 1].n_bands <= level) cnt--;
        rc = ffhip_items_launch(0, cnt, [&](unsigned grid_x, u32 wg_base) { launch(level, (const Rec *)d_rec, grid_x, wg_base); });
        if (rc) return rc;
        ++*levels;
    }
    return FFHIP_OK;
}

/* a gather kernel's workgroup; a lane owns four consecutive pixels of a row */
constexpr int FFHIP_GATHER_THREADS = 256;

/* a gather record whose width and height are set: its groups of four and its workgroups, behind the *total laid out so far */
template <class Desc> void ffhip_gather_place(Desc &d, unsigned long long *total)
{
    d.groups_x = (d.width + 3) / 4;
    d.first_wg = (u32)*total;
    d.n_wgs = (u32)(((unsigned long long)d.groups_x * d.height + FFHIP_GATHER_THREADS - 1) / FFHIP_GATHER_THREADS);
    *total += d.n_wgs;
}

/* the records and their table through scratch `kind`, then launch(d_desc, d_table, grid_x, wg_base) over the `total` workgroups */
template <class Desc, class Launch> int ffhip_gather_launch(int kind, void *stream, const std::vector<Desc> &desc, unsigned long long total, Launch launch)
{
    if (total > 0xffffffffULL) return FFHIP_EINVAL;
    const Desc *d_desc = nullptr;
    u32 *d_table = nullptr;
    const int rc = ffhip_items_upload(kind, stream, desc, total, &d_desc, &d_table);
    if (rc) return rc;
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) { launch(d_desc, d_table, grid_x, wg_base); });
}

/* what a gather kernel asks of a BGRA output: whole 16-byte stores */
inline bool ffhip_bgra_takes_stores16(const uint8_t *p, int64_t pitch, int64_t width)
{
    return p && !((uintptr_t)p & 15) && pitch >= 4 * width && !(pitch & 15) && pitch <= 0x7fffffffLL;
}

/* a debug getter's body: a thread's array out */
template <class T, int N> int ffhip_copy_out(T *out, const T (&from)[N])
{
    if (!out) return FFHIP_EINVAL;
    for (int k = 0; k < N; k++) out[k] = from[k];
    return FFHIP_OK;
}

#endif
