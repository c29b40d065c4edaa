/*
 * ffhip_hevc_plan_host.hip -- the host planner of ffhip_hevc_intra_recon: plain C++ that never touches the device.
 *
 * For a validated TU list: which luma window makes its groups contiguous runs (pick_window), the list sorted by plane (sort_by_plane),
 * the grouped kernel's schedule -- groups, slots, wait lists, tickets in dependency-depth order -- in the layout the device planner of
 * ffhip_hevc_plan_gpu.hip writes (plan_groups behind plan_with_window_search; ffhip_hevc_intra_plan is its public form), and the
 * wavefront levels of the levels form (intra_levels).  ffhip_hevc_intra.hip uploads and launches.
 */
#include "ffhip_hevc_plan.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct PlanMeta { uint32_t group, wait_begin, slot; uint8_t wait_count, signal, tile_ok; }; /* plan_groups: per TU */
/* plan_groups' pass 3: the threads' wait lists (TU ranges in order) as one, wait_begin made absolute, and the dependency depth of every group */
static void merge_waits(long long n_tus, const std::vector<std::vector<uint32_t>> &waits, PlanMeta *meta, size_t n_groups, std::vector<uint32_t> &gdepth,
                        GroupPlan &out)
{
    const int n_threads = (int)waits.size();
    size_t total_wait = 0;
    for (auto &w : waits) total_wait += w.size();
    out.wait.resize(std::max<size_t>(total_wait, 1));
    out.wait[0] = 0;
    gdepth.assign(n_groups, 0);
    size_t base = 0;
    for (int th = 0; th < n_threads; th++) {
        const long long lo = n_tus * th / n_threads, hi = n_tus * (th + 1) / n_threads;
        const std::vector<uint32_t> &w = waits[(size_t)th];
        if (!w.empty()) memcpy(out.wait.data() + base, w.data(), w.size() * sizeof(uint32_t));
        for (long long i = lo; i < hi; i++) {
            PlanMeta &m = meta[(size_t)i];
            uint32_t depth = gdepth[m.group];
            for (unsigned q = 0; q < m.wait_count; q++) depth = std::max(depth, gdepth[meta[w[m.wait_begin + q]].group] + 1);
            gdepth[m.group] = depth;
            m.wait_begin += (uint32_t)base;
        }
        base += w.size();
    }
}
/* plan_groups' last step: the tickets' order (by_depth: dependency depth, ties in decode order; else decode order), the group records, the slots */
static void order_and_emit(const ffhip_hevc_tu *tus, long long n_tus, const int win_log2[3], const int bw[3], const uint32_t jt_boff[3], const bool by_depth,
                           const PlanMeta *mp, const std::vector<uint32_t> &gcount, const std::vector<uint32_t> &gfirst, const std::vector<uint32_t> &gdepth,
                           int n_threads, GroupPlan &out)
{
    static thread_local std::vector<uint32_t> order, gbase;
    /* Tickets go out in dependency-depth order (ties: decode order), so the waves that hold tickets
     * are the ones near the ready front rather than thousands of groups ahead of it, polling.
     * Every group a group waits for has a smaller depth, hence a smaller ticket.  (Depths are only
     * trusted for contiguous groups; otherwise decode order, which pass 2 checked is valid.) */
    const size_t ng = gcount.size();
    order.resize(ng);
    for (size_t g = 0; g < ng; g++) order[g] = (uint32_t)g;
    if (by_depth) std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return gdepth[x] < gdepth[y]; });
    gbase.resize(ng);
    out.groups.resize(ng);
    uint32_t run = 0;
    for (size_t k = 0; k < ng; k++) {
        const uint32_t g = order[k];
        gbase[g] = run;
        u32x4 rec;
        rec.x = run;
        rec.y = gcount[g];
        rec.z = (uint32_t)win_log2[tus[gfirst[g]].cidx];
        rec.w = 0;
        out.groups[k] = rec;
        run += gcount[g];
    }
    out.sched.resize((size_t)n_tus * 3);
    static_assert(sizeof(ffhip_hevc_tu) == 32, "slot layout");
    const uint32_t *const gbasep = gbase.data();
    auto emit = [&](int th) {
        const long long lo = n_tus * th / n_threads, hi = n_tus * (th + 1) / n_threads;
        for (long long i = lo; i < hi; i++) {
            const PlanMeta &m = mp[(size_t)i];
            u32x4 *q = &out.sched[(size_t)(gbasep[m.group] + m.slot) * 3];
            memcpy(q, &tus[i], 32);
            q[2].x = m.wait_begin;
            q[2].y = (uint32_t)m.wait_count | ((uint32_t)m.signal << 8) | ((uint32_t)m.tile_ok << 9);
            q[2].z = (uint32_t)i;
            q[2].w = (jt_boff[tus[i].cidx] + (uint32_t)(tus[i].y >> 2) * (uint32_t)bw[tus[i].cidx] + (uint32_t)(tus[i].x >> 2)) * JT_STRIDE;
        }
    };
    ffhip_parallel_for(n_threads, n_threads, emit);
}

/* Cut the (validated) list into window-tile groups in order of first appearance and collect, per
 * TU, the TUs of OTHER groups it reads, whether some other group reads it, and whether all its
 * available neighbours inside the window were written by its own group (then the kernel may take
 * them from its LDS tile).  Returns false when some TU would wait for a group with a larger
 * ticket (window larger than the coding tree block, or an exotic list): the caller then tries a
 * smaller window or falls back to the level-synchronous form. */
static bool plan_groups(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], const int win_log2[3],
                        GroupPlan &out, const uint32_t jt_boff[3])
{
    /* scratch kept between calls: a picture's worth of maps is reallocated and refilled otherwise */
    static thread_local std::vector<int32_t> owner[3], gid_of[3];
    static thread_local std::vector<PlanMeta> meta;
    static thread_local std::vector<uint32_t> gcount, gdepth, gfirst;
    int bw[3], gw[3];
    for (int c = 0; c < 3; c++) {
        bw[c] = (pw[c] + 3) / 4;
        gw[c] = pw[c] > 0 ? ((pw[c] - 1) >> win_log2[c]) + 1 : 0;
        owner[c].assign((size_t)bw[c] * (size_t)((ph[c] + 3) / 4), -1);
        gid_of[c].assign((size_t)gw[c] * (size_t)(ph[c] > 0 ? ((ph[c] - 1) >> win_log2[c]) + 1 : 0), -1);
    }
    const auto T0 = std::chrono::steady_clock::now();
    meta.resize((size_t)n_tus);
    gcount.clear();
    gfirst.clear();
    /* ---- pass 1 (sequential, light): groups in order of first appearance, slot inside the group, block owners ----
     * contiguous: every group is one run of the list; then a group is complete before a later one starts,
     * which is what makes the dependency depths of pass 3 final when they are read */
    bool contiguous = true;
    uint32_t cur_group = ~0u;
    for (long long i = 0; i < n_tus; i++) {
        const ffhip_hevc_tu &t = tus[i];
        const int c = t.cidx, n = 1 << t.log2_size, wl = win_log2[c];
        int32_t &gslot = gid_of[c][(size_t)(t.y >> wl) * gw[c] + (t.x >> wl)];
        if (gslot < 0) {
            gslot = (int32_t)gcount.size();
            gcount.push_back(0);
            gfirst.push_back((uint32_t)i);
        } else if ((uint32_t)gslot != cur_group) {
            contiguous = false;
        }
        cur_group = (uint32_t)gslot;
        PlanMeta &m = meta[(size_t)i];
        m.group = cur_group; m.signal = 0; m.tile_ok = 1;
        m.slot = gcount[cur_group]++;
        int32_t *orow = owner[c].data() + (size_t)(t.y >> 2) * bw[c] + (t.x >> 2);
        for (int by = 0; by < n / 4; by++, orow += bw[c])
            for (int bx = 0; bx < n / 4; bx++) orow[bx] = (int32_t)i;
    }
    const auto T1 = std::chrono::steady_clock::now();
    /* ---- pass 2 (parallel over TU ranges): who reads whom.  The owner map is complete; a TU only
     * depends on TUs before it in the list (a block whose owner comes later held older content when
     * the sequential decoder looked at it) ---- */
    /* the scratch vectors are thread_local: worker threads must go through pointers taken here */
    PlanMeta *const mp = meta.data();
    const int32_t *const ownp[3] = {owner[0].data(), owner[1].data(), owner[2].data()};
    const char *pt = FFHIP_ENV("FFHIP_PLAN_THREADS");
    /* one thread unless asked: on the 16-core share of an MI355X box 2-8 threads were no faster
     * (2.5-5.0 ms against 2.7 ms for this pass on 172k TUs: thread start-up and the shared maps eat the gain) */
    const int n_threads = pt ? std::max(1, std::min(16, atoi(pt))) : 1;
    std::vector<std::vector<uint32_t>> waits((size_t)n_threads);
    std::atomic<bool> bad(false);
    auto scan = [&](int th) {
        const long long lo = n_tus * th / n_threads, hi = n_tus * (th + 1) / n_threads;
        std::vector<uint32_t> &w = waits[(size_t)th];
        w.reserve((size_t)(hi - lo) * 2);
        for (long long i = lo; i < hi; i++) {
            const ffhip_hevc_tu &t = tus[i];
            const int c = t.cidx, n = 1 << t.log2_size, wl = win_log2[c];
            PlanMeta &m = mp[(size_t)i];
            const uint32_t g = m.group;
            int32_t deps[72];
            int nd = 0;
            bool tile_ok = true;
            const int wx0 = (t.x >> wl) << wl, wy0 = (t.y >> wl) << wl, wsz = 1 << wl;
            const int32_t *own = ownp[c];
            auto dep = [&](int px, int py) {
                int32_t j = own[(size_t)(py >> 2) * bw[c] + (px >> 2)];
                if (j >= i) j = -1;
                const bool mine = j >= 0 && mp[(size_t)j].group == g;
                if (j >= 0 && !mine) {
                    bool dup = false;
                    for (int q = nd - 1; q >= 0 && !dup; q--) dup = deps[q] == j; /* neighbours repeat back to back */
                    if (!dup && nd < 72) deps[nd++] = j;
                }
                if (!mine && px >= wx0 && px < wx0 + wsz && py >= wy0 && py < wy0 + wsz) tile_ok = false; /* not in my LDS copy */
            };
            if (t.flags & 1) dep(t.x - 1, t.y - 1);
            for (int k = 0; k < 2 * n; k += 4) {
                if ((t.avail_top >> k) & 0xf) dep(t.x + k, t.y - 1);
                if ((t.avail_left >> k) & 0xf) dep(t.x - 1, t.y + k);
            }
            if (nd > 64) { bad = true; return; }
            m.tile_ok = tile_ok;
            m.wait_count = (uint8_t)nd;
            m.wait_begin = (uint32_t)w.size(); /* relative to this thread's list until pass 3 */
            for (int q = 0; q < nd; q++) {
                PlanMeta &mj = mp[(size_t)deps[q]];
                if (mj.group > g) { bad = true; return; }
                __atomic_store_n(&mj.signal, (uint8_t)1, __ATOMIC_RELAXED);
                w.push_back((uint32_t)deps[q]);
            }
        }
    };
    ffhip_parallel_for(n_threads, n_threads, scan);
    if (bad) return false;
    const auto T2 = std::chrono::steady_clock::now();
    /* ---- pass 3 (sequential, light): one wait list, dependency depth per group ---- */
    merge_waits(n_tus, waits, mp, gcount.size(), gdepth, out);
    const auto T3 = std::chrono::steady_clock::now();
    order_and_emit(tus, n_tus, win_log2, bw, jt_boff, contiguous && !FFHIP_ENV("FFHIP_HEVC_INTRA_DECODE_ORDER"), mp, gcount, gfirst, gdepth, n_threads, out);
    if (FFHIP_ENV("FFHIP_PLAN_TIMES")) {
        const auto T4 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
        fprintf(stderr, "plan: setup+pass1 %ld us, pass2 %ld us, pass3 %ld us, order+emit %ld us (threads %d)\n", us(T0, T1), us(T1, T2), us(T2, T3), us(T3, T4), n_threads);
    }
    return true;
}

/* Host-side passes over a TU list (validation, the contiguity test) are ~2-4 ns per TU and thread: 7 ms for the 1.8 million TUs of
 * eight 8K grids, more than the device needs for them.  Lists of 2^17 TUs and more are cut into pieces for up to 16 threads
 * (started per call: ~20 us each, they work while the others start). */
void host_parallel_for(long long n, const std::function<void(long long, long long)> &fn)
{
    const long long min_piece = 1 << 16;
    unsigned hw = std::thread::hardware_concurrency();
    long long nt = n / min_piece;
    nt = nt > 16 ? 16 : nt;
    nt = hw && nt > (long long)hw ? (long long)hw : nt;
    if (nt < 2) { fn(0, n); return; }
    const long long piece = (n + nt - 1) / nt;
    ffhip_parallel_for((int)nt, (int)nt, [&](int k) { fn(k * piece, std::min(n, (k + 1) * piece)); });
}

/* Are the groups of this window -- the TUs whose top-left corner falls into one window tile of one plane -- contiguous
 * runs of the list?  (Then a group is complete before a later one starts, the condition of the grouped kernel.)  Two rules in one
 * pass, a byte map per plane and rule; scratch kept per thread:
 *   bit 0  runs of the list AS IT IS: a TU opens a run where its window differs from that of the record in front of it
 *   bit 1  runs of every plane's OWN subsequence: ... from that of the previous record of the same plane.  This is the rule the
 *          reference's order needs: it decodes coding unit by coding unit, the unit's luma tree, then Cb, then Cr
 *          (coding/hevc.c:5013-5180 calling decode_intra_block :4665-4805), so a coding tree block with several coding units
 *          switches planes INSIDE every 64x64 area.  The planes do not read each other, so the device planner may work on the
 *          list sorted by plane (ffhip_hevc_plan_gpu.hip, k_part_*), where bit 1 is what bit 0 is here.
 * Bit 0 implies bit 1. */
/* sampled: only the records of every 64th stretch of 4096 are looked at -- every 256th from a million records on -- (large lists, whose full test runs on the device: a window that
 * is not contiguous there is refused by the planner and the list decoded by the serial kernel -- exact, slow, and only for a list whose
 * coding-tree-block size changes between the sampled stretches) */
static int groups_contiguous(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], const int win_log2[3], const bool sampled)
{
    static thread_local std::vector<uint8_t> seen[3];
    int gw[3];
    size_t cnt[3];
    for (int c = 0; c < 3; c++) {
        gw[c] = pw[c] > 0 ? ((pw[c] - 1) >> win_log2[c]) + 1 : 0;
        cnt[c] = (size_t)gw[c] * (size_t)(ph[c] > 0 ? ((ph[c] - 1) >> win_log2[c]) + 1 : 0);
        seen[c].assign(2 * cnt[c], 0); /* [0, cnt): the list as it is; [cnt, 2 cnt): the plane's own subsequence */
    }
    uint8_t *const map[3] = {seen[0].data(), seen[1].data(), seen[2].data()};
    std::atomic<bool> twice_raw{false}, twice_plane{false};
    auto window_of = [&](const ffhip_hevc_tu &t) -> long long { /* -1: an unvalidated record of a sampled list (the device pass refuses it) */
        const int c = t.cidx;
        if (c > 2 || t.x >= pw[c] || t.y >= ph[c]) return -1;
        return (long long)(t.y >> win_log2[c]) * gw[c] + (t.x >> win_log2[c]);
    };
    /* a TU opens a run where its window differs from its predecessor's: stateless per TU under the first rule, so the list is cut into
     * pieces for as many threads as pay (a window entered by two pieces is entered twice all the same: the mark is an atomic exchange);
     * under the second rule a piece -- and a sampled stretch -- first looks back for the last record of each plane in front of it */
    host_parallel_for(sampled ? 1 : n_tus, [&](long long b, long long e) { /* (a sample is one thread's work: starting sixteen costs more than the pass) */
        if (sampled) e = n_tus;
        long long last[3] = {-2, -2, -2}; /* the window of the plane's previous record; -2 = not looked up yet */
        auto look_back = [&](long long i) {
            int missing = 3;
            last[0] = last[1] = last[2] = -1;
            for (long long j = i - 1; j >= 0 && j >= i - 4096 && missing; j--) { /* (further back than any coding tree block reaches: a run that old is taken for a new one) */
                const int c = tus[j].cidx;
                if (c > 2 || last[c] != -1) continue;
                const long long w = window_of(tus[j]);
                if (w < 0) continue;
                last[c] = w; missing--;
            }
        };
        look_back(b);
        for (long long i = b; i < e && !twice_plane.load(std::memory_order_relaxed); i++) {
            if (sampled && sampled_out(i, n_tus)) { i |= 4095; if (i + 1 < e) look_back(i + 1); continue; }
            const ffhip_hevc_tu &t = tus[i];
            const long long w = window_of(t);
            if (w < 0) continue;
            const int c = t.cidx;
            if (last[c] != w) {
                last[c] = w;
                if (__atomic_exchange_n(map[c] + cnt[c] + w, (uint8_t)1, __ATOMIC_RELAXED)) twice_plane.store(true, std::memory_order_relaxed);
            }
            if (i > 0 && tus[i - 1].cidx == c && window_of(tus[i - 1]) == w) continue;
            if (!twice_raw.load(std::memory_order_relaxed) && __atomic_exchange_n(map[c] + w, (uint8_t)1, __ATOMIC_RELAXED)) twice_raw.store(true, std::memory_order_relaxed);
        }
    });
    const bool plane_ok = !twice_plane.load();
    return (plane_ok && !twice_raw.load() ? 1 : 0) | (plane_ok ? 2 : 0);
}

/* The list sorted by plane (stable), on the host: for the host planner and ffhip_hevc_intra_plan, what k_part_* do for the device planner.
 * perm[k] = the caller's index of sorted record k. */
void sort_by_plane(const ffhip_hevc_tu *tus, long long n_tus, std::vector<ffhip_hevc_tu> &sorted, std::vector<uint32_t> *perm)
{
    size_t cnt[3] = {0, 0, 0};
    for (long long i = 0; i < n_tus; i++) cnt[tus[i].cidx > 2 ? 2 : tus[i].cidx]++;
    size_t at[3] = {0, cnt[0], cnt[0] + cnt[1]};
    sorted.resize((size_t)n_tus);
    if (perm) perm->resize((size_t)n_tus);
    for (long long i = 0; i < n_tus; i++) {
        const size_t k = at[tus[i].cidx > 2 ? 2 : tus[i].cidx]++;
        sorted[k] = tus[i];
        if (perm) (*perm)[k] = (uint32_t)i;
    }
}
/* the largest luma window (from `wl` down to 8x8) under which the list's groups are contiguous runs, by the plane's own subsequence; *by_plane:
 * NOT by the list as it is, i.e. the list has to be sorted by plane for that window.  0 when there is none.  FFHIP_HEVC_BY_PLANE=0 keeps to the
 * list as it is (the rule until round 5), =1 sorts whenever the sort alone does not make the window smaller (tests: both forms on every list). */
int pick_window(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], int wl, const bool sampled, bool *by_plane)
{
    const char *bp = FFHIP_ENV("FFHIP_HEVC_BY_PLANE");
    const int force = bp ? atoi(bp) : -1;
    const int cs = chroma_shift(pw);
    wl = wl < 3 ? 3 : (wl > 6 ? 6 : wl);
    for (; wl >= 3; wl--) {
        const int win[3] = {wl, wl - cs, wl - cs};
        const int bits = groups_contiguous(tus, n_tus, pw, ph, win, sampled);
        if (force == 0 ? (bits & 1) : (bits & 2)) {
            *by_plane = force == 0 ? false : (force == 1 ? true : !(bits & 1));
            return wl;
        }
    }
    *by_plane = false;
    return 0;
}

/* the window search both entry points share: the requested (or default) luma window, halved until a
 * plan exists; chroma windows cover the same picture area */
bool plan_with_window_search(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], int wl,
                                    GroupPlan &plan, int *used_wl, const uint32_t jt_boff[3])
{
    wl = wl < 3 ? 3 : (wl > 6 ? 6 : wl);
    const int cs = chroma_shift(pw);
    for (; wl >= 3; wl--) {
        const int win[3] = {wl, wl - cs, wl - cs};
        if (plan_groups(tus, n_tus, pw, ph, win, plan, jt_boff)) {
            if (used_wl) *used_wl = wl;
            return true;
        }
    }
    return false;
}

/* Host only (no device needed): the schedule ffhip_hevc_intra_recon would build for a VALIDATED list.
 * out_ticket[i] = ticket of TU i's group, out_wait[i] = number of TUs of other groups it waits for
 * (either may be NULL); stats = {groups, luma window log2 used, wait entries, TUs that may use the LDS tile}.
 * Returns FFHIP_EINVAL when no window gives a deadlock-free ticket order (the caller would use levels). */
extern "C" int ffhip_hevc_intra_plan(const ffhip_hevc_tu *h_tus, long long n_tus, int width_y, int height_y, int width_c,
                                     int height_c, int window_log2, uint32_t *out_ticket, uint32_t *out_wait, int32_t *stats)
{
    if (!h_tus || n_tus <= 0 || width_y <= 0 || height_y <= 0) return FFHIP_EINVAL;
    const int pw[3] = {width_y, width_c, width_c}, ph[3] = {height_y, height_c, height_c};
    GroupPlan plan;
    int wl = 0;
    const uint32_t no_table[3] = {0, 0, 0};
    /* as ffhip_hevc_intra_recon does: a list that interleaves the planes inside a window is planned sorted by plane */
    std::vector<ffhip_hevc_tu> sorted;
    std::vector<uint32_t> perm;
    bool by_plane = false;
    const int want = window_log2 ? window_log2 : FFHIP_HEVC_INTRA_WINDOW_LOG2;
    (void)pick_window(h_tus, n_tus, pw, ph, want, false, &by_plane);
    if (by_plane) sort_by_plane(h_tus, n_tus, sorted, &perm);
    if (!plan_with_window_search(by_plane ? sorted.data() : h_tus, n_tus, pw, ph, want, plan, &wl, no_table)) return FFHIP_EINVAL;
    int tile_ok = 0;
    for (size_t g = 0; g < plan.groups.size(); g++)
        for (uint32_t k = 0; k < plan.groups[g].y; k++) {
            const u32x4 q = plan.sched[(size_t)(plan.groups[g].x + k) * 3 + 2];
            const uint32_t i = by_plane ? perm[q.z] : q.z;
            if (out_ticket) out_ticket[i] = (uint32_t)g;
            if (out_wait) out_wait[i] = q.y & 0xff;
            tile_ok += (q.y >> 9) & 1;
        }
    if (stats) { stats[0] = (int32_t)plan.groups.size(); stats[1] = wl; stats[2] = (int32_t)plan.wait.size(); stats[3] = tile_ok; }
    return FFHIP_OK;
}

/* The levels form: wavefront levels at 4x4-block granularity, per plane -- a TU's level is 1 + the highest level among the blocks its
 * available neighbours lie in.  Per level the indices of its TUs, in list order. */
std::vector<std::vector<uint32_t>> intra_levels(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], const bool chroma)
{
    std::vector<std::vector<uint32_t>> lists;
    std::vector<int> lvl[3];
    int bw[3];
    for (int k = 0; k < 3; k++) {
        bw[k] = (pw[k] + 3) / 4;
        lvl[k].assign((size_t)(k == 0 || chroma ? bw[k] * ((ph[k] + 3) / 4) : 0), -1);
    }
    for (long long i = 0; i < n_tus; i++) {
        const ffhip_hevc_tu &t = tus[i];
        const int k = t.cidx, n = 1 << t.log2_size;
        int lv = 0;
        auto dep = [&](int px, int py) { lv = std::max(lv, lvl[k][(size_t)(py / 4) * bw[k] + px / 4] + 1); };
        if (t.flags & 1) dep(t.x - 1, t.y - 1);
        for (int j = 0; j < 2 * n; j++) {
            if ((t.avail_top >> j) & 1) dep(t.x + j, t.y - 1);
            if ((t.avail_left >> j) & 1) dep(t.x - 1, t.y + j);
        }
        for (int by = t.y / 4; by < (t.y + n) / 4; by++)
            for (int bx = t.x / 4; bx < (t.x + n) / 4; bx++) lvl[k][(size_t)by * bw[k] + bx] = lv;
        if ((size_t)lv >= lists.size()) lists.resize((size_t)lv + 1);
        lists[(size_t)lv].push_back((uint32_t)i);
    }
    return lists;
}
