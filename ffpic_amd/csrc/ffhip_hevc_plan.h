/* ffhip_hevc_plan.h -- what the HEVC intra files share and nobody else reads: ffhip_hevc_intra.hip (kernels, the call), ffhip_hevc_plan_host.hip
 * (the host planner) and ffhip_hevc_plan_gpu.hip (the device planner). */
#ifndef FFHIP_HEVC_PLAN_H
#define FFHIP_HEVC_PLAN_H

#include "ffhip_internal.h"

#include <functional>

/* bits of a schedule slot's program word (second quarter, .x) that two files know: k_hevc_intra_program writes the word, k_plan_emit adds
 * what only the planner knows when the programs were built NEXT TO it (ffhip_hevc_intra.hip has the rest of the layout) */
#define FFHIP_PK_KIND_MASK 7u
#define FFHIP_PK_SIGNAL 64u
#define FFHIP_PK_WAIT 128u
#define FFHIP_PK_SLOW 256u
#define FFHIP_PROG_NO_RESIDUAL 0xffffff00u

#define JT_STRIDE 20 /* substitution table bytes per 4x4 block: a TU of size n owns n/4 consecutive blocks of its first block row, 5n >= 4n + 1 bytes */
#ifndef FFHIP_HEVC_INTRA_WINDOW_LOG2
#define FFHIP_HEVC_INTRA_WINDOW_LOG2 5 /* luma window of the host-planned grouped form: 32x32 (1080p sweep in profiles/r1_stages.json) */
#endif

/* log2 of the chroma planes' subsampling against luma, horizontally (4:2:0 / 4:2:2: 1) */
inline int chroma_shift(const int pw[3]) { return (pw[1] > 0 && pw[1] * 2 <= pw[0] + 1) ? 1 : 0; }

/* A sampled pass over a large list only looks at the records of every 64th stretch of 4096 -- every 256th from a million records on: is
 * record i left out?  (The full pass over such a list runs on the device, k_hevc_check_tus and the planner.) */
inline bool sampled_out(const long long i, const long long n_tus) { return ((i >> 12) & (n_tus >= (1LL << 20) ? 255 : 63)) != 0; }

/* THE record check, of the host's validation and of k_hevc_check_tus: field ranges, the block inside its plane (pw x ph samples per plane), no
 * availability bit pointing outside the plane; chroma_ok: the chroma planes are there and wide enough.  Whether a record may ask for a
 * residual is the callers' business.  The first two returns keep pw[c] with c > 2 and shifts by a size out of range from being evaluated;
 * the picture-edge test is bitwise on purpose (straight-line code in the kernel). */
__host__ __device__ inline bool hevc_tu_valid(const ffhip_hevc_tu &t, const int pw[3], const int ph[3], const bool chroma_ok)
{
    const int c = t.cidx;
    if (c > 2 || t.log2_size < 2 || t.log2_size > 5 || t.pred_mode > 34) return false;
    const int n = 1 << t.log2_size;
    if (t.x + n > pw[c] || t.y + n > ph[c]) return false;
    const unsigned long long span = n == 32 ? ~0ull : (1ull << (2 * n)) - 1;
    const unsigned long long top = t.avail_top & span, left = t.avail_left & span;
    const int room_x = pw[c] - t.x, room_y = ph[c] - t.y; /* samples that exist right of x0 / below y0 */
    const bool corner = (t.flags & 1) != 0;
    if (((top != 0 || corner) & (t.y == 0)) | ((left != 0 || corner) & (t.x == 0))) return false;
    if ((room_x < 64 && (top >> room_x)) || (room_y < 64 && (left >> room_y))) return false;
    return c == 0 || chroma_ok;
}

/* The device planner (ffhip_hevc_plan_gpu.hip): its kernels' argument, where its scratch is (plan_layout) ... */
struct PlanArgs {
    const ffhip_hevc_tu *tus;
    uint32_t n;
    int pw[3], ph[3], bw[3], gw[3], wl[3];
    uint32_t owner_off[3], win_off[3]; /* per plane: start inside owner[] / win_run[] */
    int32_t *owner;        /* TU index per 4x4 block, -1 = none                     */
    uint32_t *win_run;     /* run that claimed a window, ~0 = none                  */
    uint32_t *start;       /* 1 where a run starts; after the scan: runs before me  */
    uint32_t *runid;       /* inclusive scan of start, minus one                    */
    uint32_t *wcount;      /* wait entries per TU; after the scan: first entry      */
    uint32_t *wbegin;
    uint8_t *flags;        /* bit 0 signal, bit 1 tile_ok                           */
    uint32_t *gstart;      /* TU index where run r starts; [n_runs] = n             */
    uint32_t *wait_idx;
    u32x4 *sched, *groups;
    uint32_t *result;      /* [0] fail, [1] number of runs, [2] wait entries, [3] no wavefront keys, [4] the widest wavefront:
                              the largest number of runs that share a dependency depth, [5] log2 of the luma window, [6] a record failed
                              k_hevc_check_tus, [7] the list was sorted by plane (k_part_*) */
    uint32_t wait_cap;     /* words reserved for wait_idx                           */
    uint32_t wsub_n;       /* slices in use: a power of two, at most PLAN_WSUB, never more than blocks of 256 TUs */
    uint32_t *wsub;        /* PLAN_WSUB counters, one per 128-byte line: wait entries handed out of slice r of wait_idx */
    uint32_t *cell_claim;  /* per 64x64-luma cell and plane: TU that opened it, ~0 = none (is the CTB 64?) */
    uint32_t *cell_edges;  /* bit 0 left, 1 above, 2 above-left, 3 above-right: cells this cell's TUs read */
    uint32_t *cell_depth;  /* longest chain of such edges ending here: the wavefront index of the cell     */
    uint32_t n_cells, cgh[3];
    uint32_t cell_off[3], cgw[3];
    int cshift[3];         /* log2 of the cell size in samples of the plane          */
    uint32_t *rank_of;     /* ticket of a run                                          */
    uint32_t *blk_tot;     /* per block of 256 TUs: run starts                                        */
    uint32_t *blk_pre;     /* its exclusive scan: starts in the blocks before                         */
    uint32_t *cell_nruns;  /* runs per cell                                            */
    uint32_t *cell_base;   /* first ticket of the cell's runs                          */
    uint32_t *hist;        /* [depths][shards] runs per (depth, shard)                 */
    uint32_t *hist_pre;    /* its exclusive scan: first ticket of the pair             */
    uint32_t *fill;        /* [depths][shards] tickets of the pair handed out so far   */
    uint32_t depths;       /* a bound on the depths: a chain ending at cell (x, y) has at most x + 2y edges */
    float stripe_scale[3]; /* 2^shard_log2 / cells of the plane */
    uint32_t shard_log2;   /* the counters of one depth are spread over 2^shard_log2 words, picked by the cell's block: a grid of tiles has
                              two dozen distinct depths for its 200 000 cells, and that many atomic adds on two dozen words took 0.4 ms */
    /* the list sorted by plane (k_part_*): the caller's records, the copy the planner and everything behind it work on, and per
     * (plane, block of 256 records) the records of that plane in the block / in front of it in the sorted list */
    const ffhip_hevc_tu *raw;
    ffhip_hevc_tu *sorted;
    uint32_t *part_tot, *part_pre;
    uint32_t part_nb;
};
struct PlanLayout {
    size_t words, blocks, wins, cells, n_blocks, wait_cap;
    uint32_t *zero_cells; /* cell_edges | cell_nruns | hist | fill, adjacent: cleared together */
    size_t zero_cells_words;
};
/* ... and the stages ffhip_hevc_intra_recon enqueues one after the other, with its own work between them (the substitution table, the
 * per-pixel programs, the forks and joins of its side stream).  Everything goes to `st`, the stream given to begin(), but the stages that
 * take a stream.  The schedule is only ENQUEUED: the grouped kernel reads the planner's verdict (a.result) for itself. */
struct FfhipHevcPlan {
    PlanArgs a; /* behind begin(): a.sched, a.groups, a.wait_idx, a.result, a.wait_cap (the outputs); behind count(): a.flags, a.wcount are final */
    PlanLayout L;
    hipStream_t st;
    /* k_plan_init, which also clears `also_zero` (the grouped kernel's ticket counter and done flags), then -- check = {chroma_ok,
     * have_residual} -- the list's validation, k_hevc_check_tus: refused() is set for a bad record */
    void begin(const ffhip_hevc_tu *d_tus, long long n_tus, const int pw[3], const int ph[3], const int wl[3], uint32_t *scratch, hipStream_t stream,
               uint32_t *also_zero, size_t also_zero_words, const int *check, int *async_err);
    const uint32_t *refused() const { return a.result + 6; }
    /* k_part_*: a stable partition of the list by plane (for a list that interleaves the planes inside a scheduling window, the reference's
     * own order, coding/hevc.c:5013-5180); from here on a.tus is that copy, in the planner's scratch: the records the schedule refers to */
    void partition();
    void owner() const;                /* k_plan_owner */
    void sweep(hipStream_t s) const;   /* the depth sweep of the cells, behind owner() */
    void count() const;                /* k_plan_scan, k_plan_runid, k_plan_count */
    void tickets(hipStream_t s) const; /* k_plan_cell_hist, k_plan_scan, k_plan_cell_base, k_plan_rank, k_plan_emit: behind sweep() and count() */
};
/* 32-bit words of the scratch FfhipHevcPlan::begin lays out */
size_t ffhip_hevc_plan_gpu_words(long long n_tus, const int pw[3], const int ph[3], const int wl[3]);

/* ---- the host planner (ffhip_hevc_plan_host.hip): plain C++, no device needed ---- */
struct GroupPlan {
    std::vector<u32x4> sched;  /* 3 per slot */
    std::vector<u32x4> groups;
    std::vector<uint32_t> wait;
};
#pragma GCC visibility push(hidden)
/* fn(begin, end) over the pieces of [0, n): one piece below 2^17, else pieces of at least 2^16 for up to 16 threads */
void host_parallel_for(long long n, const std::function<void(long long, long long)> &fn);
/* the list sorted by plane (stable); perm[k] = the caller's index of sorted record k (may be NULL) */
void sort_by_plane(const ffhip_hevc_tu *tus, long long n_tus, std::vector<ffhip_hevc_tu> &sorted, std::vector<uint32_t> *perm);
/* the largest luma window (log2, from `wl` down to 3) under which the list's groups are contiguous runs, 0 when there is none; *by_plane: only
 * once the list is sorted by plane */
int pick_window(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], int wl, bool sampled, bool *by_plane);
/* the schedule of a validated list under the largest luma window from `wl` down that gives one (*used_wl); false: none does */
bool plan_with_window_search(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], int wl, GroupPlan &plan, int *used_wl,
                             const uint32_t jt_boff[3]);
/* the levels form's schedule of a validated list: per wavefront level the indices of its TUs, in list order */
std::vector<std::vector<uint32_t>> intra_levels(const ffhip_hevc_tu *tus, long long n_tus, const int pw[3], const int ph[3], bool chroma);
#pragma GCC visibility pop

#endif
