/*
 * ffhip_state.hip -- what libffpic_hip.so keeps between calls, in two registries with one lock:
 *   per (device, stream): device scratch and pinned staging per kind, the VP8 retry record, the HEVC tile guard;
 *   per (thread, device): the side stream and the other streams and events of the calls that fork work off the caller's stream, the two
 *   slot streams of the JPEG file pipeline (their buffers are entries of the first registry, like any stream's),
 *   and per thread the Huffman decoder's header records.
 * One path (ffhip_state_release) empties both; one test hook (ffhip_debug_scratch_fill) overwrites what they hold.
 */
#include "ffhip_internal.h"
#include "ffhip_entropy_internal.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <utility>

std::mutex g_ffhip_state_mu;

/* ---- per (device, stream) ---- */
namespace {
std::map<std::pair<int, void *>, FfhipStreamState> g_streams;

/* `b` grown to hold `n` units (and some headroom: lists of nearly equal size do not reallocate).  Growing waits for the stream first: the
 * old buffer may still be read by what that stream has queued.  Everything a call enqueues is ordered on its stream, so the same stream
 * may reuse its buffer call after call without waiting, and calls on different streams (or threads) never share one. */
void *grow(FfhipBuf &b, size_t n, size_t unit, size_t pad, bool pinned, void *stream)
{
    if (n <= b.cap) return b.p;
    if (b.p) {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return nullptr;
        (void)(pinned ? hipHostFree(b.p) : hipFree(b.p));
    }
    b = FfhipBuf();
    const size_t want = n + n / 4 + pad;
    if ((pinned ? hipHostMalloc(&b.p, want * unit, hipHostMallocDefault) : hipMalloc(&b.p, want * unit)) != hipSuccess) { b.p = nullptr; return nullptr; }
    b.cap = want;
    return b.p;
}
void release(FfhipStreamState &s)
{
    for (auto &e : s.scratch) (void)hipFree(e.second.p);
    for (auto &e : s.pinned) (void)hipHostFree(e.second.p);
    for (auto &e : s.staged) (void)hipEventDestroy(e.second);
    if (s.retry.err) (void)hipHostFree(s.retry.err);
    for (hipEvent_t e : s.tiles.ev)
        if (e) (void)hipEventDestroy(e);
}
/* With g_ffhip_state_mu held and nothing of `s` in flight: every entry of the handle `s` goes, whatever device was current when it was made,
 * so that a stream made next with the same handle starts from nothing.  An abort a side-by-side VP8 call of `s` reported, and nobody
 * collected, goes to the process-wide word: not lost. */
void forget_stream(void *s)
{
    for (auto it = g_streams.begin(); it != g_streams.end();) {
        if (it->first.second != s) { ++it; continue; }
        const int *err = it->second.retry.err;
        if (err && *(volatile const int *)err) {
            int *g = ffhip_async_err_word();
            if (g) *(volatile int *)g = *(volatile const int *)err;
        }
        release(it->second);
        it = g_streams.erase(it);
    }
}
} // namespace

FfhipStreamState *ffhip_stream_state(void *stream, bool make)
{
    int dev = -1;
    (void)hipGetDevice(&dev);
    const auto key = std::make_pair(dev, stream);
    if (make) return &g_streams[key];
    auto it = g_streams.find(key);
    return it == g_streams.end() ? nullptr : &it->second;
}

extern "C" uint32_t *ffhip_scratch(int kind, void *stream, size_t words)
{
    std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
    return (uint32_t *)grow(ffhip_stream_state(stream)->scratch[kind], words, sizeof(uint32_t), 1024, false, stream);
}
/* The caller must not refill its staging before what it enqueued from it on that stream has run (a stream sync, as a rule). */
extern "C" uint8_t *ffhip_pinned_scratch(int kind, void *stream, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
    return (uint8_t *)grow(ffhip_stream_state(stream)->pinned[kind], bytes, 1, 4096, true, stream);
}

extern "C" uint8_t *ffhip_pinned_staging(int kind, void *stream, size_t bytes)
{
    hipEvent_t ev = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        auto &m = ffhip_stream_state(stream)->staged;
        auto it = m.find(kind);
        if (it != m.end()) ev = it->second;
    }
    if (ev && hipEventSynchronize(ev) != hipSuccess) return nullptr; /* (outside the lock: other streams' calls go on meanwhile) */
    return ffhip_pinned_scratch(kind, stream, bytes);
}
extern "C" int ffhip_pinned_staged(int kind, void *stream)
{
    std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
    hipEvent_t &ev = ffhip_stream_state(stream)->staged[kind];
    if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; return FFHIP_EIO; }
    return hipEventRecord(ev, (hipStream_t)stream) == hipSuccess ? FFHIP_OK : FFHIP_EIO;
}

/* Waits for what `s` holds, then frees its entries with the stream (forget_stream) */
extern "C" void ffhip_stream_destroy(void *s)
{
    if (!s) return;
    (void)hipStreamSynchronize((hipStream_t)s);
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        forget_stream(s);
    }
    (void)hipStreamDestroy((hipStream_t)s);
}

/* ---- per (thread, device) ---- */
namespace {
/* streams and events made together: all or none (nothing half-made is kept, the next call tries again from nothing) */
template <int NS, int NE> struct Group {
    hipStream_t s[NS] = {};
    hipEvent_t ev[NE] = {};
    void release()
    {
        for (auto &x : s) { if (x) (void)hipStreamDestroy(x); x = nullptr; }
        for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
    /* top: the highest stream priority the device has (FFHIP_SIDE_PRIORITY=0: the default one); events from `timed` on can time */
    bool make(bool top, int timed = NE)
    {
        if (s[0]) return true;
        int least = 0, greatest = 0;
        const char *pe = FFHIP_ENV("FFHIP_SIDE_PRIORITY");
        top = top && !(pe && atoi(pe) == 0);
        if (top && hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); greatest = 0; }
        bool ok = true;
        for (auto &x : s)
            ok = ok && (top ? hipStreamCreateWithPriority(&x, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&x, hipStreamNonBlocking)) == hipSuccess;
        for (int k = 0; k < NE; k++) ok = ok && hipEventCreateWithFlags(&ev[k], k < timed ? hipEventDisableTiming : hipEventDefault) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); release(); }
        return ok;
    }
};
struct ThreadSet {
    /* the side stream with fork, join, mid: what runs there is the SHORT chain next to a large kernel of the caller's stream (the HEVC planner's
     * ticket kernels next to the per-pixel programs: a few workgroups each, which otherwise queue behind thousands), or, in the VP8 side-by-side
     * call, a kernel whose share of the residency is its own -- hence the top priority */
    Group<1, 3> side;
    Group<1, 1> pipe;                    /* plan; plan_done */
    Group<2, FFHIP_HUFF_PARTS + 4> huff; /* up, c2; the last two events time */
    Group<2, 0> slots;                   /* the JPEG file pipeline's (ffhip_pipeline.hip): a chunk in flight on each */
    /* with g_ffhip_state_mu held, no call of the thread in flight.  The slot streams own registry entries: those go with them */
    void release()
    {
        for (hipStream_t s : slots.s) {
            if (!s) continue;
            (void)hipStreamSynchronize(s);
            forget_stream(s);
        }
        side.release(); pipe.release(); huff.release(); slots.release();
    }
};
struct ThreadState;
std::vector<ThreadState *> g_threads;
struct ThreadState {
    std::map<int, ThreadSet> sets; /* by device: a thread that alternates devices keeps each one's */
    std::unique_ptr<struct jpeg_hdr[]> hdr;
    size_t hdr_cap = 0;
    ThreadState() { std::lock_guard<std::mutex> l(g_ffhip_state_mu); g_threads.push_back(this); }
    ~ThreadState()
    {
        std::lock_guard<std::mutex> l(g_ffhip_state_mu);
        g_threads.erase(std::remove(g_threads.begin(), g_threads.end(), this), g_threads.end());
        for (auto &e : sets) e.second.release();
    }
};
ThreadState &this_thread() { static thread_local ThreadState t; return t; } /* (registers itself: not with g_ffhip_state_mu held) */
/* the calling thread's group `which` for its current device, made on first use; NULL when it could not be */
template <class G> G *thread_group(G ThreadSet::*which, bool top, int timed)
{
    ThreadState &ts = this_thread();
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> l(g_ffhip_state_mu);
    G &g = ts.sets[dev].*which;
    return g.make(top, timed) ? &g : nullptr;
}
} // namespace

/* for the stages of the library that have two independent chains in one call (ffhip_vp8_predict_loopfilter, ffhip_hevc_intra_recon: the
 * substitution table next to the planner's kernels) */
extern "C" int ffhip_side_stream_get(FfhipSide *out)
{
    const auto *g = thread_group(&ThreadSet::side, true, 3);
    if (!g) return FFHIP_EIO;
    *out = {g->s[0], g->ev[0], g->ev[1], g->ev[2]};
    return FFHIP_OK;
}
extern "C" int ffhip_slot_streams_get(FfhipSlotStreams *out)
{
    const auto *g = thread_group(&ThreadSet::slots, false, 0);
    if (!g) return FFHIP_EIO;
    *out = {{g->s[0], g->s[1]}};
    return FFHIP_OK;
}
extern "C" int ffhip_pipe_streams_get(FfhipPipe *out)
{
    const auto *g = thread_group(&ThreadSet::pipe, false, 1);
    if (!g) return FFHIP_EIO;
    *out = {g->s[0], g->ev[0]};
    return FFHIP_OK;
}
extern "C" int ffhip_huff_streams_get(FfhipHuffStreams *out)
{
    const auto *g = thread_group(&ThreadSet::huff, false, FFHIP_HUFF_PARTS + 2);
    if (!g) return FFHIP_EIO;
    out->up = g->s[0]; out->c2 = g->s[1];
    for (int k = 0; k < FFHIP_HUFF_PARTS; k++) out->part_ev[k] = g->ev[k];
    out->fork = g->ev[FFHIP_HUFF_PARTS]; out->join = g->ev[FFHIP_HUFF_PARTS + 1];
    out->time_ev[0] = g->ev[FFHIP_HUFF_PARTS + 2]; out->time_ev[1] = g->ev[FFHIP_HUFF_PARTS + 3];
    return FFHIP_OK;
}

/* (not a std::vector: that would zero 20 KB a file on the calling thread before the parsing threads start -- 84 MB and 10 ms for 4 096
 * thumbnails -- and ffhip_jpeg_parse clears its record itself; kept, because 84 MB of fresh pages and their return are milliseconds) */
struct jpeg_hdr *ffhip_huff_hdr_records(size_t n)
{
    ThreadState &t = this_thread();
    std::lock_guard<std::mutex> l(g_ffhip_state_mu);
    if (n > t.hdr_cap) {
        t.hdr.reset(new (std::nothrow) struct jpeg_hdr[n + n / 4]);
        t.hdr_cap = t.hdr ? n + n / 4 : 0;
    }
    return t.hdr.get();
}

/* ---- diagnostics: the contents of what is kept, set by a test (include/ffpic_hip.h) ----
 * Scratch is (current device, stream)'s device and pinned buffers over their whole capacity, the same of the calling thread's two slot streams
 * of the current device, and the thread's header records.  State is left alone: the retry record's pinned word, the async error word, events,
 * streams, the tile guard.  Two kinds keep content a later call needs, and the host-side mark that says it is valid is dropped with it:
 * SCRATCH_VP8_RETRY, the luma column ffhip_stream_sync puts back when it repeats a side-by-side call (`armed`; a report that is still waiting
 * to be collected refuses the fill), and the device planner's verdict in the HEVC scratch that ffhip_debug_hevc_plan_result reads (the calling
 * thread's pointer to it). */
namespace {
/* waits for `stream` and for the events behind the last copies out of its pinned staging (outside the lock, as ffhip_pinned_staging waits) */
int drain_for_fill(void *stream)
{
    FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO);
    std::vector<hipEvent_t> staged;
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        if (FfhipStreamState *e = ffhip_stream_state(stream, false))
            for (auto &s : e->staged)
                if (s.second) staged.push_back(s.second);
    }
    for (hipEvent_t ev : staged) FFHIP_CHECK(hipEventSynchronize(ev), FFHIP_EIO);
    return FFHIP_OK;
}
/* with g_ffhip_state_mu held: every byte of every buffer of `e`, the device ones by memsets enqueued on `st`; bytes[0] += device bytes,
 * bytes[1] += pinned bytes, the kinds behind `seen` */
int fill_entry(FfhipStreamState &e, hipStream_t st, int value, uint64_t bytes[2], std::vector<int> &seen)
{
    for (auto &b : e.scratch) {
        if (!b.second.p) continue;
        FFHIP_CHECK(hipMemsetAsync(b.second.p, value, b.second.cap * sizeof(uint32_t), st), FFHIP_EIO);
        bytes[0] += b.second.cap * sizeof(uint32_t);
        seen.push_back(b.first);
    }
    for (auto &b : e.pinned) {
        if (!b.second.p) continue;
        memset(b.second.p, value, b.second.cap);
        bytes[1] += b.second.cap;
        seen.push_back(b.first);
    }
    return FFHIP_OK;
}
} // namespace

extern "C" int ffhip_debug_scratch_fill(void *stream, int value, uint64_t bytes[2], int *kinds, int cap)
{
    if (!bytes || cap < 0 || (cap > 0 && !kinds)) return FFHIP_EINVAL;
    bytes[0] = bytes[1] = 0;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    ThreadState &t = this_thread();
    int dev = -1;
    (void)hipGetDevice(&dev);
    void *streams[3] = {stream, nullptr, nullptr}; /* the caller's, then the thread's slot streams of this device, where they exist */
    int n_streams = 1;
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        auto set = t.sets.find(dev);
        if (set != t.sets.end())
            for (hipStream_t s : set->second.slots.s)
                if (s) streams[n_streams++] = s;
    }
    std::vector<int> seen;
    for (int k = 0; k < n_streams; k++) {
        const int rc = drain_for_fill(streams[k]);
        if (rc) return rc;
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        FfhipStreamState *e = ffhip_stream_state(streams[k], false);
        if (!e) continue;
        if (k == 0) {
            if (e->retry.armed && e->retry.err && *(volatile int *)e->retry.err) return FFHIP_EIO; /* ffhip_stream_sync first: the repeat needs the column */
            e->retry.armed = false;
            ffhip_hevc_plan_result_forget(stream);
        }
        const int frc = fill_entry(*e, (hipStream_t)streams[k], value, bytes, seen);
        if (frc) return frc;
    }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    int count = 0;
    for (int k : seen) {
        if (count < cap) kinds[count] = k;
        count++;
    }
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        if (t.hdr) {
            memset((void *)t.hdr.get(), value, t.hdr_cap * sizeof(struct jpeg_hdr));
            bytes[1] += t.hdr_cap * sizeof(struct jpeg_hdr);
        }
    }
    for (int k = n_streams - 1; k >= 0; k--) FFHIP_CHECK(hipStreamSynchronize((hipStream_t)streams[k]), FFHIP_EIO);
    return count;
}

/* No call of ANY thread may be in flight, host part included: every thread's streams, events and header records go too. */
void ffhip_state_release(void)
{
    std::lock_guard<std::mutex> l(g_ffhip_state_mu);
    for (ThreadState *t : g_threads) {
        for (auto &e : t->sets) e.second.release();
        t->sets.clear();
        t->hdr.reset();
        t->hdr_cap = 0;
    }
    for (auto &e : g_streams) release(e.second);
    g_streams.clear();
}
