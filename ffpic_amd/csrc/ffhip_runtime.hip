/*
 * ffhip_runtime.hip -- device binding, memory/stream/event helpers and the copy
 * calibration kernel of libffpic_hip.so.  Plain plumbing around the HIP runtime
 * so that a C11 host (the reference is C) needs no HIP headers.
 */
#include "ffhip_internal.h"

#include <stdio.h>
#include <string.h>

#include <stdarg.h>

#include <mutex>

/* Process-wide, under g_init_mu: the bound device and its name are written by ffhip_init (any thread's first compute call gets there through
 * ffhip_have_device), the text of the last error by whichever thread failed last.  g_ready is read without the lock (an atomic load): it is
 * set last, when the name is whole.  ffhip_strerror hands out g_last_error itself: a text another thread may be replacing. */
static std::mutex g_init_mu;
static int g_device = -1;
static int g_ready = 0;
static char g_arch[64] = "";
static char g_last_error[256] = "";
static void set_last_error(const char *fmt, ...)
{
    std::lock_guard<std::mutex> lock(g_init_mu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}

/* FFHIP_* switches: read once per call site and process, re-read after ffhip_reload_env() */
#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
static std::atomic<int> g_env_gen{0};
static std::mutex g_env_mu;
static std::set<std::string> g_env_values; /* interned: element addresses of a std::set never move, nothing is ever erased */
extern "C" const char *ffhip_env_lookup(struct ffhip_env_site *site)
{
    const int gen = g_env_gen.load(std::memory_order_acquire);
    if (__atomic_load_n(&site->gen, __ATOMIC_ACQUIRE) != gen) {
        std::lock_guard<std::mutex> lock(g_env_mu);
        const char *v = getenv(site->name);
        const char *kept = v ? g_env_values.insert(std::string(v)).first->c_str() : nullptr;
        __atomic_store_n(&site->val, kept, __ATOMIC_RELAXED);
        __atomic_store_n(&site->gen, gen, __ATOMIC_RELEASE);
    }
    return __atomic_load_n(&site->val, __ATOMIC_RELAXED);
}
extern "C" void ffhip_reload_env(void) { g_env_gen.fetch_add(1, std::memory_order_acq_rel); }
/* test hook (tests/test_capi.py; needs no device): the value the library holds for switch `name`, by the same lookup a call
 * site makes (a site per name, kept for the process); copies it into dst[0..cap) and returns its full length, or -1 when unset */
extern "C" long ffhip_env_value_test(const char *name, char *dst, size_t cap)
{
    static std::mutex mu;
    static std::map<std::string, ffhip_env_site *> sites;
    if (!name) return -1;
    ffhip_env_site *site;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = sites.find(name);
        if (it == sites.end()) {
            auto ins = sites.emplace(std::string(name), nullptr);
            ins.first->second = new ffhip_env_site{ins.first->first.c_str(), -1, nullptr};
            it = ins.first;
        }
        site = it->second;
    }
    const char *v = ffhip_env_lookup(site);
    if (!v) return -1;
    const size_t n = strlen(v);
    if (dst && cap) { strncpy(dst, v, cap - 1); dst[cap - 1] = 0; }
    return (long)n;
}

extern "C" void ffhip_note_hip_error(int hip_error, const char *what)
{
    set_last_error("%s: %s", what, hipGetErrorString((hipError_t)hip_error));
    if (FFHIP_ENV("FFHIP_VERBOSE")) fprintf(stderr, "ffpic_hip: %s: %s\n", what, hipGetErrorString((hipError_t)hip_error));
}

/* How many single-wave workgroups of `kernel` the device holds at once: what a kernel whose waves WAIT for each other
 * (tickets + progress counters) may launch without a wave holding a ticket it cannot run yet -- and, for two such
 * kernels side by side, what lets both be resident whatever the hardware starts first. */
static std::map<std::tuple<int, const void *, int>, int> g_resident; /* keyed by device too: CU counts differ between parts */
extern "C" int ffhip_resident_waves(const void *kernel, int block_threads)
{
    std::lock_guard<std::mutex> lock(g_env_mu);
    int per_cu = 0, cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
    const auto key = std::make_tuple(dev, kernel, block_threads);
    auto it = g_resident.find(key);
    if (it != g_resident.end()) return it->second;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, 0) != hipSuccess || per_cu < 1 || cus < 1) {
        (void)hipGetLastError();
        return 256; /* one wave per CU of the smallest part: always resident */
    }
    const int n = per_cu * cus;
    g_resident[key] = n;
    return n;
}

extern "C" int ffhip_have_device(void)
{
    if (__atomic_load_n(&g_ready, __ATOMIC_ACQUIRE)) return 1;
    int dev;
    {
        std::lock_guard<std::mutex> lock(g_init_mu);
        dev = g_device < 0 ? 0 : g_device;
    }
    ffhip_init(dev);
    return __atomic_load_n(&g_ready, __ATOMIC_ACQUIRE);
}

extern "C" int ffhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int ffhip_init(int device)
{
    int n = ffhip_device_count();
    if (device < 0 || device >= n) return FFHIP_ENODEV;
    FFHIP_CHECK(hipSetDevice(device), FFHIP_ENODEV);
    hipDeviceProp_t prop;
    FFHIP_CHECK(hipGetDeviceProperties(&prop, device), FFHIP_ENODEV);
    char arch[sizeof g_arch] = "";
    strncpy(arch, prop.gcnArchName, sizeof arch - 1);
    char *colon = strchr(arch, ':');
    if (colon) *colon = 0;
    /* the code object only holds gfx950 ISA: refuse anything else up front */
    if (strcmp(arch, "gfx950") != 0) {
        set_last_error("device %d is %s, this library is built for gfx950 only", device, arch);
        return FFHIP_ENODEV;
    }
    std::lock_guard<std::mutex> lock(g_init_mu);
    memcpy(g_arch, arch, sizeof g_arch); /* (whole before g_ready says so: another thread's first call may be reading it) */
    g_device = device;
    __atomic_store_n(&g_ready, 1, __ATOMIC_RELEASE);
    return FFHIP_OK;
}

/* Nothing of the library's may be in flight.  Frees what the library keeps between calls (ffhip_state.hip); the next compute call binds
 * the device again. */
extern "C" void ffhip_shutdown(void)
{
    if (__atomic_load_n(&g_ready, __ATOMIC_ACQUIRE)) {
        (void)hipDeviceSynchronize();
        ffhip_release_caches();
    }
    __atomic_store_n(&g_ready, 0, __ATOMIC_RELEASE);
}

/* One pinned, device-visible word that a kernel with an in-launch dependency wait writes when it
 * gives up (its bounded spin ran out); checked and cleared by ffhip_stream_sync. */
/* Process-wide.  g_async_mu owns its making and its freeing: two first calls at once make ONE word (with two, a kernel would report into one
 * and the sync read the other).  It is read without the lock, by atomic loads: once made it stays until ffhip_release_caches, which needs
 * every thread quiet. */
static std::mutex g_async_mu;
static int *g_async_err = nullptr;
static int *async_err_peek(void) { return __atomic_load_n(&g_async_err, __ATOMIC_ACQUIRE); }
extern "C" int *ffhip_async_err_word(void)
{
    int *w = async_err_peek();
    if (w) return w;
    if (!ffhip_have_device()) return nullptr;
    std::lock_guard<std::mutex> lock(g_async_mu);
    w = g_async_err;
    if (!w) {
        if (hipHostMalloc((void **)&w, 64, hipHostMallocMapped) != hipSuccess) return nullptr;
        *w = 0;
        __atomic_store_n(&g_async_err, w, __ATOMIC_RELEASE);
    }
    return w;
}

extern "C" const char *ffhip_arch_name(void) { return g_arch; }

extern "C" void ffhip_release_caches(void)
{
    ffhip_state_release();
    std::lock_guard<std::mutex> lock(g_async_mu);
    if (g_async_err) {
        int *w = g_async_err;
        __atomic_store_n(&g_async_err, (int *)nullptr, __ATOMIC_RELEASE);
        (void)hipHostFree(w);
    }
}

extern "C" const char *ffhip_strerror(int code)
{
    switch (code) {
    case FFHIP_OK: return "ok";
    case FFHIP_RETRIED: return "a side-by-side VP8 call was repeated by the sync: its outputs are good, what was enqueued behind it is stale";
    case FFHIP_EINVAL: return "invalid argument or unsupported geometry";
    case FFHIP_ENOMEM: return "out of memory";
    case FFHIP_ENODEV: return g_last_error[0] ? g_last_error : "no usable gfx950 device";
    case FFHIP_EIO: return g_last_error[0] ? g_last_error : "HIP launch or copy failed";
    case FFHIP_EWEBP_LOSSLESS: return "lossless WebP (VP8L) is not decoded by this call (the ffhip_vp8l_* calls decode it)";
    case FFHIP_EWEBP_ANIMATION: return "animated WebP is not decoded";
    case FFHIP_EWEBP_INTER_FRAME: return "the VP8 frame is not a key frame";
    case FFHIP_EJPEG_NOSPACE: return "the JPEG file does not fit the output's cap (the length is the size it needs)";
    case FFHIP_EJPEG_RANGE: return "a coefficient Annex K's Huffman tables cannot code (AC magnitude over 1023 or DC difference beyond +-2047)";
    case FFHIP_EVP8L_NOSPACE: return "the lossless WebP file does not fit the output's cap (the length is the size it needs)";
    case FFHIP_EVP8_NOSPACE: return "the lossy WebP file does not fit the output's cap (the length is the size it needs)";
    case FFHIP_EVP8_PARTITION: return "a partition of the lossy WebP file is longer than a VP8 frame can say";
    case FFHIP_EPNG_NOSPACE: return "the PNG file does not fit the output's cap (the length is the size it needs)";
    case FFHIP_EDEFLATE_NOSPACE: return "the zlib stream does not fit the output's cap (the length is the size it needs)";
    default: return "unknown error";
    }
}

extern "C" void *ffhip_malloc(size_t bytes)
{
    void *p = nullptr;
    if (!ffhip_have_device()) return nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    return p;
}
extern "C" void ffhip_free(void *p) { if (p) (void)hipFree(p); }

extern "C" int ffhip_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream)
{
    FFHIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), FFHIP_EIO);
    return FFHIP_OK;
}
extern "C" int ffhip_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream)
{
    FFHIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream), FFHIP_EIO);
    return FFHIP_OK;
}
extern "C" int ffhip_memset(void *dst, int value, size_t bytes, void *stream)
{
    FFHIP_CHECK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream), FFHIP_EIO);
    return FFHIP_OK;
}
extern "C" void *ffhip_stream_create(void)
{
    hipStream_t s = nullptr;
    if (!ffhip_have_device()) return nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return (void *)s;
}
extern "C" int ffhip_stream_sync(void *s)
{
    FFHIP_CHECK(hipStreamSynchronize((hipStream_t)s), FFHIP_EIO);
    /* A bounded wait of a side-by-side VP8 call of THIS stream ran out (reported in a pinned word of that call's own: possible on a device
     * shared with other work, where one of its two kernels may not become resident next to the other).  Its inputs are intact and the one thing
     * of the planes' former contents it reads is kept (the last luma column), so the library repeats the stages ONE AFTER THE OTHER here and
     * says so: FFHIP_RETRIED, not FFHIP_OK -- what the caller had enqueued behind the call has consumed the aborted run's planes. */
    const int retried = ffhip_vp8_side_by_side_retry(s);
    int *const word = async_err_peek();
    if (retried < 0) {
        set_last_error("a side-by-side VP8 call aborted and could not be repeated");
        if (word) __atomic_store_n(word, 0, __ATOMIC_RELAXED);
        return FFHIP_EIO;
    }
    /* (taken with an exchange: the word is process-wide, and of two threads that sync at once ONE collects a give-up) */
    if (const int code = word ? __atomic_exchange_n(word, 0, __ATOMIC_ACQ_REL) : 0) {
        set_last_error(code == FFHIP_ASYNC_BAD_INPUT ? "a dependency-scheduled kernel refused its input (code %d)"
                                                     : "a dependency-scheduled kernel aborted (code %d)", code);
        return code == FFHIP_ASYNC_BAD_INPUT ? FFHIP_EINVAL : FFHIP_EIO;
    }
    {
        std::lock_guard<std::mutex> lock(g_ffhip_state_mu);
        if (FfhipStreamState *e = ffhip_stream_state(s, false)) e->retry.armed = false; /* clean: whatever was enqueued there has run */
    }
    return retried;
}
extern "C" void *ffhip_event_create(void)
{
    hipEvent_t e = nullptr;
    if (!ffhip_have_device()) return nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return (void *)e;
}
extern "C" void ffhip_event_destroy(void *e) { if (e) (void)hipEventDestroy((hipEvent_t)e); }
extern "C" int ffhip_event_record(void *e, void *s)
{
    FFHIP_CHECK(hipEventRecord((hipEvent_t)e, (hipStream_t)s), FFHIP_EIO);
    return FFHIP_OK;
}
extern "C" float ffhip_event_elapsed_ms(void *start, void *stop)
{
    float ms = -1.0f;
    if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess) return -1.0f;
    return ms;
}

/* 16 B per lane non-temporal copy, one element per thread (no loop): the launch shape and
 * cache policy that stream fastest on MI355X (tests/tools/membench.hip).  The achievable-HBM yardstick the fused
 * kernel is compared with in the same process (bench.py). */
__global__ __launch_bounds__(256) void k_copy_calibrate(u32x4 *dst, const u32x4 *src, size_t n16)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]), &dst[i]);
}

extern "C" int ffhip_copy_calibrate(void *d_dst, const void *d_src, size_t bytes, void *stream)
{
    if (!d_dst || !d_src || (bytes & 15) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_src & 15)) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    size_t n16 = bytes / 16;
    if (!n16) return FFHIP_OK;
    if (n16 > (size_t)0x7fffffff * 256) return FFHIP_EINVAL;
    hipLaunchKernelGGL(k_copy_calibrate, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (u32x4 *)d_dst, (const u32x4 *)d_src, n16);
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return FFHIP_OK;
}
