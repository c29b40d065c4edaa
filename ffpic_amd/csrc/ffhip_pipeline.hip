/*
 * ffhip_pipeline.hip -- files in, pixels out: the JPEG front end (ffhip_entropy.c, host threads) and the
 * fused reconstruction (ffhip_jpeg.hip) as one double-buffered pipeline, the transbmp-shaped caller of
 * SURVEY 8 rows f1 + f2 (format/jpg.c:588-655 -> :540-560 -> struct pic, format/file.h:29-40).
 *
 * Pictures of one geometry are processed in chunks.  While the host threads Huffman-decode chunk k + 1
 * straight into pinned memory, chunk k is on its stream: H2D copy, one reconstruction launch, D2H copy into
 * pinned memory; finished chunks are copied out to the caller's (pageable) buffer.  Steady state is the
 * slower of "entropy decode on the host" and "PCIe", not their sum.  PCIe-inclusive by construction: this
 * is never the number bench.py reports.
 */
#include "ffhip_internal.h"
#include "ffhip_entropy_internal.h"
#include "ffhip_jpeg_scaled_body.h"
#include "ffhip_jpeg_prog_internal.h"

#include <stdlib.h>
#include <string.h>

#include <array>
#include <mutex>
#include <thread> /* copy_out */
#include <vector>

namespace {
/* two slots of pinned + device buffers and a stream each, kept between calls (pinning hundreds of MB costs
 * more than decoding them) and grown on demand; one pipeline call at a time (mutex) */
struct Slot {
    int16_t *h_y = nullptr, *h_u = nullptr, *h_v = nullptr; /* pinned */
    uint16_t *h_q = nullptr;
    uint8_t *h_out = nullptr;                               /* pinned staging, unused when the caller's buffer is pinned */
    int16_t *d_y = nullptr, *d_u = nullptr, *d_v = nullptr;
    uint16_t *d_q = nullptr;
    uint8_t *d_out = nullptr;
    hipStream_t st = nullptr;
    size_t cap_y = 0, cap_c = 0, cap_q = 0, cap_out = 0, cap_hout = 0; /* bytes */
    int first = -1, count = 0; /* pictures in flight in this slot */
};
Slot g_slot[2];
std::mutex g_pipe_mu;

bool grow_pair(void **h, void **d, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return true;
    if (*h) (void)hipHostFree(*h);
    if (*d) (void)hipFree(*d);
    *h = *d = nullptr;
    *cap = 0;
    if (hipHostMalloc(h, bytes, hipHostMallocDefault) != hipSuccess) { *h = nullptr; return false; }
    if (hipMalloc(d, bytes) != hipSuccess) { *d = nullptr; return false; }
    *cap = bytes;
    return true;
}
bool prepare(Slot &s, size_t by, size_t bc, size_t bq, size_t bout, bool need_hout)
{
    if (!s.st && hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess) return false;
    if (!grow_pair((void **)&s.h_y, (void **)&s.d_y, &s.cap_y, by)) return false;
    if (bc > s.cap_c) {
        size_t c1 = s.cap_c, c2 = s.cap_c;
        if (!grow_pair((void **)&s.h_u, (void **)&s.d_u, &c1, bc) || !grow_pair((void **)&s.h_v, (void **)&s.d_v, &c2, bc)) { s.cap_c = 0; return false; }
        s.cap_c = bc;
    }
    if (!grow_pair((void **)&s.h_q, (void **)&s.d_q, &s.cap_q, bq)) return false;
    if (bout > s.cap_out) {
        if (s.d_out) (void)hipFree(s.d_out);
        s.d_out = nullptr; s.cap_out = 0;
        if (hipMalloc((void **)&s.d_out, bout) != hipSuccess) { s.d_out = nullptr; return false; }
        s.cap_out = bout;
    }
    if (need_hout && bout > s.cap_hout) {
        if (s.h_out) (void)hipHostFree(s.h_out);
        s.h_out = nullptr; s.cap_hout = 0;
        if (hipHostMalloc((void **)&s.h_out, bout, hipHostMallocDefault) != hipSuccess) { s.h_out = nullptr; return false; }
        s.cap_hout = bout;
    }
    s.first = -1;
    s.count = 0;
    return true;
}
/* rows of `count` pictures from tight pinned staging to the caller's pageable buffer, over host threads */
void copy_out(uint8_t *bgra, int64_t pitch, int64_t image_stride, const uint8_t *src, size_t dev_pitch, int64_t height, int first,
              int count, int n_threads)
{
    const long long rows = (long long)count * height;
    auto part = [&](int t, int nt) {
        for (long long r = rows * t / nt, e = rows * (t + 1) / nt; r < e; r++) {
            const long long i = r / height, y = r % height;
            memcpy(bgra + (first + i) * image_stride + y * pitch, src + (size_t)r * dev_pitch, dev_pitch);
        }
    };
    const int nt = n_threads < 1 ? 1 : (n_threads > 16 ? 16 : n_threads);
    if (nt == 1 || rows < 64) { part(0, 1); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(part, t, nt);
    part(0, nt);
    for (auto &th : pool) th.join();
}

/* Does the entropy decode of these files go to the device?  FFHIP_JPEG_GPU_ENTROPY=0 keeps it on the host threads and =1 forces it to the device.
 * Unset, it goes there: the subsequence decoder takes files whatever their restart markers.  Only with FFHIP_JPEG_SYNC=0 -- the kernel with a lane
 * per restart interval, to which a file without markers is ONE lane, its latency per batch that of one interval -- it takes a batch whose first
 * file has markers, or a thousand files or more. */
bool jpeg_entropy_on_device(const uint8_t *file0, size_t len0, int n)
{
    const char *ge = FFHIP_ENV("FFHIP_JPEG_GPU_ENTROPY");
    if (ge && (ge[0] == '0' || ge[0] == '1')) return ge[0] == '1';
    const char *sy = FFHIP_ENV("FFHIP_JPEG_SYNC");
    return !(sy && sy[0] == '0') || ffhip_jpeg_probe_restart(file0, len0) > 0 || n >= 1024;
}

/* Y | U | V | quantiser tables of a batch in one block, device or pinned: yb and cb are the int16 elements of the luma plane and of each chroma
 * plane (cb 0: grey, no chroma planes), the n pictures' tables lie on a 16-byte boundary behind the planes */
struct Planes { int16_t *y, *u, *v; uint16_t *q; };
struct PlaneBlock {
    size_t yb, cb, q_off, bytes;
    PlaneBlock(size_t yb_, size_t cb_, size_t n) : yb(yb_), cb(cb_), q_off(((yb_ + 2 * cb_) * 2 + 15) & ~(size_t)15), bytes(q_off + n * 512) {}
    Planes at(uint8_t *base) const { int16_t *y = (int16_t *)base; return {y, cb ? y + yb : nullptr, cb ? y + yb + cb : nullptr, (uint16_t *)(base + q_off)}; }
};

/* Host threads Huffman-decode pictures [first, first + cnt) into the slot's pinned planes (yb, cb: int16 elements per picture), then four H2D
 * copies on the slot's stream.  The decoder's code goes to *result if that holds none yet: per-picture codes are in status[], bad pictures
 * still occupy their place. */
int host_decode_chunk(Slot &sl, const uint8_t *const *files, const size_t *lens, int first, int cnt, int n_threads, const ffhip_jpeg_geom &g,
                      size_t yb, size_t cb, int *status, int *result)
{
    const int erc = ffhip_jpeg_entropy_batch(files + first, lens + first, cnt, n_threads, &g, sl.h_y, cb ? sl.h_u : nullptr, cb ? sl.h_v : nullptr, sl.h_q,
                                             status + first);
    if (erc && !*result) *result = erc;
    hipError_t e = hipMemcpyAsync(sl.d_y, sl.h_y, cnt * yb * 2, hipMemcpyHostToDevice, sl.st);
    if (e == hipSuccess && cb) e = hipMemcpyAsync(sl.d_u, sl.h_u, cnt * cb * 2, hipMemcpyHostToDevice, sl.st);
    if (e == hipSuccess && cb) e = hipMemcpyAsync(sl.d_v, sl.h_v, cnt * cb * 2, hipMemcpyHostToDevice, sl.st);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.d_q, sl.h_q, (size_t)cnt * 512, hipMemcpyHostToDevice, sl.st);
    return e == hipSuccess ? FFHIP_OK : FFHIP_EIO;
}
} // namespace

void ffhip_pipeline_release(void)
{
    std::lock_guard<std::mutex> lock(g_pipe_mu);
    for (int s = 0; s < 2; s++) {
        Slot &sl = g_slot[s];
        if (sl.st) (void)hipStreamSynchronize(sl.st);
        (void)hipHostFree(sl.h_y); (void)hipHostFree(sl.h_u); (void)hipHostFree(sl.h_v); (void)hipHostFree(sl.h_q); (void)hipHostFree(sl.h_out);
        (void)hipFree(sl.d_y); (void)hipFree(sl.d_u); (void)hipFree(sl.d_v); (void)hipFree(sl.d_q); (void)hipFree(sl.d_out);
        if (sl.st) (void)hipStreamDestroy(sl.st);
        sl = Slot();
    }
}

extern "C" void *ffhip_host_malloc(size_t bytes)
{
    void *p = nullptr;
    if (!ffhip_have_device()) return nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void ffhip_host_free(void *p) { if (p) (void)hipHostFree(p); }

extern "C" int ffhip_jpeg_decode_files(const uint8_t *const *files, const size_t *lens, int n, int n_threads, int chunk,
                                       ffhip_jpeg_geom *geom_out, uint8_t *bgra, int64_t pitch, int64_t image_stride,
                                       int *status)
{
    if (n < 0 || (n > 0 && (!files || !lens || !bgra || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    ffhip_jpeg_geom g;
    int w = 0, h = 0;
    int rc = ffhip_jpeg_probe(files[0], lens[0], &g, &w, &h);
    if (rc) return rc;
    if (geom_out) *geom_out = g;
    const int64_t width = (int64_t)g.mcu_cols * 8 * g.h, height = (int64_t)g.mcu_rows * 8 * g.v;
    if (pitch < width * 4 || (pitch & 15) || (n > 1 && image_stride < pitch * height)) return FFHIP_EINVAL;
    if (g.mcu_cols <= 0 || g.mcu_rows <= 0) return FFHIP_EINVAL; /* workspace_bytes is 0 for a geometry it rejects, too */
    if (ffhip_jpeg_workspace_bytes(&g, 1) != 0) return FFHIP_EINVAL; /* one component with several blocks per MCU: not here */
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const bool gpu_entropy = jpeg_entropy_on_device(files[0], lens[0], n);
    if (chunk <= 0) {
        /* a chunk is a device call and a stream sync: 32 pictures of 4K (a gigabyte of BGRA per slot), and as many small pictures as make 256 MB of BGRA
         * -- 1 024 thumbnails of 256x256, not 32 */
        chunk = gpu_entropy ? 32 : 8;
        const int64_t px = width * height * 4;
        if (gpu_entropy && px > 0 && (256ll << 20) / px > chunk) chunk = (int)((256ll << 20) / px > 4096 ? 4096 : (256ll << 20) / px);
    }
    if (chunk > n) chunk = n;
    const size_t mcus = (size_t)g.mcu_cols * g.mcu_rows;
    const size_t yb = mcus * g.h * g.v * 64, cb = g.ncomp == 3 ? mcus * 64 : 0; /* int16 elements per picture */
    /* on the device the pictures have the pitch ffhip_bgra_layout recommends (the buffer is the library's); the pinned staging
     * for a pageable destination is tight, and every copy off the device is a 2-D copy */
    int64_t lp = 0, ls = 0;
    if (ffhip_bgra_layout(&g, &lp, &ls) != FFHIP_OK) return FFHIP_EINVAL;
    const size_t dev_pitch = (size_t)lp, out_b = (size_t)ls, row_b = (size_t)width * 4;
    /* a pinned (hipHostMalloc'ed / registered) destination takes the D2H copy directly */
    hipPointerAttribute_t attr;
    const bool pinned_dst = hipPointerGetAttributes(&attr, bgra) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned_dst) (void)hipGetLastError(); /* an unknown pointer leaves an error behind: not ours */

    std::lock_guard<std::mutex> lock(g_pipe_mu);
    Slot *slot = g_slot;
    for (int s = 0; s < 2; s++)
        if (!prepare(slot[s], chunk * yb * 2, chunk * cb * 2, (size_t)chunk * 512, chunk * out_b, !pinned_dst)) return FFHIP_ENOMEM;
    int result = FFHIP_OK;
    /* wait for a slot's chunk and hand its pixels to the caller */
    auto drain = [&](Slot &sl) -> int {
        if (sl.count == 0) return FFHIP_OK;
        if (hipStreamSynchronize(sl.st) != hipSuccess) return FFHIP_EIO;
        if (!pinned_dst) copy_out(bgra, pitch, image_stride, sl.h_out, row_b, height, sl.first, sl.count, n_threads);
        sl.count = 0;
        return FFHIP_OK;
    };
    rc = FFHIP_OK;
    int k = 0;
    for (int first = 0; first < n && rc == FFHIP_OK; first += chunk, k++) {
        Slot &sl = slot[k & 1];
        const int cnt = n - first < chunk ? n - first : chunk;
        rc = drain(sl); /* the slot's previous chunk (k - 2) */
        if (rc) break;
        hipError_t e = hipSuccess;
        /* entropy decode.  On the device, straight into the device planes (the host only parses headers and unstuffs the
         * scan bytes), unless the gate keeps the files on the host or the device call refuses them: then host threads
         * into pinned memory and H2D.  Either way chunk k - 1 is on the GPU meanwhile. */
        bool on_device = false;
        if (gpu_entropy) {
            const int grc = ffhip_jpeg_entropy_batch_gpu(files + first, lens + first, cnt, n_threads, &g, sl.d_y, cb ? sl.d_u : nullptr,
                                                         cb ? sl.d_v : nullptr, sl.d_q, status + first, sl.st);
            on_device = grc == FFHIP_OK;
            if (!on_device && grc != FFHIP_EINVAL) { rc = grc; break; }
        }
        if (!on_device) {
            rc = host_decode_chunk(sl, files, lens, first, cnt, n_threads, g, yb, cb, status, &result);
            if (rc) break;
        }
        rc = ffhip_jpeg_recon_batch(&g, cnt, sl.d_y, cb ? sl.d_u : nullptr, cb ? sl.d_v : nullptr, sl.d_q, 256, sl.d_out, (int64_t)dev_pitch,
                                    (int64_t)out_b, nullptr, 0, sl.st);
        if (rc) break;
        if (pinned_dst) {
            if (cnt == 1 || image_stride == pitch * height) /* the caller's pictures follow each other row after row: one copy for the chunk */
                e = hipMemcpy2DAsync(bgra + (int64_t)first * image_stride, (size_t)pitch, sl.d_out, dev_pitch, row_b, (size_t)height * cnt, hipMemcpyDeviceToHost, sl.st);
            else
                for (int i = 0; i < cnt && e == hipSuccess; i++)
                    e = hipMemcpy2DAsync(bgra + (int64_t)(first + i) * image_stride, (size_t)pitch, sl.d_out + (size_t)i * out_b, dev_pitch, row_b,
                                         (size_t)height, hipMemcpyDeviceToHost, sl.st);
        } else {
            e = hipMemcpy2DAsync(sl.h_out, row_b, sl.d_out, dev_pitch, row_b, (size_t)height * cnt, hipMemcpyDeviceToHost, sl.st);
        }
        if (e != hipSuccess) { rc = FFHIP_EIO; break; }
        sl.first = first;
        sl.count = cnt;
    }
    for (int s = 0; s < 2; s++) {
        const int r2 = drain(slot[(k + s) & 1]); /* oldest first */
        if (rc == FFHIP_OK) rc = r2;
    }
    return rc ? rc : result;
}

/* Files in, pixels out ON THE DEVICE: for consumers that live on the GPU (a resize, an inference pre-processing
 * stage) nothing but the compressed bytes crosses PCIe.  Coefficient planes are library scratch (kept per stream). */
extern "C" int ffhip_jpeg_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                              ffhip_jpeg_geom *geom_out, uint8_t *d_bgra, int64_t pitch, int64_t image_stride,
                                              int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    ffhip_jpeg_geom g;
    int w = 0, h = 0;
    int rc = ffhip_jpeg_probe(files[0], lens[0], &g, &w, &h);
    if (rc) return rc;
    if (geom_out) *geom_out = g;
    if (g.mcu_cols <= 0 || g.mcu_rows <= 0 || ffhip_jpeg_workspace_bytes(&g, 1) != 0) return FFHIP_EINVAL;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t mcus = (size_t)g.mcu_cols * g.mcu_rows;
    const size_t yb = mcus * g.h * g.v * 64, cb = g.ncomp == 3 ? mcus * 64 : 0; /* int16 elements per picture */
    hipStream_t st = (hipStream_t)stream;
    if (jpeg_entropy_on_device(files[0], lens[0], n)) {
        /* entropy decode on the device, straight into planes in library scratch; the reconstruction is enqueued by the entropy call itself, behind
         * each part of the batch as it is decoded */
        const PlaneBlock blk((size_t)n * yb, (size_t)n * cb, (size_t)n);
        uint8_t *base = (uint8_t *)ffhip_scratch(SCRATCH_FILES_DEV, stream, blk.bytes / 4 + 16);
        if (!base) return FFHIP_ENOMEM;
        const Planes d = blk.at(base);
        const FfhipHuffThen then = {d_bgra, pitch, image_stride, nullptr};
        rc = jpeg_entropy_batch_gpu_impl(files, lens, n, n_threads, &g, nullptr, d.y, d.u, d.v, d.q, status, stream, &then);
        if (rc == FFHIP_OK) return FFHIP_OK;
        if (rc != FFHIP_EINVAL) return rc;
    }
    /* Host threads (the gate's answer, or the device call refused the files).  A pipeline of
     * chunks over the two slots ffhip_jpeg_decode_files uses: while the host threads decode chunk k + 1 into pinned memory, chunk k is copied
     * to the device and reconstructed on the slot's own stream, straight into the caller's d_bgra.  (Until round 5 this path decoded the whole
     * batch into pageable vectors, then uploaded it: 1.84 s for 256 4K files, most of it page faults and a pageable copy of 9.5 GB.)  Everything
     * has run when the call returns. */
    int chunk = n_threads < 8 ? 8 : (n_threads > 32 ? 32 : n_threads);
    if (chunk > n) chunk = n;
    FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO); /* d_bgra may still be read by what `stream` holds */
    std::lock_guard<std::mutex> lock(g_pipe_mu);
    Slot *slot = g_slot;
    for (int s = 0; s < 2; s++)
        if (!prepare(slot[s], chunk * yb * 2, chunk * cb * 2, (size_t)chunk * 512, 0, false)) return FFHIP_ENOMEM;
    int result = FFHIP_OK, k = 0;
    rc = FFHIP_OK;
    for (int first = 0; first < n && rc == FFHIP_OK; first += chunk, k++) {
        Slot &sl = slot[k & 1];
        const int cnt = n - first < chunk ? n - first : chunk;
        if (hipStreamSynchronize(sl.st) != hipSuccess) { rc = FFHIP_EIO; break; } /* the slot's previous chunk (k - 2) has left its pinned planes */
        rc = host_decode_chunk(sl, files, lens, first, cnt, n_threads, g, yb, cb, status, &result);
        if (rc) break;
        rc = ffhip_jpeg_recon_batch(&g, cnt, sl.d_y, cb ? sl.d_u : nullptr, cb ? sl.d_v : nullptr, sl.d_q, 256, d_bgra + (int64_t)first * image_stride, pitch, image_stride,
                                    nullptr, 0, sl.st);
    }
    for (int s = 0; s < 2; s++)
        if (hipStreamSynchronize(slot[s].st) != hipSuccess && rc == FFHIP_OK) rc = FFHIP_EIO;
    return rc ? rc : result;
}

/* Files of any baseline geometry, pixels on the device, one call: headers on host threads, the files grouped by layout class (the items
 * kernels take one class a launch, the device entropy decoder one MCU block record a call), and per class the device entropy decoder
 * over pictures of different sizes with one ffhip_jpeg_recon_items launch behind each part of its write pass; a class it refuses goes to
 * host threads.  A class's planes are library scratch of the stream, reused by the next class: every class's work has run when its
 * turn ends (the entropy call synchronises the stream). */
/* denom == NULL: every picture at full size, the call as it was.  Otherwise picture i at 1 / denom[i] of its size (ffhip_jpeg_recon_items_scaled):
 * its output is checked against the SCALED coded width, and the denominators travel with the items to both reconstruction sites -- behind
 * the device entropy decoder's parts, and behind the host threads' upload */
/* flags (ffhip_jpeg_decode_files_mixed_device_ex): 0, the call as it was.  FFHIP_JPEG_ACCEPT_PROGRESSIVE: the probe is ffhip_jpeg_probe_any, and a
 * class's progressive files take a turn of their own behind its baseline files: the same planes, items and reconstruction, another front end --
 * jpeg_progressive_batch_gpu_impl or ffhip_jpeg_progressive_decode on host threads (FFHIP_JPEG_PROGRESSIVE_GPU; unset: host threads, DESIGN.md
 * 4.14), with k_max = 0 / 4 / 24 for a file at 1/8, 1/4, 1/2 size: the reconstruction reads no coefficient behind those.
 * FFHIP_JPEG_PIXELS_LIBJPEG: the reconstruction at all three sites is ffhip_jpeg_recon_items_libjpeg with the probed display sizes (DESIGN.md
 * 4.16); any denominator but 1 refuses the call */
static int jpeg_decode_files_mixed(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch,
                                   const int *denom, unsigned flags, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status)) || (flags & ~(FFHIP_JPEG_ACCEPT_PROGRESSIVE | FFHIP_JPEG_PIXELS_LIBJPEG))) return FFHIP_EINVAL;
    const bool lj = (flags & FFHIP_JPEG_PIXELS_LIBJPEG) != 0; /* libjpeg's pixels: full size only */
    for (int i = 0; denom && i < n; i++)
        if (!jpeg_denom_ok(denom[i]) || (lj && denom[i] != 1)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    /* ---- headers: each file's geometry and class; a file the mixed path cannot take (progressive, 12-bit, a two-pass layout, an output
     * or pitch ffhip_jpeg_recon_items refuses) has its code now and takes no further part ---- */
    std::vector<ffhip_jpeg_geom> geoms((size_t)n);
    std::vector<int> cls((size_t)n, -1);
    std::vector<int> prog((size_t)n, 0); /* 1: a progressive file (never with flags = 0) */
    std::vector<ffhip_size> shown(lj ? (size_t)n : 0); /* the probed display sizes: ffhip_jpeg_recon_items_libjpeg's */
    int prog_last[5] = {0, 0, 0, 0, 0};
    const JpegChoices ch = jpeg_choices();
    ffhip_parallel_for(n, n_threads, [&](int i) {
        int w = 0, h = 0;
        ffhip_jpeg_geom &g = geoms[(size_t)i];
        memset(&g, 0, sizeof(g));
        if (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) status[i] = files[i] && lens[i] ? ffhip_jpeg_probe_any(files[i], lens[i], &g, &w, &h, &prog[(size_t)i]) : FFHIP_EINVAL;
        else status[i] = files[i] && lens[i] ? ffhip_jpeg_probe(files[i], lens[i], &g, &w, &h) : FFHIP_EINVAL;
        if (geom_out) geom_out[i] = g;
        if (status[i]) return;
        if (lj) {
            shown[(size_t)i] = ffhip_size{w, h};
            cls[(size_t)i] = jpeg_libjpeg_item_ok(&g, w, h, d_bgra[i], pitch[i]) ? jpeg_geom_class(&g) : -1;
        } else if (denom && denom[i] > 1) /* the output holds the scaled picture: rows of 8 / denom x h x mcu_cols pixels */
            cls[(size_t)i] = jpeg_scaled_item_class(&g, denom[i], d_bgra[i], pitch[i]);
        else
            cls[(size_t)i] = jpeg_item_class(ch, &g, d_bgra[i], pitch[i]);
        if (cls[(size_t)i] < 0) status[i] = FFHIP_EINVAL;
    });
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    int rc = FFHIP_OK;
    const int turns = (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) ? 2 : 1;
    for (int turn = 0; turn < JPEG_CLASSES * turns && rc == FFHIP_OK; turn++) {
        const int c = turn / turns, pg = turn % turns; /* a class's baseline files, then its progressive files */
        std::vector<int> idx;
        for (int i = 0; i < n; i++)
            if (cls[(size_t)i] == c && prog[(size_t)i] == pg) idx.push_back(i);
        const int nc = (int)idx.size();
        if (!nc) continue;
        std::vector<const uint8_t *> cf((size_t)nc);
        std::vector<size_t> cl((size_t)nc);
        std::vector<ffhip_jpeg_geom> cg((size_t)nc);
        std::vector<ffhip_jpeg_item> items((size_t)nc);
        std::vector<int> cs((size_t)nc, 0), cd((size_t)nc, 1); /* cd: the class's denominators */
        std::vector<ffhip_size> cshown(lj ? (size_t)nc : 0);
        std::vector<size_t> base((size_t)nc + 1); /* MCUs of the class's pictures before picture k */
        for (int k = 0; k < nc; k++) {
            const int i = idx[(size_t)k];
            if (denom) cd[(size_t)k] = denom[i];
            if (lj) cshown[(size_t)k] = shown[(size_t)i];
            cf[(size_t)k] = files[i]; cl[(size_t)k] = lens[i]; cg[(size_t)k] = geoms[(size_t)i];
            ffhip_jpeg_item &it = items[(size_t)k];
            memset(&it, 0, sizeof(it));
            it.geom = geoms[(size_t)i]; it.d_bgra = d_bgra[i]; it.pitch = pitch[i];
            base[(size_t)k + 1] = base[(size_t)k] + (size_t)it.geom.mcu_cols * it.geom.mcu_rows;
        }
        const ffhip_jpeg_geom &g0 = cg[0];
        const size_t mcus = base[(size_t)nc], yb = mcus * g0.h * g0.v * 64, cb = g0.ncomp == 3 ? mcus * 64 : 0; /* int16 elements of the class */
        const PlaneBlock blk(yb, cb, (size_t)nc);
        uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_FILES_MIXED, stream, blk.bytes / 4 + 16);
        if (!dev) { rc = FFHIP_ENOMEM; break; }
        const Planes d = blk.at(dev);
        bool done = false;
        std::vector<int> kmax((size_t)nc, 63); /* progressive files: the last coefficient the reconstruction reads */
        for (int k = 0; pg && k < nc; k++) kmax[(size_t)k] = cd[(size_t)k] == 8 ? 0 : cd[(size_t)k] == 4 ? 4 : cd[(size_t)k] == 2 ? 24 : 63;
        const char *pgpu = pg ? FFHIP_ENV("FFHIP_JPEG_PROGRESSIVE_GPU") : nullptr;
        if (pg && pgpu && pgpu[0] == '1') {
            const FfhipHuffThen then = {nullptr, 0, 0, items.data(), denom && !lj ? cd.data() : nullptr, lj ? cshown.data() : nullptr};
            int counts[4] = {0, 0, 0, 0};
            const int grc = jpeg_progressive_batch_gpu_impl(cf.data(), cl.data(), nc, n_threads, &g0, cg.data(), d.y, d.u, d.v, d.q, 63, kmax.data(), cs.data(),
                                                            stream, &then, counts);
            if (grc != FFHIP_OK && grc != FFHIP_EINVAL) { rc = grc; break; }
            done = grc == FFHIP_OK;
            if (done) {
                for (int q = 0; q < 4; q++) prog_last[q] += counts[q];
                prog_last[4] = 1;
            }
        } else if (!pg && jpeg_entropy_on_device(cf[0], cl[0], nc)) {
            const FfhipHuffThen then = {nullptr, 0, 0, items.data(), denom && !lj ? cd.data() : nullptr, lj ? cshown.data() : nullptr};
            const int grc = jpeg_entropy_batch_gpu_impl(cf.data(), cl.data(), nc, n_threads, &g0, cg.data(), d.y, d.u, d.v, d.q, cs.data(), stream, &then);
            if (grc != FFHIP_OK && grc != FFHIP_EINVAL) { rc = grc; break; }
            done = grc == FFHIP_OK;
        }
        if (!done) {
            /* host threads: each picture at its own offsets of the pinned planes, one upload, the good pictures reconstructed */
            if (hipStreamSynchronize(st) != hipSuccess) { rc = FFHIP_EIO; break; } /* the scratch may still be read by what `stream` holds */
            uint8_t *pin = ffhip_pinned_scratch(SCRATCH_FILES_MIXED, stream, blk.bytes);
            if (!pin) { rc = FFHIP_ENOMEM; break; }
            const Planes h = blk.at(pin);
            std::vector<std::array<int, 3>> pcounts(pg ? (size_t)nc : 0);
            ffhip_parallel_for(nc, n_threads, [&](int k) {
                const ffhip_jpeg_geom &g = cg[(size_t)k];
                const size_t b = base[(size_t)k];
                if (pg) {
                    pcounts[(size_t)k] = {0, 0, 0};
                    cs[(size_t)k] = ffhip_prog_decode_host(cf[(size_t)k], cl[(size_t)k], &g, h.y + b * g.h * g.v * 64, h.u ? h.u + b * 64 : nullptr,
                                                           h.v ? h.v + b * 64 : nullptr, h.q + (size_t)k * 256, kmax[(size_t)k], pcounts[(size_t)k].data());
                    return;
                }
                cs[(size_t)k] = ffhip_jpeg_entropy_decode(cf[(size_t)k], cl[(size_t)k], &g, h.y + b * g.h * g.v * 64, h.u ? h.u + b * 64 : nullptr,
                                                          h.v ? h.v + b * 64 : nullptr, h.q + (size_t)k * 256);
            });
            if (pg) {
                for (int k = 0; k < nc; k++) {
                    prog_last[0] += pcounts[(size_t)k][0] + pcounts[(size_t)k][1] > 0; /* files that parsed, as the device front end counts them */
                    for (int q = 0; q < 3; q++) prog_last[1 + q] += pcounts[(size_t)k][(size_t)q];
                }
                prog_last[4] = 0;
            }
            if (hipMemcpyAsync(dev, pin, blk.bytes, hipMemcpyHostToDevice, st) != hipSuccess) { rc = FFHIP_EIO; break; }
            std::vector<ffhip_jpeg_item> good;
            std::vector<int> good_d;
            std::vector<ffhip_size> good_s;
            for (int k = 0; k < nc; k++) {
                if (cs[(size_t)k]) continue;
                ffhip_jpeg_item it = items[(size_t)k];
                jpeg_item_planes(&it, d.y, d.u, d.v, d.q, base[(size_t)k], (size_t)k);
                good.push_back(it);
                good_d.push_back(cd[(size_t)k]);
                if (lj) good_s.push_back(cshown[(size_t)k]);
            }
            rc = lj ? jpeg_recon_items_libjpeg_impl(good.data(), good_s.data(), (int)good.size(), stream, 0)
                 : denom ? jpeg_recon_items_scaled_impl(good.data(), good_d.data(), (int)good.size(), stream, 0)
                         : jpeg_recon_items_impl(good.data(), (int)good.size(), stream, 0);
            if (hipStreamSynchronize(st) != hipSuccess && rc == FFHIP_OK) rc = FFHIP_EIO;
        }
        for (int k = 0; k < nc; k++) status[idx[(size_t)k]] = cs[(size_t)k];
    }
    if (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) ffhip_prog_note_last(prog_last);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}

extern "C" int ffhip_jpeg_decode_files_mixed_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                                       const int64_t *pitch, const int *denom, unsigned flags, ffhip_jpeg_geom *geom_out,
                                                       int *status, void *stream)
{
    return jpeg_decode_files_mixed(files, lens, n, n_threads, d_bgra, pitch, denom, flags, geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_mixed_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                                    uint8_t *const *d_bgra, const int64_t *pitch, ffhip_jpeg_geom *geom_out,
                                                    int *status, void *stream)
{
    return jpeg_decode_files_mixed(files, lens, n, n_threads, d_bgra, pitch, nullptr, 0u, geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_mixed_device_scaled(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                                           uint8_t *const *d_bgra, const int64_t *pitch, const int *denom,
                                                           ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (n > 0 && !denom) return FFHIP_EINVAL;
    return jpeg_decode_files_mixed(files, lens, n, n_threads, d_bgra, pitch, denom, 0u, geom_out, status, stream);
}
