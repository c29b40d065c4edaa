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
#include "ffhip_planes.h"

#include <stdlib.h>
#include <string.h>

#include <array>
#include <vector>

namespace {
/* rows of `count` pictures from tight pinned staging to the caller's pageable buffer, a contiguous range of them to each of 16 host threads
 * at most; fewer than 64 rows are copied inline (ffhip_planes.h) */
void copy_out(uint8_t *bgra, int64_t pitch, int64_t image_stride, const uint8_t *src, size_t row_b, int64_t height, int first, int count,
              int n_threads)
{
    const long long rows = (long long)count * height;
    const int nt = ffhip_copy_threads(rows, n_threads);
    ffhip_parallel_for(nt, nt, [&](int t) {
        const FfhipRows mine = ffhip_copy_rows(rows, t, nt);
        for (long long r = mine.lo; r < mine.hi; r++) {
            const long long i = r / height, y = r % height;
            memcpy(bgra + (first + i) * image_stride + y * pitch, src + (size_t)r * row_b, row_b);
        }
    });
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

/* One of the calling thread's two slots, as a call sees it: the slot's stream (kept per thread and device, ffhip_slot_streams_get) and what
 * the registry keeps under it (pinning hundreds of MB costs more than decoding them): a chunk's planes and tables as one block on the
 * device and its pinned twin, both laid out by PlaneBlock; for ffhip_jpeg_decode_files the chunk's pictures on the device and, for a
 * pageable destination, their tight pinned staging */
struct Slot {
    hipStream_t st;
    uint8_t *h_blk, *d_blk;
    uint8_t *d_out, *h_out;
    int first, count; /* pictures in flight in this slot */
};
/* both slots for chunks of blk_bytes of planes and tables and out_bytes of pictures (0: none), the staging where need_hout */
int take_slots(Slot slot[2], size_t blk_bytes, size_t out_bytes, bool need_hout)
{
    FfhipSlotStreams ss;
    const int rc = ffhip_slot_streams_get(&ss);
    if (rc) return rc;
    for (int s = 0; s < 2; s++) {
        Slot &sl = slot[s];
        sl = Slot{(hipStream_t)ss.s[s], nullptr, nullptr, nullptr, nullptr, -1, 0};
        sl.d_blk = (uint8_t *)ffhip_scratch(SCRATCH_FILES_PLANES, sl.st, (blk_bytes + 3) / 4);
        sl.h_blk = ffhip_pinned_scratch(SCRATCH_FILES_PLANES, sl.st, blk_bytes);
        if (!sl.d_blk || !sl.h_blk) return FFHIP_ENOMEM;
        if (out_bytes && !(sl.d_out = (uint8_t *)ffhip_scratch(SCRATCH_FILES_PIXELS, sl.st, (out_bytes + 3) / 4))) return FFHIP_ENOMEM;
        if (out_bytes && need_hout && !(sl.h_out = ffhip_pinned_scratch(SCRATCH_FILES_PIXELS, sl.st, out_bytes))) return FFHIP_ENOMEM;
    }
    return FFHIP_OK;
}

/* where the chunk loop's pictures go: DEVICE, the reconstruction writes picture i at dst + i * image_stride itself; PINNED, it writes the
 * slot's pictures and 2-D copies behind it take them to dst; PAGEABLE, one 2-D copy takes them to the slot's staging, and host threads from
 * there to dst once the slot has been waited for */
struct PixelsOut {
    enum { DEVICE, PINNED, PAGEABLE } to;
    uint8_t *dst;
    int64_t pitch, image_stride;
};

/* Files [0, n) of geometry g in chunks over the calling thread's two slots: while the front end works on chunk k + 1, chunk k is on its
 * slot's stream.  The front end is the device decoder where gpu_entropy says so and it takes the chunk (straight into the device planes: the
 * host only parses headers and unstuffs the scan bytes), else host threads into the pinned block and one upload.  Everything has run when
 * it returns.  The host decoder's first code is the call's if nothing worse happens: per-picture codes are in status[], bad pictures still
 * occupy their place. */
int chunk_loop(const uint8_t *const *files, const size_t *lens, int n, int n_threads, int chunk, const ffhip_jpeg_geom &g, bool gpu_entropy,
               const PixelsOut &out, int *status)
{
    const size_t mcus = (size_t)g.mcu_cols * g.mcu_rows;
    const size_t yb = mcus * g.h * g.v * 64, cb = g.ncomp == 3 ? mcus * 64 : 0; /* int16 elements per picture */
    const int64_t width = (int64_t)g.mcu_cols * 8 * g.h, height = (int64_t)g.mcu_rows * 8 * g.v;
    /* on the device the pictures have the pitch ffhip_bgra_layout recommends (the buffer is the library's); the pinned staging
     * for a pageable destination is tight, and every copy off the device is a 2-D copy */
    int64_t lp = 0, ls = 0;
    if (out.to != PixelsOut::DEVICE && ffhip_bgra_layout(&g, &lp, &ls) != FFHIP_OK) return FFHIP_EINVAL;
    const size_t dev_pitch = (size_t)lp, out_b = (size_t)ls, row_b = (size_t)width * 4;
    Slot slot[2];
    int rc = take_slots(slot, PlaneBlock(chunk * yb, chunk * cb, (size_t)chunk).bytes, chunk * out_b, out.to == PixelsOut::PAGEABLE);
    if (rc) return rc;
    int result = FFHIP_OK;
    /* wait for what a slot's stream holds -- its chunk has left the pinned block -- and hand the pixels of a chunk that was enqueued whole to the caller */
    auto drain = [&](Slot &sl) -> int {
        if (hipStreamSynchronize(sl.st) != hipSuccess) return FFHIP_EIO;
        if (sl.count && out.to == PixelsOut::PAGEABLE) copy_out(out.dst, out.pitch, out.image_stride, sl.h_out, row_b, height, sl.first, sl.count, n_threads);
        sl.count = 0;
        return FFHIP_OK;
    };
    int k = 0;
    for (int first = 0; first < n; first += chunk, k++) {
        Slot &sl = slot[k & 1];
        const int cnt = n - first < chunk ? n - first : chunk;
        rc = drain(sl); /* the slot's previous chunk (k - 2) */
        if (rc) break;
        const PlaneBlock blk(cnt * yb, cnt * cb, (size_t)cnt);
        const Planes d = blk.at(sl.d_blk), h = blk.at(sl.h_blk);
        bool on_device = false;
        if (gpu_entropy) {
            const int grc = ffhip_jpeg_entropy_batch_gpu(files + first, lens + first, cnt, n_threads, &g, d.y, d.u, d.v, d.q, status + first, sl.st);
            on_device = grc == FFHIP_OK;
            if (!on_device && grc != FFHIP_EINVAL) { rc = grc; break; }
        }
        if (!on_device) {
            const int erc = ffhip_jpeg_entropy_batch(files + first, lens + first, cnt, n_threads, &g, h.y, h.u, h.v, h.q, status + first);
            if (erc && !result) result = erc;
            if (hipMemcpyAsync(sl.d_blk, sl.h_blk, blk.bytes, hipMemcpyHostToDevice, sl.st) != hipSuccess) { rc = FFHIP_EIO; break; }
        }
        if (out.to == PixelsOut::DEVICE)
            rc = ffhip_jpeg_recon_batch(&g, cnt, d.y, d.u, d.v, d.q, 256, out.dst + (int64_t)first * out.image_stride, out.pitch, out.image_stride, nullptr, 0, sl.st);
        else
            rc = ffhip_jpeg_recon_batch(&g, cnt, d.y, d.u, d.v, d.q, 256, sl.d_out, (int64_t)dev_pitch, (int64_t)out_b, nullptr, 0, sl.st);
        if (rc) break;
        hipError_t e = hipSuccess;
        if (out.to == PixelsOut::PAGEABLE)
            e = hipMemcpy2DAsync(sl.h_out, row_b, sl.d_out, dev_pitch, row_b, (size_t)height * cnt, hipMemcpyDeviceToHost, sl.st);
        else if (out.to == PixelsOut::PINNED && (cnt == 1 || out.image_stride == out.pitch * height)) /* the caller's pictures follow each other row after row: one copy for the chunk */
            e = hipMemcpy2DAsync(out.dst + (int64_t)first * out.image_stride, (size_t)out.pitch, sl.d_out, dev_pitch, row_b, (size_t)height * cnt, hipMemcpyDeviceToHost, sl.st);
        else if (out.to == PixelsOut::PINNED)
            for (int i = 0; i < cnt && e == hipSuccess; i++)
                e = hipMemcpy2DAsync(out.dst + (int64_t)(first + i) * out.image_stride, (size_t)out.pitch, sl.d_out + (size_t)i * out_b, dev_pitch, row_b, (size_t)height,
                                     hipMemcpyDeviceToHost, sl.st);
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
} // namespace

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
    /* a pinned (hipHostMalloc'ed / registered) destination takes the D2H copy directly */
    hipPointerAttribute_t attr;
    const bool pinned_dst = hipPointerGetAttributes(&attr, bgra) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned_dst) (void)hipGetLastError(); /* an unknown pointer leaves an error behind: not ours */
    return chunk_loop(files, lens, n, n_threads, chunk, g, gpu_entropy, {pinned_dst ? PixelsOut::PINNED : PixelsOut::PAGEABLE, bgra, pitch, image_stride}, status);
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
    /* Host threads (the gate's answer, or the device call refused the files).  The chunk loop of ffhip_jpeg_decode_files over the same two slots:
     * while the host threads decode chunk k + 1 into pinned memory, chunk k is copied to the device and reconstructed on the slot's own stream,
     * straight into the caller's d_bgra.  (Until round 5 this path decoded the whole batch into pageable vectors, then uploaded it: 1.84 s for
     * 256 4K files, most of it page faults and a pageable copy of 9.5 GB.)  Everything has run when the call returns. */
    int chunk = n_threads < 8 ? 8 : (n_threads > 32 ? 32 : n_threads);
    if (chunk > n) chunk = n;
    FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO); /* d_bgra may still be read by what `stream` holds */
    return chunk_loop(files, lens, n, n_threads, chunk, g, false, {PixelsOut::DEVICE, d_bgra, pitch, image_stride}, status);
}

namespace {
/* One picture of a class turn: a class's baseline files, or its progressive files */
struct MixedPic {
    int index;            /* the file's place in the call */
    const uint8_t *file;
    size_t len;
    ffhip_jpeg_item item; /* geometry, output and pitch; the turn gives it its place in the class's planes */
    int denom;            /* 1 where the call has none */
    ffhip_size shown;     /* the probed display size (libjpeg's pixels only) */
    size_t mcu_base;      /* MCUs of the turn's pictures in front of this one */
    int k_max;            /* the last coefficient the reconstruction reads: what a progressive file is decoded up to */
    int status;           /* the host threads' verdict */
};

/* the items of a turn's pictures (good_only: of those without a code) and the call's rule over them, in their order */
struct TurnItems {
    std::vector<ffhip_jpeg_item> items;
    std::vector<int> denom;
    std::vector<ffhip_size> display;
    TurnItems(const std::vector<MixedPic> &pics, const JpegPixelRule &call, bool good_only)
    {
        items.reserve(pics.size());
        if (call.denom) denom.reserve(pics.size());
        if (call.display) display.reserve(pics.size());
        for (const MixedPic &p : pics) {
            if (good_only && p.status) continue;
            items.push_back(p.item);
            if (call.denom) denom.push_back(p.denom);
            if (call.display) display.push_back(p.shown);
        }
    }
    JpegPixelRule rule(const JpegPixelRule &call) const { return {call.denom ? denom.data() : nullptr, call.display ? display.data() : nullptr}; }
};

/* A turn through its device front end, the reconstruction behind it by the entropy call itself: jpeg_progressive_batch_gpu_impl (prog) or
 * jpeg_entropy_batch_gpu_impl.  *done = false with FFHIP_OK: the front end refuses the class (FFHIP_EINVAL), host threads take it; any
 * other error ends the call */
int mixed_turn_device(std::vector<MixedPic> &pics, bool prog, const JpegPixelRule &call, const Planes &d, int n_threads, void *stream, int *status,
                      int prog_last[5], bool *done)
{
    const size_t nc = pics.size();
    std::vector<const uint8_t *> files(nc);
    std::vector<size_t> lens(nc);
    std::vector<ffhip_jpeg_geom> geoms(nc);
    std::vector<int> k_maxes(nc), cs(nc, 0);
    for (size_t k = 0; k < nc; k++) {
        files[k] = pics[k].file; lens[k] = pics[k].len; geoms[k] = pics[k].item.geom; k_maxes[k] = pics[k].k_max;
    }
    const TurnItems t(pics, call, false);
    const FfhipHuffThen then = {nullptr, 0, 0, t.items.data(), t.rule(call)};
    int counts[4] = {0, 0, 0, 0};
    const int grc = prog ? jpeg_progressive_batch_gpu_impl(files.data(), lens.data(), (int)nc, n_threads, &geoms[0], geoms.data(), d.y, d.u, d.v, d.q, 63, k_maxes.data(),
                                                           cs.data(), stream, &then, counts)
                         : jpeg_entropy_batch_gpu_impl(files.data(), lens.data(), (int)nc, n_threads, &geoms[0], geoms.data(), d.y, d.u, d.v, d.q, cs.data(), stream, &then);
    *done = grc == FFHIP_OK;
    if (!*done) return grc == FFHIP_EINVAL ? FFHIP_OK : grc;
    if (prog) {
        for (int q = 0; q < 4; q++) prog_last[q] += counts[q];
        prog_last[4] = 1;
    }
    for (size_t k = 0; k < nc; k++) status[pics[k].index] = cs[k];
    return FFHIP_OK;
}

/* A turn on host threads: each picture at its own offsets of the pinned planes, one upload, the good pictures reconstructed.  Everything
 * has run when it returns */
int mixed_turn_host(std::vector<MixedPic> &pics, bool prog, const JpegPixelRule &call, const PlaneBlock &blk, uint8_t *dev, int n_threads, void *stream,
                    int *status, int prog_last[5])
{
    hipStream_t st = (hipStream_t)stream;
    const int nc = (int)pics.size();
    if (hipStreamSynchronize(st) != hipSuccess) return FFHIP_EIO; /* the scratch may still be read by what `stream` holds */
    uint8_t *pin = ffhip_pinned_scratch(SCRATCH_FILES_MIXED, stream, blk.bytes);
    if (!pin) return FFHIP_ENOMEM;
    const Planes h = blk.at(pin);
    std::vector<std::array<int, 3>> pcounts(prog ? (size_t)nc : 0);
    ffhip_parallel_for(nc, n_threads, [&](int k) {
        MixedPic &p = pics[(size_t)k];
        const ffhip_jpeg_geom &g = p.item.geom;
        const size_t b = p.mcu_base;
        int16_t *y = h.y + b * g.h * g.v * 64, *u = h.u ? h.u + b * 64 : nullptr, *v = h.v ? h.v + b * 64 : nullptr;
        uint16_t *q = h.q + (size_t)k * 256;
        if (prog) {
            pcounts[(size_t)k] = {0, 0, 0};
            p.status = ffhip_prog_decode_host(p.file, p.len, &g, y, u, v, q, p.k_max, pcounts[(size_t)k].data());
        } else
            p.status = ffhip_jpeg_entropy_decode(p.file, p.len, &g, y, u, v, q);
    });
    if (prog) {
        for (int k = 0; k < nc; k++) {
            prog_last[0] += pcounts[(size_t)k][0] + pcounts[(size_t)k][1] > 0; /* files that parsed, as the device front end counts them */
            for (int q = 0; q < 3; q++) prog_last[1 + q] += pcounts[(size_t)k][(size_t)q];
        }
        prog_last[4] = 0;
    }
    if (hipMemcpyAsync(dev, pin, blk.bytes, hipMemcpyHostToDevice, st) != hipSuccess) return FFHIP_EIO;
    const TurnItems good(pics, call, true);
    int rc = jpeg_recon_items_by_rule(good.items.data(), good.rule(call), (int)good.items.size(), stream, 0);
    if (hipStreamSynchronize(st) != hipSuccess && rc == FFHIP_OK) rc = FFHIP_EIO;
    for (const MixedPic &p : pics) status[p.index] = p.status;
    return rc;
}

/* One turn: the class's planes in library scratch of the stream, every picture behind the MCUs of those before it; the device front end
 * where the gate (baseline) or FFHIP_JPEG_PROGRESSIVE_GPU=1 (progressive) says so, host threads otherwise and for a class it refuses */
int mixed_turn(std::vector<MixedPic> &pics, bool prog, const JpegPixelRule &call, int n_threads, void *stream, int *status, int prog_last[5])
{
    size_t mcus = 0;
    for (MixedPic &p : pics) {
        p.mcu_base = mcus;
        mcus += (size_t)p.item.geom.mcu_cols * p.item.geom.mcu_rows;
    }
    const ffhip_jpeg_geom &g0 = pics[0].item.geom;
    const PlaneBlock blk(mcus * g0.h * g0.v * 64, g0.ncomp == 3 ? mcus * 64 : 0, pics.size()); /* int16 elements of the class */
    uint8_t *dev = (uint8_t *)ffhip_scratch(SCRATCH_FILES_MIXED, stream, blk.bytes / 4 + 16);
    if (!dev) return FFHIP_ENOMEM;
    const Planes d = blk.at(dev);
    for (size_t k = 0; k < pics.size(); k++) jpeg_item_planes(&pics[k].item, d.y, d.u, d.v, d.q, pics[k].mcu_base, k);
    const char *pgpu = prog ? FFHIP_ENV("FFHIP_JPEG_PROGRESSIVE_GPU") : nullptr;
    bool done = false;
    if (prog ? (pgpu && pgpu[0] == '1') : jpeg_entropy_on_device(pics[0].file, pics[0].len, (int)pics.size())) {
        const int rc = mixed_turn_device(pics, prog, call, d, n_threads, stream, status, prog_last, &done);
        if (rc) return rc;
    }
    return done ? FFHIP_OK : mixed_turn_host(pics, prog, call, blk, dev, n_threads, stream, status, prog_last);
}
} // namespace

JpegProbed jpeg_probe_file(const uint8_t *file, size_t len, unsigned flags)
{
    JpegProbed p;
    memset(&p, 0, sizeof(p));
    if (!file || !len) p.status = FFHIP_EINVAL;
    else if (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) p.status = ffhip_jpeg_probe_any(file, len, &p.geom, &p.width, &p.height, &p.progressive);
    else p.status = ffhip_jpeg_probe(file, len, &p.geom, &p.width, &p.height);
    return p;
}

/* Files of any baseline geometry, pixels on the device, one call: headers on host threads, the files grouped by layout class (the items
 * kernels take one class a launch, the device entropy decoder one MCU block record a call), and per class the device entropy decoder
 * over pictures of different sizes with one items launch (jpeg_recon_items_by_rule) behind each part of its write pass; a class it refuses goes to
 * host threads.  A class's planes are library scratch of the stream, reused by the next class: every class's work has run when its
 * turn ends (the entropy call synchronises the stream). */
/* denom == NULL: every picture at full size, the call as it was.  Otherwise picture i at 1 / denom[i] of its size (ffhip_jpeg_recon_items_scaled):
 * its output is checked against the SCALED coded width, and the denominators travel with the items to both reconstruction sites -- behind
 * the device entropy decoder's parts, and behind the host threads' upload */
/* flags (ffhip_jpeg_decode_files_mixed_device_ex): 0, the call as it was.  FFHIP_JPEG_ACCEPT_PROGRESSIVE: the probe is ffhip_jpeg_probe_any, and a
 * class's progressive files take a turn of their own behind its baseline files: the same planes, items and reconstruction, another front end --
 * jpeg_progressive_batch_gpu_impl or ffhip_jpeg_progressive_decode on host threads (FFHIP_JPEG_PROGRESSIVE_GPU; unset: host threads, DESIGN.md
 * 4.14), with jpeg_scaled_k_max of the file's denominator: the reconstruction reads no coefficient behind it.
 * FFHIP_JPEG_PIXELS_LIBJPEG: the reconstruction at all three sites is ffhip_jpeg_recon_items_libjpeg with the probed display sizes (DESIGN.md
 * 4.16); any denominator but 1 refuses the call */
int jpeg_decode_files_mixed(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch,
                            const int *denom, unsigned flags, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status)) || (flags & ~(FFHIP_JPEG_ACCEPT_PROGRESSIVE | FFHIP_JPEG_PIXELS_LIBJPEG))) return FFHIP_EINVAL;
    const bool lj = (flags & FFHIP_JPEG_PIXELS_LIBJPEG) != 0; /* libjpeg's pixels: full size only */
    for (int i = 0; denom && i < n; i++)
        if (!jpeg_denom_ok(denom[i]) || (lj && denom[i] != 1)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    n_threads = ffhip_host_threads(n_threads);
    /* ---- headers: each file's geometry and class; a file the mixed path cannot take (progressive without the flag, 12-bit, a two-pass
     * layout, an output or pitch the rule's items call refuses) has its code now and takes no further part ---- */
    std::vector<JpegProbed> probed((size_t)n);
    std::vector<int> cls((size_t)n, -1);
    std::vector<ffhip_size> shown(lj ? (size_t)n : 0); /* the probed display sizes: the libjpeg rule's */
    const JpegPixelRule rule = {lj ? nullptr : denom, lj ? shown.data() : nullptr};
    const JpegChoices ch = jpeg_choices();
    ffhip_parallel_for(n, n_threads, [&](int i) {
        JpegProbed &p = probed[(size_t)i];
        p = jpeg_probe_file(files[i], lens[i], flags);
        status[i] = p.status;
        if (geom_out) geom_out[i] = p.geom;
        if (status[i]) return;
        if (lj) shown[(size_t)i] = ffhip_size{p.width, p.height};
        cls[(size_t)i] = jpeg_rule_item_class(ch, rule, i, &p.geom, p.width, p.height, d_bgra[i], pitch[i]);
        if (cls[(size_t)i] < 0) status[i] = FFHIP_EINVAL;
    });
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    int rc = FFHIP_OK;
    int prog_last[5] = {0, 0, 0, 0, 0};
    const int turns = (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) ? 2 : 1;
    int count[JPEG_CLASSES * 2] = {}; /* pictures of every turn */
    for (int i = 0; i < n; i++)
        if (cls[(size_t)i] >= 0) count[cls[(size_t)i] * turns + probed[(size_t)i].progressive]++;
    for (int turn = 0; turn < JPEG_CLASSES * turns && rc == FFHIP_OK; turn++) {
        const int c = turn / turns, pg = turn % turns; /* a class's baseline files, then its progressive files */
        std::vector<MixedPic> pics;
        pics.reserve((size_t)count[turn]);
        for (int i = 0; i < n; i++) {
            if (cls[(size_t)i] != c || probed[(size_t)i].progressive != pg) continue;
            MixedPic p;
            memset(&p, 0, sizeof(p));
            p.index = i; p.file = files[i]; p.len = lens[i];
            p.item.geom = probed[(size_t)i].geom; p.item.d_bgra = d_bgra[i]; p.item.pitch = pitch[i];
            p.denom = denom ? denom[i] : 1;
            if (lj) p.shown = shown[(size_t)i];
            p.k_max = pg ? jpeg_scaled_k_max(p.denom) : 63;
            pics.push_back(p);
        }
        if (!pics.empty()) rc = mixed_turn(pics, pg != 0, rule, n_threads, stream, status, prog_last);
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
