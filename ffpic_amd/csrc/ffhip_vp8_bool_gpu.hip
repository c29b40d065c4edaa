/* ffhip_vp8_bool_gpu.hip -- the VP8 bool decoder on the device: lossy WebP files to BGRA with only the file bytes crossing PCIe.
 *
 * The host parses each file's frame header (ffhip_webp_read_header: a few hundred bool decodes) and hands over the first
 * partition's decoder state, the probabilities and the partition table.  Two kernels then do what vp8_decode's macroblock loop
 * does in front of the predictor (format/webp.c:1833-1844), with the per-macroblock parsers of ffhip_vp8_bool.h that the host
 * front end runs as well:
 *   k_webp_mb_headers  the first partition: vp8_decode_mb_header for every macroblock -> mode records, skip flags, residual map
 *   k_webp_tokens      the token partitions: vp8_decode_residual_data for every macroblock -> levels, token counts
 * and ffhip_vp8_decode_items takes it from there.  Arithmetic decoding is serial per stream, so the unit of parallelism is the
 * frame: ONE LANE decodes a frame in either kernel.  A lone active lane issues as fast as a full wave, so every frame has a wave
 * of its own while a part has no more frames than the device holds waves; beyond that `pack` frames share a wave, one per lane,
 * divergent.  A frame with several token partitions is walked row by row by its one lane (row y reads partition
 * y & (nbr_partitions - 1), webp.c:1836), the decoders it is not using parked in memory: there are no waits between lanes or
 * waves anywhere.  The coefficient probabilities of a wave's frames sit in LDS. */
#include <string.h>

#include <algorithm>
#include <vector>

#include "ffhip_internal.h"
#include "ffhip_webp_internal.h"

#define WEBP_PACK_MAX 32                /* frames per wave at most: 32 x 1056 bytes of probabilities in LDS */
#define WEBP_PART_MB_HOST (1LL << 19)   /* macroblocks per part of a call, host-thread front end: bounds the scratch and its pinned mirror */
#define WEBP_PART_MB_DEVICE (1LL << 23) /* ... device front end: a part costs what its LARGEST frame costs one lane, however many frames it
                                           holds, so the parts are as large as the scratch bound allows (include/ffpic_hip.h) */
#define WEBP_SCRATCH_KEEP (1ull << 30)  /* a part's arrays above this size are the call's own allocation, freed when the part is done */
/* Unforced, a part goes to the kernels when it is worth at least this many of its largest frame PER HOST THREAD of the call (macroblocks of
 * the part / macroblocks of its largest file: the file count, for files of one size), to the host threads below.  A lane takes 45 us per
 * macroblock of a photograph and a host thread 1.7 us, a ratio of 26; measured with 16 threads the kernels lose at 256
 * copies of a 1080p stream (16 per thread) and win at 512 (32 per thread).  Other thread counts were not measured: the threshold assumes
 * that the host threads scale linearly, as they do from 1 to 16 on this stream (14 ms a frame on one core, 1.0 ms at 16). */
#define FFHIP_WEBP_GPU_FILES_PER_THREAD 32

struct WebpDesc {
    const uint8_t *bytes; /* the file from its first partition on */
    uint32_t p0_len, pos, value, range;
    int32_t count;
    ffb_mbhdr_probs mb;
    int32_t mbcols, mbrows, nparts;
    uint32_t part_off[8], part_len[8]; /* from `bytes` */
    uint8_t *modes;   /* [n_mb][20] */
    int16_t *levels;  /* [n_mb][25][16], cleared */
    uint8_t *mbinfo;  /* [n_mb][32], cleared */
    int32_t *resmap;  /* [n_mb] */
    uint8_t *skip;    /* [n_mb] mb_skip_coeff */
    uint16_t *top;    /* [mbcols] the nine context flags of each column, cleared */
    uint32_t *parked; /* [8][4] value, range, count, pos of the token decoders the lane is not using */
    uint8_t probs[1056];
};

/* the two kernels, once per rule */
#define WEBP_K_HEADERS k_webp_mb_headers
#define WEBP_K_TOKENS k_webp_tokens
#define WEBP_K_RULE WEBP_RULE_REFERENCE
#define WEBP_K_MB_TOKENS ffb_mb_tokens
#include "ffhip_vp8_bool_kernels.inc"
#undef WEBP_K_HEADERS
#undef WEBP_K_TOKENS
#undef WEBP_K_RULE
#undef WEBP_K_MB_TOKENS
#define WEBP_K_HEADERS k_webp_mb_headers_libwebp
#define WEBP_K_TOKENS k_webp_tokens_libwebp
#define WEBP_K_RULE WEBP_RULE_LIBWEBP
#define WEBP_K_MB_TOKENS ffb_mb_tokens_libwebp
#include "ffhip_vp8_bool_kernels.inc"
#undef WEBP_K_HEADERS
#undef WEBP_K_TOKENS
#undef WEBP_K_RULE
#undef WEBP_K_MB_TOKENS

namespace {

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

/* where a part's arrays lie in its device scratch (and in the pinned mirror of the host path) */
struct PartLayout {
    size_t levels, mbinfo, modes, resmap, skip, top, parked, descs, verdict, bytes, total;
    PartLayout(size_t n_mb, size_t cols_sum, size_t n_files, size_t file_bytes)
    {
        size_t o = 0;
        levels = o; o = up16(o + n_mb * 800);
        mbinfo = o; o = up16(o + n_mb * 32);
        top = o; o = up16(o + cols_sum * 2); /* levels, token counts and contexts are cleared together */
        modes = o; o = up16(o + n_mb * 20);
        resmap = o; o = up16(o + n_mb * 4);
        skip = o; o = up16(o + n_mb);
        parked = o; o = up16(o + n_files * 128);
        descs = o; o = up16(o + n_files * sizeof(WebpDesc));
        verdict = o; o = up16(o + n_files * 8);
        bytes = o; o = up16(o + file_bytes + 16);
        total = o;
    }
};

struct PartFile {
    int idx;          /* in the call */
    size_t first_mb, first_col, byte_off, byte_len;
};

thread_local int t_last_parts[2]; /* parts of the calling thread's last call that went to the kernels / to the host threads */

int env_int(const char *v, int dflt) { return v && *v ? atoi(v) : dflt; }

/* One part: the arrays of its files on the device (kernels, or host threads + upload), each file's verdict in status[]; when
 * `outs` is given the arrays are copied back to the host instead of being decoded (ffhip_webp_parse_device). */
int run_part(const std::vector<PartFile> &pf, const std::vector<ffhip_webp_frame> &frames, const uint8_t *const *files, const size_t *lens,
             size_t n_mb, size_t cols_sum, size_t file_bytes, bool on_device, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch,
             ffhip_webp_parsed *outs, int *status, void *stream, int rule, uint8_t *const *planes)
{
    const bool lw = rule == WEBP_RULE_LIBWEBP;
    hipStream_t st = (hipStream_t)stream;
    const int nf = (int)pf.size();
    const PartLayout L(n_mb, cols_sum, (size_t)nf, on_device ? file_bytes : 0);
    /* up to WEBP_SCRATCH_KEEP the arrays are library scratch of the stream, kept between calls; a larger part (hundreds of 1080p frames)
     * allocates its own and gives them back when it is done, so that no call leaves gigabytes standing on the device */
    struct Own {
        void *p = nullptr;
        ~Own() { if (p) (void)hipFree(p); }
    } own;
    uint8_t *dev = nullptr;
    if (L.total > WEBP_SCRATCH_KEEP) {
        FFHIP_CHECK(hipMalloc(&own.p, L.total + 64), FFHIP_ENOMEM);
        dev = (uint8_t *)own.p;
    } else {
        dev = (uint8_t *)ffhip_scratch(SCRATCH_WEBP, stream, L.total / 4 + 16);
    }
    if (!dev) return FFHIP_ENOMEM;
    if (on_device) {
        const size_t pin_bytes = L.total - L.descs; /* descriptors, verdicts (unused on the host side), file bytes: one upload */
        uint8_t *pin = ffhip_pinned_scratch(SCRATCH_WEBP, stream, pin_bytes);
        if (!pin) return FFHIP_ENOMEM;
        WebpDesc *hd = (WebpDesc *)pin;
        uint8_t *hbytes = pin + (L.bytes - L.descs);
        ffhip_parallel_for(nf, n_threads, [&](int k) {
            const PartFile &p = pf[(size_t)k];
            const ffhip_webp_frame &f = frames[(size_t)p.idx];
            memcpy(hbytes + p.byte_off, files[p.idx] + f.p0_off, p.byte_len);
            WebpDesc &D = hd[k];
            D.bytes = dev + L.bytes + p.byte_off;
            D.p0_len = f.p0_len; D.pos = f.pos; D.value = f.value; D.range = f.range; D.count = f.count;
            D.mb = f.mb;
            D.mbcols = f.info.mbcols; D.mbrows = f.info.mbrows; D.nparts = f.info.nbr_partitions;
            for (int q = 0; q < 8; q++) { D.part_off[q] = q < D.nparts ? f.part_off[q] - f.p0_off : 0; D.part_len[q] = q < D.nparts ? f.part_len[q] : 0; }
            D.levels = (int16_t *)(dev + L.levels) + p.first_mb * 400;
            D.mbinfo = dev + L.mbinfo + p.first_mb * 32;
            D.modes = dev + L.modes + p.first_mb * 20;
            D.resmap = (int32_t *)(dev + L.resmap) + p.first_mb;
            D.skip = dev + L.skip + p.first_mb;
            D.top = (uint16_t *)(dev + L.top) + p.first_col;
            D.parked = (uint32_t *)(dev + L.parked) + (size_t)k * 32;
            memcpy(D.probs, f.probs, 1056);
        });
        FFHIP_CHECK(hipMemcpyAsync(dev + L.descs, pin, pin_bytes, hipMemcpyHostToDevice, st), FFHIP_EIO);
        FFHIP_CHECK(hipMemsetAsync(dev + L.levels, 0, L.modes - L.levels, st), FFHIP_EIO);
        int slots = ffhip_resident_waves(lw ? (const void *)k_webp_tokens_libwebp : (const void *)k_webp_tokens, 64);
        if (slots < 1) slots = 1024;
        int pack = nf <= slots ? 1 : std::min(WEBP_PACK_MAX, (nf + slots - 1) / slots);
        pack = std::max(1, std::min(WEBP_PACK_MAX, env_int(FFHIP_ENV("FFHIP_WEBP_PACK"), pack))); /* tests: several frames to a wave in a small batch */
        const int grid = (nf + pack - 1) / pack;
        const WebpDesc *dd = (const WebpDesc *)(dev + L.descs);
        int32_t *dv = (int32_t *)(dev + L.verdict);
        if (lw) {
            hipLaunchKernelGGL(k_webp_mb_headers_libwebp, dim3(grid), dim3(64), 0, st, dd, nf, pack, dv);
            hipLaunchKernelGGL(k_webp_tokens_libwebp, dim3(grid), dim3(64), (size_t)pack * 1056, st, dd, nf, pack, dv);
        } else {
            hipLaunchKernelGGL(k_webp_mb_headers, dim3(grid), dim3(64), 0, st, dd, nf, pack, dv);
            hipLaunchKernelGGL(k_webp_tokens, dim3(grid), dim3(64), (size_t)pack * 1056, st, dd, nf, pack, dv);
        }
        FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
        std::vector<int32_t> verdict((size_t)nf * 2);
        FFHIP_CHECK(hipMemcpyAsync(verdict.data(), dv, (size_t)nf * 8, hipMemcpyDeviceToHost, st), FFHIP_EIO);
        FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO);
        /* The kernels refuse one thing, a partition asked for a byte beyond its length, and the host parser -- the same source over the
         * same lengths -- refuses exactly that: their verdict is the file's code, there is nothing a second parse on the host could save. */
        for (int k = 0; k < nf; k++)
            if (verdict[2 * (size_t)k] | verdict[2 * (size_t)k + 1]) status[pf[(size_t)k].idx] = FFHIP_EINVAL;
    } else {
        /* host threads, into a pinned mirror of the four arrays the decode reads, uploaded whole */
        FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO); /* the scratch may still be read by what `stream` holds */
        uint8_t *pin = ffhip_pinned_scratch(SCRATCH_WEBP + 1, stream, L.skip);
        if (!pin) return FFHIP_ENOMEM;
        ffhip_parallel_for(nf, n_threads, [&](int k) {
            const PartFile &p = pf[(size_t)k];
            status[p.idx] = (lw ? ffhip_webp_parse_frame_libwebp : ffhip_webp_parse_frame)(files[p.idx], &frames[(size_t)p.idx], pin + L.modes + p.first_mb * 20,
                                                   (int16_t *)(pin + L.levels) + p.first_mb * 400, pin + L.mbinfo + p.first_mb * 32,
                                                   (int32_t *)(pin + L.resmap) + p.first_mb);
        });
        FFHIP_CHECK(hipMemcpyAsync(dev, pin, L.skip, hipMemcpyHostToDevice, st), FFHIP_EIO);
    }
    if (outs) { /* the raw arrays back to the caller */
        for (int k = 0; k < nf; k++) {
            const PartFile &p = pf[(size_t)k];
            if (status[p.idx]) continue;
            const size_t m = (size_t)frames[(size_t)p.idx].info.mbcols * frames[(size_t)p.idx].info.mbrows;
            ffhip_webp_parsed &o = outs[p.idx];
            FFHIP_CHECK(hipMemcpyAsync(o.levels, dev + L.levels + p.first_mb * 800, m * 800, hipMemcpyDeviceToHost, st), FFHIP_EIO);
            FFHIP_CHECK(hipMemcpyAsync(o.mbinfo, dev + L.mbinfo + p.first_mb * 32, m * 32, hipMemcpyDeviceToHost, st), FFHIP_EIO);
            FFHIP_CHECK(hipMemcpyAsync(o.modes, dev + L.modes + p.first_mb * 20, m * 20, hipMemcpyDeviceToHost, st), FFHIP_EIO);
            FFHIP_CHECK(hipMemcpyAsync(o.resmap, dev + L.resmap + p.first_mb * 4, m * 4, hipMemcpyDeviceToHost, st), FFHIP_EIO);
        }
        FFHIP_CHECK(hipStreamSynchronize(st), FFHIP_EIO);
        return FFHIP_OK;
    }
    std::vector<ffhip_vp8_item> items;
    std::vector<ffhip_size> display;
    std::vector<uint8_t *> item_planes;
    for (int k = 0; k < nf; k++) {
        const PartFile &p = pf[(size_t)k];
        if (status[p.idx]) continue;
        const ffhip_webp_frame &f = frames[(size_t)p.idx];
        ffhip_vp8_item it;
        memset(&it, 0, sizeof(it));
        it.mbcols = f.info.mbcols;
        it.mbrows = f.info.mbrows;
        it.d_modes = dev + L.modes + p.first_mb * 20; /* h_modes NULL: checked on the device */
        it.d_levels = (const int16_t *)(dev + L.levels) + p.first_mb * 400;
        it.d_mbinfo = dev + L.mbinfo + p.first_mb * 32;
        memcpy(it.quant, f.info.quant, sizeof(it.quant));
        it.d_resmap = lw ? nullptr : (const int32_t *)(dev + L.resmap) + p.first_mb; /* the libwebp rule's map is the identity */
        it.filter_type = f.info.filter_type;
        memcpy(it.filters, f.info.filters, sizeof(it.filters));
        it.d_bgra = d_bgra[p.idx];
        it.pitch = pitch[p.idx];
        items.push_back(it);
        display.push_back({f.info.width, f.info.height});
        if (planes)
            for (int q = 0; q < 3; q++) item_planes.push_back(planes[3 * p.idx + q]);
    }
    /* (the mode records are this part's scratch: the libwebp rule's residual stage writes their byte [19]) */
    int rc = vp8_decode_items_rule(items.data(), (int)items.size(), rule, lw ? display.data() : nullptr, planes ? item_planes.data() : nullptr, stream);
    const int src = ffhip_stream_sync(stream); /* the next part reuses the scratch */
    if (rc == FFHIP_OK && src < 0) rc = src;
    return rc;
}

int webp_files_impl(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch,
                    ffhip_webp_info *info_out, ffhip_webp_parsed *outs, int *status, void *stream, int rule, uint8_t *const *planes)
{
    const bool lw = rule == WEBP_RULE_LIBWEBP;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    std::vector<ffhip_webp_frame> frames((size_t)n);
    ffhip_parallel_for(n, n_threads, [&](int i) {
        ffhip_webp_frame &f = frames[(size_t)i];
        status[i] = files[i] && lens[i] ? (lw ? ffhip_webp_read_header_libwebp : ffhip_webp_read_header)(files[i], lens[i], &f) : FFHIP_EINVAL;
        if (info_out) info_out[i] = f.info;
        if (status[i]) return;
        const int64_t n_mb = (int64_t)f.info.mbcols * f.info.mbrows;
        if (outs) {
            ffhip_webp_parsed &o = outs[i];
            if (!o.modes || !o.levels || !o.mbinfo || !o.resmap || o.n_mb_cap < n_mb) status[i] = FFHIP_EINVAL;
            else o.info = f.info;
        } else if (!d_bgra[i] || ((uintptr_t)d_bgra[i] & 15) || pitch[i] < 64LL * f.info.mbcols || pitch[i] > 0x7fffffffLL ||
                   (pitch[i] & 15) || pitch[i] * 16 * f.info.mbrows > 0x7fffffffLL) { /* what ffhip_vp8_decode_items asks of an output */
            status[i] = FFHIP_EINVAL;
        } else if (planes && (!planes[3 * i] || !planes[3 * i + 1] || !planes[3 * i + 2] ||
                              (((uintptr_t)planes[3 * i] | (uintptr_t)planes[3 * i + 1] | (uintptr_t)planes[3 * i + 2]) & 3))) {
            status[i] = FFHIP_EINVAL;
        }
    });
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const char *ge = FFHIP_ENV("FFHIP_WEBP_GPU_ENTROPY");
    const int min_files = env_int(FFHIP_ENV("FFHIP_WEBP_GPU_MIN_FILES"), FFHIP_WEBP_GPU_FILES_PER_THREAD * n_threads);
    t_last_parts[0] = t_last_parts[1] = 0;
    const long long forced_mb = env_int(FFHIP_ENV("FFHIP_WEBP_PART_MB"), 0); /* tests: small parts */
    int rc = FFHIP_OK;
    int i = 0;
    while (i < n && rc == FFHIP_OK) {
        /* the part the kernels would take from here; should it be the host threads' instead, it is cut again at their bound */
        std::vector<PartFile> pf;
        size_t n_mb = 0, cols_sum = 0, file_bytes = 0, max_mb = 0;
        bool on_device = true;
        int next = i;
        for (int pass = 0; pass < 2; pass++) {
            const long long cap = forced_mb > 0 ? forced_mb : on_device ? WEBP_PART_MB_DEVICE : WEBP_PART_MB_HOST;
            pf.clear();
            n_mb = cols_sum = file_bytes = max_mb = 0;
            for (next = i; next < n; next++) {
                if (status[next]) continue;
                const ffhip_webp_frame &f = frames[(size_t)next];
                const size_t m = (size_t)f.info.mbcols * f.info.mbrows;
                if (!pf.empty() && n_mb + m > (size_t)cap) break;
                size_t end = (size_t)f.p0_off + f.p0_len;
                for (int q = 0; q < f.info.nbr_partitions; q++) end = std::max(end, (size_t)f.part_off[q] + f.part_len[q]);
                pf.push_back({next, n_mb, cols_sum, file_bytes, end - f.p0_off});
                n_mb += m;
                max_mb = std::max(max_mb, m);
                cols_sum += (size_t)f.info.mbcols;
                file_bytes = up16(file_bytes + (end - f.p0_off));
            }
            if (pf.empty() || pass == 1) break;
            on_device = outs || (ge ? ge[0] != '0' : n_mb >= (size_t)min_files * max_mb);
            if (on_device) break;
        }
        if (pf.empty()) break;
        i = next;
        t_last_parts[on_device ? 0 : 1]++;
        rc = run_part(pf, frames, files, lens, n_mb, cols_sum, file_bytes, on_device, n_threads, d_bgra, pitch, outs, status, stream, rule, planes);
    }
    if (rc) return rc;
    for (int k = 0; k < n; k++)
        if (status[k]) return status[k];
    return FFHIP_OK;
}

} // namespace

extern "C" int ffhip_webp_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                              const int64_t *pitch, ffhip_webp_info *info_out, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    return webp_files_impl(files, lens, n, n_threads, d_bgra, pitch, info_out, nullptr, status, stream, WEBP_RULE_REFERENCE, nullptr);
}

extern "C" int ffhip_webp_decode_files_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                                 const int64_t *pitch, uint8_t *const *planes, unsigned flags, ffhip_webp_info *info_out, int *status,
                                                 void *stream)
{
    if (flags & ~(FFHIP_WEBP_PIXELS_LIBWEBP | FFHIP_WEBP_ALPHA)) return FFHIP_EINVAL;
    const int rule = (flags & FFHIP_WEBP_PIXELS_LIBWEBP) ? WEBP_RULE_LIBWEBP : WEBP_RULE_REFERENCE;
    if ((flags & FFHIP_WEBP_ALPHA) && rule != WEBP_RULE_LIBWEBP) return FFHIP_EINVAL; /* the alpha plane goes with libwebp's pixels only */
    if (planes && rule != WEBP_RULE_LIBWEBP) return FFHIP_EINVAL; /* the default rule's file call writes no planes */
    if (n < 0 || (n > 0 && (!files || !lens || !d_bgra || !pitch || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    int rc = webp_files_impl(files, lens, n, n_threads, d_bgra, pitch, info_out, nullptr, status, stream, rule, planes);
    if (!(flags & FFHIP_WEBP_ALPHA)) return rc;
    /* the colour is what the unflagged call gives; a failure that is no file's own ends the call */
    int first = FFHIP_OK;
    for (int k = 0; k < n && !first; k++) first = status[k];
    if (rc != first) return rc;
    rc = webp_alpha_stage(files, lens, n, n_threads, d_bgra, pitch, status, stream);
    if (rc) return rc;
    for (int k = 0; k < n; k++)
        if (status[k]) return status[k];
    return FFHIP_OK;
}

extern "C" int ffhip_webp_parse_device(const uint8_t *const *files, const size_t *lens, int n, ffhip_webp_parsed *outs, int *status, void *stream)
{
    if (n < 0 || (n > 0 && (!files || !lens || !outs || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    return webp_files_impl(files, lens, n, 1, nullptr, nullptr, nullptr, outs, status, stream, WEBP_RULE_REFERENCE, nullptr);
}

extern "C" int ffhip_webp_parse_device_ex(const uint8_t *const *files, const size_t *lens, int n, unsigned flags, ffhip_webp_parsed *outs, int *status,
                                          void *stream)
{
    if (flags & ~FFHIP_WEBP_PIXELS_LIBWEBP) return FFHIP_EINVAL;
    if (n < 0 || (n > 0 && (!files || !lens || !outs || !status))) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    return webp_files_impl(files, lens, n, 1, nullptr, nullptr, nullptr, outs, status, stream,
                           (flags & FFHIP_WEBP_PIXELS_LIBWEBP) ? WEBP_RULE_LIBWEBP : WEBP_RULE_REFERENCE, nullptr);
}

extern "C" int ffhip_debug_webp_last_parts(int out[2])
{
    if (!out) return FFHIP_EINVAL;
    out[0] = t_last_parts[0];
    out[1] = t_last_parts[1];
    return FFHIP_OK;
}
