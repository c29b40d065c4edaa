/* ffhip_internal.h -- shared by the .hip translation units of libffpic_hip.so. */
#ifndef FFHIP_INTERNAL_H
#define FFHIP_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "ffpic_hip.h"

#define FFHIP_CHECK(expr, code)                    \
    do {                                           \
        hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess) {                   \
            ffhip_note_hip_error((int)e__, #expr); \
            return (code);                         \
        }                                          \
    } while (0)

#ifdef __cplusplus
extern "C" {
#endif
void ffhip_note_hip_error(int hip_error, const char *what);
int ffhip_have_device(void); /* 1 once ffhip_init succeeded on a gfx950 device */
uint32_t *ffhip_scratch(int kind, void *stream, size_t words); /* per (kind, device, stream) device scratch, NULL on failure */
uint8_t *ffhip_pinned_scratch(int kind, void *stream, size_t bytes); /* per (kind, device, stream) pinned host staging, NULL on failure */
/* the same staging for a call that only enqueues: waits for the copy out of it that the stream's previous call of this kind recorded with
 * ffhip_pinned_staged (not for the whole stream), so that the buffer may be refilled */
uint8_t *ffhip_pinned_staging(int kind, void *stream, size_t bytes);
int ffhip_pinned_staged(int kind, void *stream); /* behind the copy just enqueued out of the kind's staging on `stream` */
int *ffhip_async_err_word(void); /* pinned word kernels report an in-launch abort through; see ffhip_stream_sync */
void ffhip_release_caches(void); /* frees what the library keeps between calls, every thread's (ffhip_state_release): no call of any thread may be
                                    in flight, its host part included */
/* The FFHIP_* switches (A/B knobs of the tools, diagnostics) are read from the environment ONCE per process, at a call
 * site's first use, and kept; ffhip_reload_env() (public, include/ffpic_hip.h) makes every site read its switch again. */
/* `val` points into storage the library keeps for the life of the process (values are interned, whatever their length:
 * FFHIP_RCCL_LIB is a path), so a pointer a caller got stays valid and unchanged across ffhip_reload_env(); `gen` and `val`
 * are only touched with atomic loads / stores (val first, then gen with release), so lookups may race with a reload. */
struct ffhip_env_site { const char *name; int gen; const char *val; };
const char *ffhip_env_lookup(struct ffhip_env_site *site); /* NULL when unset */
int ffhip_resident_waves(const void *kernel, int block_threads); /* workgroups of `block_threads` threads of `kernel` the device holds at once (occupancy x CUs), cached */
#ifdef __cplusplus
}
#endif

/* codes a dependency-scheduled kernel leaves in the async error word: 1-3 a bounded wait ran out (FFHIP_EIO), 4 the kernel
 * met input it refuses, e.g. a mode byte no VP8 stream can hold (FFHIP_EINVAL) */
#define FFHIP_ASYNC_BAD_INPUT 4

#ifdef __cplusplus
#define FFHIP_ENV(NAME) ([]() -> const char * { static struct ffhip_env_site site = {NAME, -1, nullptr}; return ffhip_env_lookup(&site); }())
#endif

/* f(i) for every i < count over n_threads host threads, strided: thread t takes i = t, t + n_threads, ...; the calling thread is thread 0,
 * and one thread (or one item) runs inline */
template <class F> void ffhip_parallel_for(int count, int n_threads, F f)
{
    if (n_threads > count) n_threads = count;
    if (n_threads <= 1) { for (int i = 0; i < count; i++) f(i); return; }
    std::vector<std::thread> pool;
    auto part = [&](int t) { for (int i = t; i < count; i += n_threads) f(i); };
    for (int t = 1; t < n_threads; t++) pool.emplace_back(part, t);
    part(0);
    for (auto &th : pool) th.join();
}
inline int ffhip_host_threads(int n_threads) { return n_threads < 1 ? 1 : n_threads > 64 ? 64 : n_threads; }

typedef unsigned int u32;
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#ifdef __HIPCC__
/* Device-coherent ("sc1") loads that are ORDINARY loads to the compiler: a relaxed agent-scope
 * __hip_atomic_load of a sub-dword type gets an s_waitcnt vmcnt(0) right behind it (its extension
 * is a separate instruction), which serialises every fetch; a raw buffer load with the sc1 bit in
 * its cache policy is the same memory operation and is waited for at first use only.
 * Out-of-range offsets (offset >= bytes, so negative ones too) read as 0. */
#define FFHIP_AUX_SC1 16
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ffhip_rsrc(const void *base, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ int ffhip_load_u8_sc1(__amdgpu_buffer_rsrc_t r, int byte_off)
{
    return (int)(unsigned char)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, FFHIP_AUX_SC1);
}
__device__ __forceinline__ int ffhip_load_s16_sc1(__amdgpu_buffer_rsrc_t r, int byte_off)
{
    return (int)(short)__builtin_amdgcn_raw_buffer_load_b16(r, byte_off, 0, FFHIP_AUX_SC1);
}
#endif

/* Kinds of ffhip_scratch / ffhip_pinned_scratch: a (kind, device, stream) owns its buffer.  ".. + n": the kind's sub-slots go up to kind + n.
 * (tests/test_scratch_fill_gpu.py reads this enum, ranges included: a kind added here needs a case there that runs on its buffer behind a fill.) */
enum FfhipScratchKind {
    SCRATCH_VP8_PRED = 1,
    SCRATCH_VP8_LF = 2,
    SCRATCH_HEVC_INTRA = 3,
    SCRATCH_HUFF = 4,
    SCRATCH_FILES_DEV = 5,
    SCRATCH_JPEG_HOST = 6,
    SCRATCH_VP8_RETRY = 8,
    SCRATCH_VP8_FRAMES = 9,        /* .. + 1 */
    SCRATCH_FILES_PLANES = 11,     /* a slot stream of the JPEG file pipeline (ffhip_pipeline.hip): a chunk's planes and quantiser tables, and their pinned twin the host threads decode into */
    SCRATCH_FILES_PIXELS = 12,     /* a slot stream of ffhip_jpeg_decode_files: a chunk's pictures at ffhip_bgra_layout's pitch; pinned, the tight staging of a pageable destination */
    SCRATCH_HEVC_TILES_ONE = 25,   /* .. + 1 */
    SCRATCH_HUFF_SYNC = 30,        /* .. + FFHIP_HUFF_PARTS - 1 */
    SCRATCH_FILES_MIXED = 7,       /* ffhip_jpeg_decode_files_mixed_device: a class's planes and quantiser tables, the host decoder's pinned planes */
    SCRATCH_JPEG_ITEMS = 40,       /* .. + FFHIP_HUFF_PARTS - 1: ffhip_jpeg_recon_items' records and per-workgroup table, pinned records */
    SCRATCH_WEBP = 60,             /* .. + 1: ffhip_webp_decode_files_device: a part's arrays, descriptors and file bytes (and their pinned copy); the host threads' pinned arrays */
    SCRATCH_VP8_LIBWEBP = 55,      /* .. + 1: the libwebp rule of ffhip_vp8_decode_items: the colour items' records and table (pinned records); the filtered planes */
    SCRATCH_VP8_ITEMS = 50,        /* .. + 2: ffhip_vp8_decode_items' tables (and their pinned copy), the levels items' residual, the line slots */
    SCRATCH_TENSOR_ITEMS = 70,     /* ffhip_bgra_to_tensor_items' records and per-workgroup table, pinned records */
    SCRATCH_TENSOR_BGRA = 71,      /* ffhip_*_decode_files_tensor: a part's BGRA pictures */
    SCRATCH_RESIZE_ITEMS = 72,     /* ffhip_bgra_resize_items' records, per-workgroup table and tap tables, pinned records */
    SCRATCH_RESIZE_BGRA = 73,      /* ffhip_*_decode_files_tensor_resized: a part's resized BGRA pictures */
    SCRATCH_ORIENT_ITEMS = 74,     /* ffhip_bgra_orient_items' records and per-workgroup table, pinned records */
    SCRATCH_ORIENT_BGRA = 75,      /* ffhip_*_decode_files_tensor_oriented: a part's upright BGRA pictures */
    SCRATCH_JPEG_SCALED = 80,     /* .. + FFHIP_HUFF_PARTS - 1: ffhip_jpeg_recon_items_scaled's records and per-workgroup table, pinned records */
    SCRATCH_JPEG_LIBJPEG = 100,   /* .. + FFHIP_HUFF_PARTS - 1: ffhip_jpeg_recon_items_libjpeg's records, per-workgroup tables and sample planes, pinned records */
    SCRATCH_PNG = 110,           /* .. + 2: ffhip_png_decode_files_device: a part's filtered pictures and palettes (and their pinned copy); k_png_unfilter's records; k_png_expand's records and per-workgroup table (pinned records).  With FFHIP_PNG_INFLATE_DEVICE slot + 0 holds, behind the filtered pictures, the palettes, the host-inflated files' filtered bytes, the zlib streams and k_inflate's records (their pinned copy: everything but the pictures); ffhip_inflate_streams_device: the streams and records in slot + 0 */
    SCRATCH_VP8L = 113,          /* .. + 2: ffhip_vp8l_decode_files_device: a part's residual images, block images and palettes (and their pinned copy); k_vp8l_predict's records; k_vp8l_finish's records and per-workgroup table (pinned records) */
    SCRATCH_WEBP_ALPHA = 116,    /* .. + 5: FFHIP_WEBP_ALPHA: a part's raw planes and lossless planes' residual images (and their pinned copy); k_vp8l_predict's records; k_vp8l_finish's records and table; the scratch pictures and unfiltered planes; k_webp_alpha_unfilter's records; k_webp_alpha_merge's records and table (pinned records) */
    SCRATCH_JPEG_ENC = 130,      /* .. + 4: the JPEG encoder.  + 0 ffhip_jpeg_fdct_items' records, per-workgroup tables and sample planes (pinned records); + 1 ffhip_jpeg_huff_encode_items' records, code tables, per-workgroup table, positions and results (pinned records); + 2 its stream records, per-chunk table, FF counts, unstuffed streams and masks (pinned records); + 3 its results on the host (pinned only); + 4 ffhip_jpeg_encode_items: a part's coefficient planes */
    SCRATCH_PNG_ENC = 140,       /* .. + 1: ffhip_png_encode_items and ffhip_deflate_streams_device (one call of either at a time per stream).  + 0 a part's picture and stream records (pinned records), per-workgroup tables, chunk offsets and results, verdicts, the chunks' zeroed output words, the filtered pictures, the token words; + 1 the verdicts on the host (pinned only) */
    SCRATCH_VP8L_ENC = 150,      /* .. + 1: ffhip_vp8l_encode_items.  + 0 a part's picture records (pinned records), per-workgroup tables, the chunks' bits and positions, the tables of codes, verdicts, the sub-images, the zeroed counters and files' words, the residual pictures, the token words; + 1 the verdicts on the host (pinned only) */
    SCRATCH_VP8_ENC = 160,       /* .. + 1: ffhip_vp8_encode_items.  + 0 a part's picture records (pinned records), per-workgroup tables, the files' records, masks, levels, modes, source planes and reconstruction, the partitions; + 1 the files' records on the host (pinned only) */
    SCRATCH_HUFF_PROG = 90,      /* ffhip_jpeg_progressive_batch_gpu: staged scans, tables, records and work lists (and their pinned copy) */
};

/* ffhip_vp8_decode_items (ffhip_vp8_frame.hip): its levels items' residual stage (ffhip_vp8.hip) and its device mode check
 * (ffhip_vp8_pred.hip).  Both tables end in a sentinel whose `first` is the total. */
struct Vp8ResItem {
    const int16_t *levels; /* [n_mb][25][16] */
    const uint8_t *info;   /* [n_mb][32] */
    int16_t *out;          /* [n_mb][384]: the call's residual scratch at `first` */
    long long first;       /* its first macroblock among the call's levels items */
    uint16_t quant[32];    /* [4][8] as Vp8ResArgs::quant */
};
struct Vp8CheckItem { const uint8_t *modes; long long first; /* its first record among the items checked on the device */ };
int vp8_residual_items_enqueue(const Vp8ResItem *d_items, int n, long long n_mb, uint32_t *d_wg_item, void *stream);
int vp8_check_modes_items_enqueue(const Vp8CheckItem *d_items, int n, long long n_records, uint32_t *ctrl, int *async_err, void *stream);

/* ---- WEBP_RULE_LIBWEBP behind the front end (ffhip_vp8_bool.h has the rule's value) ----
 * the residual stage's items (ffhip_vp8_libwebp.hip): as Vp8ResItem, with the item's mode records, byte [19] of which receives "some block of
 * the macroblock has a non-zero dequantised coefficient"; the table ends in a sentinel whose `first` is the total */
struct Vp8LwResItem : Vp8ResItem {
    uint8_t *modes; /* [n_mb][20], the call's own copy */
};
int vp8_libwebp_residual_items_enqueue(const Vp8LwResItem *d_items, int n, long long n_mb, void *stream);
/* planes to BGRA over the display rectangle, a HOST array of items, one launch (k_vp8_upsample_color): planes 4-byte aligned, strides multiples
 * of 4 with ys >= width rounded up to 4; bgra 16-byte aligned, pitch a multiple of 16.  Only enqueues */
struct Vp8LwColorItem {
    const uint8_t *y, *u, *v;
    int ys, uvs, width, height;
    uint8_t *bgra;
    long long pitch;
};
int vp8_libwebp_color_items(const Vp8LwColorItem *items, int n, void *stream);
/* ffhip_vp8_decode_items under a rule.  WEBP_RULE_LIBWEBP: levels items without a residual map only; display[i] = the picture's width and height
 * (within its macroblock grid); planes: NULL or per item a triple y, u, v that receives the filtered planes as well */
int vp8_decode_items_rule(const ffhip_vp8_item *items, int n, int rule, const ffhip_size *display, uint8_t *const *planes, void *stream);

/* FFHIP_WEBP_ALPHA behind the colour of ffhip_webp_decode_files_device_ex (ffhip_webp_alpha_gpu.hip): the files with status[i] == 0 that have an
 * alpha plane get it in byte 3 of their width x height pixels; a refused plane sets status[i].  Synchronises the stream part by part */
int webp_alpha_stage(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch, int *status,
                     void *stream);

/* ffhip_vp8_decode_frames (row form) -> ffhip_vp8_predict_loopfilter: the colour conversion the caller enqueues behind the call belongs to
 * it -- a retry has to run it again, behind the filter */
struct FfhipVp8Then { uint8_t *bgra; int pitch; int64_t image_stride; };

/* ffhip_vp8_predict_loopfilter: the two row kernels of one call side by side (ffhip_vp8_lf.hip).  The prediction records `fork` behind its
 * counter reset and fills in the rest; the loop filter launches on `side` behind `fork`, polling the prediction's counters. */
struct Vp8SideBySide {
    hipStream_t side;
    hipEvent_t fork;
    int *err_word; /* where the two kernels of THIS call report a bounded wait that ran out: the call's own pinned word (its retry record's), so that
                      nobody else's abort can set off the retry; NULL = the process-wide word */
    const uint32_t *pred_progress; /* set by the prediction: its per-row counters (NULL: it did not launch the row kernel) */
    int pshift;     /* set by the prediction: a row's progress counter is word (image * mbrows + row) << pshift */
    int pred_split; /* set by the prediction: it runs luma and chroma rows apart, its chroma counters (behind the luma ones) count too */
};
/* the entry points with their hand-offs as an argument (the public entries pass NULL) */
int vp8_predict_recon_impl(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                           int64_t residual_stride, const int32_t *d_resmap, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y,
                           int64_t plane_stride_uv, void *stream, Vp8SideBySide *sbs);
int vp8_loopfilter_impl(int mbcols, int mbrows, int n_images, int filter_type, const uint8_t *d_modes, const uint8_t *d_filters, uint8_t *d_y,
                        uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y, int64_t plane_stride_uv, void *stream, const Vp8SideBySide *sbs);
int vp8_predict_args_check(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                           int64_t residual_stride, const uint8_t *d_y, const uint8_t *d_u, const uint8_t *d_v);
/* shared by the two stages' host entries (ffhip_vp8_pred.hip).  The row forms' switches: FFHIP_VP8_PROGRESS_SHIFT, FFHIP_VP8_SLACK, and where the
 * kernel reports a wait that ran out -- the process-wide pinned word, the side-by-side call's own, or NULL: no row form (`mode` is "levels") */
struct Vp8RowSwitches { int pshift, slack; int *async_err; };
Vp8RowSwitches vp8_row_switches(const char *mode, const Vp8SideBySide *sbs);
/* the levels forms' common end: lists[level] = (image, macroblock) pairs; flattened into scratch `scratch_kind` of the stream (after a
 * synchronise: an earlier call may still read it), then launch(work, count) for every level that has pairs, in order */
int vp8_levels_upload_and_launch(int scratch_kind, void *stream, const std::vector<std::vector<uint32_t>> &lists,
                                 const std::function<void(const uint32_t *work, int count)> &launch);
int vp8_predict_loopfilter_impl(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes, const int16_t *d_residual,
                                int64_t residual_stride, const int32_t *d_resmap, int filter_type, const uint8_t *d_filters, uint8_t *d_y,
                                uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y, int64_t plane_stride_uv, void *stream, const FfhipVp8Then *then);

/* Which reconstruction a JPEG file call gives its pictures.  Both NULL: the reference's pixels at full size (ffhip_jpeg_recon_items).  denom:
 * per picture its denominator 1, 2, 4 or 8 (ffhip_jpeg_recon_items_scaled).  display, never with denom: per picture its display size, libjpeg's
 * pixels (ffhip_jpeg_recon_items_libjpeg) */
struct JpegPixelRule {
    const int *denom;
    const ffhip_size *display;
    JpegPixelRule at(int lo) const { return {denom ? denom + lo : nullptr, display ? display + lo : nullptr}; } /* the rule of the pictures from lo on */
};
/* ffhip_jpeg_decode_files_device -> ffhip_jpeg_entropy_batch_gpu: the reconstruction of the pictures, enqueued by the entropy call itself behind
 * each part of the batch it has decoded */
/* items (mixed batches, ffhip_jpeg_decode_files_mixed_device): per picture its geometry, output and pitch; the call fills in the plane and
 * quantiser pointers and reconstructs with jpeg_recon_items_by_rule under `rule` instead (bgra, pitch and image_stride unused) */
struct FfhipHuffThen { uint8_t *bgra; int64_t pitch, image_stride; const ffhip_jpeg_item *items; JpegPixelRule rule; };
/* geoms: NULL = every picture has *geom; else picture i has geoms[i], all of *geom's layout class (ncomp, h, v): the planes hold the
 * pictures one behind the other, picture i at the sum of the MCUs of the pictures before it */
int jpeg_entropy_batch_gpu_impl(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_jpeg_geom *geom,
                                const ffhip_jpeg_geom *geoms, int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant,
                                int *status, void *stream, const FfhipHuffThen *then);
/* ffhip_jpeg_progressive_batch_gpu (ffhip_huff_prog_gpu.hip) with per-picture geometries of one layout class, a k_max per picture (k_maxes, or NULL:
 * k_max for all) and the hand-off (items form only).  counts[4] += progressive files, scans decoded, scans skipped, levels launched.  FFHIP_OK when the
 * batch ran, whatever the files' own verdicts in status[]; FFHIP_EINVAL when the call refuses the batch as a whole */
int jpeg_progressive_batch_gpu_impl(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_jpeg_geom *geom,
                                    const ffhip_jpeg_geom *geoms, int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant,
                                    int k_max, const int *k_maxes, int *status, void *stream, const FfhipHuffThen *then, int counts[4]);
/* The layout classes of the fused JPEG kernels (ffhip_jpeg.hip: 4:2:0, 4:4:4, 4:2:2, 4:4:0, h4v1, h1v4, grey) and what one call chooses for its
 * kernels, read from the FFHIP_JPEG_* switches once, up front */
#define JPEG_CLASSES 7
struct JpegChoices {
    int variant; /* 4:2:0: <quads per wave><nt bits> */
    int remap;   /* the mode of the workgroup-to-XCD remap */
    int strips[JPEG_CLASSES], mps[JPEG_CLASSES], per_wave[JPEG_CLASSES]; /* per class: strips' worth per wave (1 / 2), MCUs of a unit (a quad, or
                                                                            that many strips), units a wave takes */
};
JpegChoices jpeg_choices(void);
/* the layout class 0..6 of a picture ffhip_jpeg_recon_items takes with this output and pitch under these choices, -1 if it refuses it */
int jpeg_item_class(const JpegChoices &ch, const ffhip_jpeg_geom *g, const uint8_t *d_bgra, int64_t pitch);
int jpeg_geom_class(const ffhip_jpeg_geom *g); /* the layout class 0..6 of a geometry, -1 for a bad one and for the two-pass layouts */
/* the layout class 0..6 of a picture ffhip_jpeg_recon_items_scaled takes at denominator 2, 4 or 8 with this output and pitch, -1 if it refuses
 * it: the one statement of what that call asks of geometry and output (ffhip_jpeg_scaled.hip) */
int jpeg_scaled_item_class(const ffhip_jpeg_geom *g, int denom, const uint8_t *d_bgra, int64_t pitch);
/* what ffhip_jpeg_recon_items_libjpeg asks of one picture's geometry, display size, output and pitch (the planes aside) */
bool jpeg_libjpeg_item_ok(const ffhip_jpeg_geom *g, int width, int height, const uint8_t *d_bgra, int64_t pitch);
/* The three items calls with scratch slot 0..FFHIP_HUFF_PARTS-1: ffhip_jpeg_recon_items; ffhip_jpeg_recon_items_scaled (item i at 1 / denom[i]
 * of its size, denominator 1 through jpeg_recon_items_impl); ffhip_jpeg_recon_items_libjpeg.  The file calls reach them through the rule only */
int jpeg_recon_items_impl(const ffhip_jpeg_item *items, int n, void *stream, int slot);
int jpeg_recon_items_scaled_impl(const ffhip_jpeg_item *items, const int *denom, int n, void *stream, int slot);
int jpeg_recon_items_libjpeg_impl(const ffhip_jpeg_item *items, const ffhip_size *display, int n, void *stream, int slot);
/* The two owners of "which pixels" (ffhip_jpeg.hip).  The items call of the rule over n items, the rule's arrays in the items' order; and the
 * layout class 0..6 that call gives picture i of the rule (geometry *g, display size w x h) with this output and pitch, -1 if it refuses it */
int jpeg_recon_items_by_rule(const ffhip_jpeg_item *items, const JpegPixelRule &rule, int n, void *stream, int slot);
int jpeg_rule_item_class(const JpegChoices &ch, const JpegPixelRule &rule, int i, const ffhip_jpeg_geom *g, int w, int h, const uint8_t *d_bgra, int64_t pitch);
/* A JPEG file's header for the file calls: ffhip_jpeg_probe, or with FFHIP_JPEG_ACCEPT_PROGRESSIVE in flags ffhip_jpeg_probe_any; a NULL or
 * empty file is FFHIP_EINVAL.  Geometry, display size and the progressive bit are zero where the probe left them so */
struct JpegProbed { ffhip_jpeg_geom geom; int width, height, progressive, status; };
JpegProbed jpeg_probe_file(const uint8_t *file, size_t len, unsigned flags);
/* ffhip_jpeg_decode_files_mixed_device_ex's body (ffhip_pipeline.hip): the three public mixed file calls and the tensor file calls' parts */
int jpeg_decode_files_mixed(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra, const int64_t *pitch,
                            const int *denom, unsigned flags, ffhip_jpeg_geom *geom_out, int *status, void *stream);
/* the plane and quantiser pointers of picture `index` of a call whose planes hold its pictures one behind the other: the picture's blocks start
 * at MCU `mcu_base` of y / u / v (u, v NULL for grey), its tables are the index-th 256 of q */
inline void jpeg_item_planes(ffhip_jpeg_item *it, const int16_t *y, const int16_t *u, const int16_t *v, const uint16_t *q, size_t mcu_base, size_t index)
{
    it->d_coef_y = y + mcu_base * it->geom.h * it->geom.v * 64;
    it->d_coef_u = u ? u + mcu_base * 64 : nullptr;
    it->d_coef_v = v ? v + mcu_base * 64 : nullptr;
    it->d_quant = q + index * 256;
}

/* ---- what the library keeps between calls (ffhip_state.hip) ---- */
/* The record of a stream's last side-by-side VP8 call, for its repeat by ffhip_stream_sync (ffhip_vp8_lf.hip); `armed` says whether it
 * describes a call.  The mode copy's storage and the pinned word are reused call after call. */
struct FfhipVp8Retry {
    bool armed = false;
    int mbcols = 0, mbrows = 0, n_images = 0, filter_type = 0;
    std::vector<uint8_t> h_modes;
    const uint8_t *d_modes = nullptr, *d_filters = nullptr;
    const int16_t *d_residual = nullptr;
    int64_t residual_stride = 0, plane_y = 0, plane_uv = 0;
    const int32_t *d_resmap = nullptr;
    uint8_t *y = nullptr, *u = nullptr, *v = nullptr, *keep = nullptr;
    FfhipVp8Then then = {nullptr, 0, 0}; /* bgra NULL: none */
    int *err = nullptr; /* pinned, device-visible: the call's own abort word */
    unsigned long long seq = 0; /* the stream's vp8_seq behind the call */
};
/* Who used a one-chunk scratch of ffhip_hevc_intra_recon_tiles last (ffhip_hevc_intra.hip): the parity of the call, and per scratch an event
 * recorded on the stream behind the call's grouped kernel.  Calls that share a stream take turns (`turn`) for the length of their enqueue. */
struct FfhipTileGuard {
    std::mutex turn;
    unsigned parity = 0;
    bool recorded[2] = {false, false};
    hipEvent_t ev[2] = {nullptr, nullptr};
};
struct FfhipBuf { void *p = nullptr; size_t cap = 0; };
/* One per (device, stream), made on first use.  A stream of ffhip_stream_create's loses its entries in ffhip_stream_destroy, any other stream
 * in ffhip_release_caches / ffhip_shutdown. */
struct FfhipStreamState {
    std::map<int, FfhipBuf> scratch, pinned; /* by kind; cap in words / bytes */
    std::map<int, hipEvent_t> staged;        /* by kind: behind the last copy out of its pinned staging (ffhip_pinned_staged) */
    FfhipVp8Retry retry;
    unsigned long long vp8_seq = 0; /* VP8 prediction / filter calls enqueued so far: a retry record is only good while its call is the LAST of them */
    FfhipTileGuard tiles;
};
/* the entry of (current device, stream), made when missing unless !make; hold g_ffhip_state_mu while touching it (the tile guard's `turn` aside) */
extern std::mutex g_ffhip_state_mu;
FfhipStreamState *ffhip_stream_state(void *stream, bool make = true);
void ffhip_state_release(void); /* no call of any thread in flight: empties both registries */
void ffhip_hevc_plan_result_forget(void *stream); /* ffhip_hevc_intra.hip, for ffhip_debug_scratch_fill: the calling thread's pointer to its last plan's verdict in `stream`'s scratch */
int ffhip_vp8_side_by_side_retry(void *stream); /* ffhip_vp8_lf.hip, for ffhip_stream_sync: 0 nothing reported by a side-by-side call of this
                                                   stream, FFHIP_RETRIED repeated, FFHIP_EIO */
struct jpeg_hdr *ffhip_huff_hdr_records(size_t n); /* the calling thread's header records, room for at least n, kept between calls; NULL: no memory */

/* the calling thread's side stream with its fork / join events (ffhip_state.hip: one set per thread and device) */
struct FfhipSide { void *stream, *fork, *join, *mid; }; /* mid: a second point of the main stream the side stream may wait for */
extern "C" int ffhip_side_stream_get(FfhipSide *out);
/* the calling thread's stream and event for the early pre-pass of ffhip_hevc_intra_recon_tiles: the stream the pre-passes follow each other on,
 * the event the caller's stream waits for in front of the grouped kernel; same owner and lifetime as the side stream */
struct FfhipPipe { void *plan, *plan_done; };
extern "C" int ffhip_pipe_streams_get(FfhipPipe *out);
/* the calling thread's two slot streams of the JPEG file pipeline (ffhip_pipeline.hip); same owner and lifetime, and what the registry keeps
 * under them (SCRATCH_FILES_PLANES, SCRATCH_FILES_PIXELS, the device front end's kinds) goes with them */
struct FfhipSlotStreams { void *s[2]; };
extern "C" int ffhip_slot_streams_get(FfhipSlotStreams *out);

/* ... and the device Huffman decoder's (ffhip_jpeg_entropy_batch_gpu): the copy stream its parts' bytes go up on, the second kernel stream, the
 * parts' events, fork / join, two timing events; all made together (none is published unless all exist); same owner and lifetime */
#define FFHIP_HUFF_PARTS 8
struct FfhipHuffStreams { void *up, *c2, *part_ev[FFHIP_HUFF_PARTS], *fork, *join, *time_ev[2]; };
extern "C" int ffhip_huff_streams_get(FfhipHuffStreams *out);

/* Control words of the VP8 row kernels (ffhip_vp8_pred.hip, ffhip_vp8_lf.hip; the scratch they live in starts on a 256-byte boundary): the
 * ticket counters -- one device-scope atomic per row from every wave -- and the abort word -- read by waiting waves between polls -- each
 * ALONE in a 128-byte line, the per-row progress counters behind them.  (Until late in round 4 they were words 0, 2 and 1 of one line, with
 * the first progress counters behind them in the same line: every poll of a waiting wave queued up with the ticket atomics.) */
#define FFHIP_VP8_CTRL_TICKET_C 32
#define FFHIP_VP8_CTRL_ABORT 64
#define FFHIP_VP8_CTRL_HDR 128
#define FFHIP_VP8_LF_CTRL_ABORT 32
#define FFHIP_VP8_LF_CTRL_HDR 64

#endif
