/*
 * ffpic_hip.h -- C ABI of libffpic_hip.so, the MI355X (gfx950) back-end for the
 * post-entropy reconstruction stage of the ffpic image decoder.
 *
 * Everything here is plain C: pointers, sizes, ints.  No C++/torch types.
 * Three groups of entry points, each citing the reference interface it stands
 * behind (paths relative to the ffpic source tree):
 *
 *  (1) the accelerator registry seam           arch/accl.h:13-35, arch/accl.c:17-62
 *  (2) the built-in op tables JPEG decodes by  utils/idct.h:14-25, utils/colorspace.h:29-35
 *  (3) a batched, device-resident extension    (new; the per-block ABI of (1)/(2)
 *      cannot be fast on a GPU -- arch/opencl/opcl.c:42-88 shows why)
 *
 * Error convention of (3): 0 on success, negative errno-style code otherwise
 * (FFHIP_E*).  (1) and (2) return void like the reference; a back-end that
 * cannot run does not register (arch/opencl/opcl.c:112-114), callers fall back
 * to C when the lookup returns NULL (format/webp.c:1173, coding/hevc.c:3913-3919).
 *
 * THREADS AND STREAMS (held by tests/test_concurrent_gpu.py; the state behind it is listed in DESIGN.md 4.27):
 *  - In flight together: calls of different host threads, each on a stream of ITS OWN, and calls of one thread on different streams.  What
 *    the library keeps between calls is per (device, stream) -- scratch, pinned staging, the VP8 retry record, the HEVC tile guard -- or per
 *    (thread, device) -- the side, pipe and Huffman streams it forks work to, the two slot streams of the JPEG file pipeline -- and the
 *    ffhip_debug_*_last* records are per thread: a thread reads the record of its own last call whatever other threads do meanwhile.  A
 *    thread binds its device with ffhip_init first (hipSetDevice is per thread).
 *  - Calls on ONE stream, the NULL stream included, are ordered by the caller: no two threads may have a call on the same stream in
 *    flight, and the entries without a stream argument, other than those of the next point, use the NULL stream.
 *  - Entries that serialise themselves, because each has ONE staging allocation (the NULL stream's): ffhip_jpeg_recon_batch_host and the block
 *    operations (every function of ffhip_accl_ops_get, ffhip_get_dct_ops and ffhip_get_cs_ops, and ffhip_idct_4x4_hevc).  Any number of
 *    threads may call them at once; they take turns, a whole call at a time.
 *  - ffhip_jpeg_decode_files (and the host-thread path of ffhip_jpeg_decode_files_device) shares nothing: each calling thread keeps two slots
 *    per device -- a stream each, with pinned and device memory for a chunk of pictures -- and ffhip_shutdown / ffhip_release_caches or the
 *    thread's end frees them.  Any number of threads may call at once, and none waits for another.
 *  - ffhip_shutdown and hip_accl_uninit free what calls in flight use: every thread must be quiet,
 *    host parts of calls included.  ffhip_stream_destroy needs only its own stream's caller quiet.  ffhip_reload_env may be called at any
 *    time, but a call in flight may have read a switch before it.
 *  - The async error word, through which a dependency-scheduled kernel (VP8 prediction and loop filter, HEVC intra) reports a bounded wait
 *    that ran out, is ONE per process: the next ffhip_stream_sync of ANY thread on ANY stream collects it and returns FFHIP_EIO, once.  (The
 *    side-by-side VP8 call reports into a word of its stream's own: its FFHIP_RETRIED goes to the sync of that stream.)  The text behind
 *    ffhip_strerror(FFHIP_EIO / FFHIP_ENODEV) is the process's last one and may be another thread's.
 */
#ifndef FFPIC_HIP_H
#define FFPIC_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFHIP_ABI_VERSION 1

/* error codes (negative errno values) */
#define FFHIP_OK 0
#define FFHIP_EINVAL (-22)  /* bad argument / unsupported geometry          */
#define FFHIP_ENOMEM (-12)  /* device or host allocation failed             */
#define FFHIP_ENODEV (-19)  /* no usable gfx950 device / HIP runtime error  */
#define FFHIP_EIO    (-5)   /* kernel launch or copy failed                 */
#define FFHIP_RETRIED 1     /* ffhip_stream_sync only, not an error: a side-by-side VP8 call on the stream ran into a bounded wait and was
                               repeated by the sync; its outputs are now those of an undisturbed call, but whatever the CALLER had enqueued
                               behind it on the stream has consumed the aborted run's output and must be enqueued again */

/* ------------------------------------------------------------------ runtime */

/* Number of visible HIP devices (0 when there is no GPU; never fails). */
int ffhip_device_count(void);
/* Bind the calling thread's library state to `device` (hipSetDevice) and create
 * the small internal staging buffers used by the per-block entry points. */
int ffhip_init(int device);
void ffhip_shutdown(void); /* with no call of any thread in flight: frees the scratch and staging the library keeps between calls, with
                              every thread's own streams (the file pipeline's slots among them); a later compute call binds the device again */
const char *ffhip_strerror(int code);
/* The FFHIP_* environment switches (A/B knobs of tests/tools, diagnostics; none is needed in production) are read ONCE per
 * process, at first use.  A host that changes one in a live process calls this to have them read again. */
void ffhip_reload_env(void);
/* Test hook (no device needed): what the library holds for the switch `name` -- copied into dst[0..cap), full length returned,
 * -1 when unset.  Values are kept whole whatever their length (FFHIP_RCCL_LIB is a path). */
long ffhip_env_value_test(const char *name, char *dst, size_t cap);
/* Diagnostics, a test hook: sets every byte of what the library keeps between calls for (current device, `stream`) to the low byte of `value`,
 * so that a test can show that no call's output depends on what an earlier call left there.  With no call of the library in flight on `stream`
 * (and, for the slots and records below, none of the calling thread's at all): waits for `stream` and for the events behind the last copies out
 * of its pinned staging, then fills, over their WHOLE capacity (the headroom behind what the last call used included),
 *   - every device scratch buffer and every pinned buffer of (current device, stream);
 *   - the calling thread's slots of the current device, every kind kept under their streams, the front end's included (pinned and device
 *     planes and tables, pixels; the device Huffman decoder's staging and sync arrays), each after its own stream has drained;
 *   - the calling thread's header records of ffhip_jpeg_entropy_batch_gpu;
 * and waits again.  bytes[0], bytes[1]: device and host bytes written.  kinds[0..cap): the scratch kinds (the library's internal numbering,
 * ascending) that had a device or a pinned buffer; the return value is their count, whatever cap is.
 * NOT touched, being state and not scratch: the pinned word of the stream's VP8 retry record, the process-wide async error word, every event
 * and stream, the HEVC tile guard (its parity and events).
 * One kind keeps content a later call needs: the luma column ffhip_vp8_predict_loopfilter saves for the repeat by ffhip_stream_sync.  The hook
 * fills it like the others and drops the host-side mark that says it is valid (the record is disarmed: there is nothing left to repeat once
 * the stream has drained clean); while a report of that call is still waiting to be collected it fills nothing and returns FFHIP_EIO --
 * call ffhip_stream_sync first.
 * And one diagnostic reads scratch of an earlier call: ffhip_debug_hevc_plan_result, the device planner's verdict of the calling thread's last
 * ffhip_hevc_intra_recon.  Where that verdict lies in `stream`'s scratch the hook drops the thread's record of it: the diagnostic answers
 * FFHIP_EINVAL, as before the first call, until the thread's next device-planned call.
 * FFHIP_EINVAL: bytes NULL, cap < 0, or kinds NULL with cap > 0 (checked first); FFHIP_ENODEV: no device. */
int ffhip_debug_scratch_fill(void *stream, int value, uint64_t bytes[2], int *kinds, int cap);
/* "gfx950" etc. of the bound device, "" if none. */
const char *ffhip_arch_name(void);

/* Device memory / stream / event helpers so that a pure-C host (the reference is
 * C11) can drive the batched API without linking the HIP runtime itself. */
void *ffhip_malloc(size_t bytes);
void ffhip_free(void *dptr);
int ffhip_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int ffhip_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int ffhip_memset(void *dst, int value, size_t bytes, void *stream);
void *ffhip_stream_create(void);
void ffhip_stream_destroy(void *stream); /* waits for what `stream` holds, then frees the library's state of it (scratch, staging, VP8
                                            retry record, HEVC tile guard) with it */
int ffhip_stream_sync(void *stream); /* NULL = the default stream; FFHIP_EIO also if a dependency-scheduled
                                         kernel (VP8 predict / loop filter, HEVC intra) reported an abort;
                                         FFHIP_RETRIED (> 0) when a side-by-side VP8 call was repeated, see there */
void *ffhip_event_create(void);
void ffhip_event_destroy(void *event);
int ffhip_event_record(void *event, void *stream);
/* milliseconds between two recorded events (synchronises on `stop`); <0 on error */
float ffhip_event_elapsed_ms(void *start, void *stop);

/* ------------------------------------------- (1) accelerator registry seam */

/* New member of `enum simd_type` (arch/accl.h:13-18 uses 1, 2, 25, 26). */
#define GPU_TYPE_HIP 27

/* Layout-compatible with `struct accl_ops` (arch/accl.h:20-25) on LP64:
 * fn ptrs @0,@8; type @16; TAILQ_ENTRY{tqe_next @24, tqe_prev @32}; sizeof 40. */
struct ffhip_accl_ops {
    void (*idct_4x4)(int16_t *in, int bitdepth); /* VP8 4x4, == idct_4x4_16 (utils/idct.c:100-151) */
    void (*idct_8x8)(int16_t *in, int bitdepth); /* JPEG 8x8, == idct_8x8_16 (utils/idct.c:512-534) */
    int type;                                    /* GPU_TYPE_HIP */
    struct {
        struct ffhip_accl_ops *tqe_next;
        struct ffhip_accl_ops **tqe_prev;
    } next;
};

/* Same protocol as x86_sse2_init / opcl_amd_init / vulkan_init (arch/accl.c:21-35):
 * on success registers the static ops with accl_ops_register() when that symbol
 * exists in the process (i.e. libffpic is loaded); registers nothing when no
 * gfx950 device can be initialised.  hip_accl_uninit mirrors opcl_amd_uninit. */
void hip_accl_init(void);
void hip_accl_uninit(void);
/* The ops struct itself, or NULL when no device could be initialised. */
struct ffhip_accl_ops *ffhip_accl_ops_get(void);

/* ------------------------------------------------ (2) built-in op tables   */

/* Layout-compatible with `struct dct_ops` (utils/idct.h:14-21). */
struct ffhip_dct_ops {
    int bitdepth;
    void (*idct_4x4)(void *in, int bitdepth);
    void (*idct_8x8)(void *in, int bitdepth);
    void (*fdct_4x4)(void *in); /* NULL: encoder side, out of scope */
    void (*fdct_8x8)(void *in); /* NULL */
};
/* Layout-compatible with `struct cs_ops` (utils/colorspace.h:29-33). */
struct ffhip_cs_ops {
    void (*YUV_to_BGRA32)(uint8_t *dst, int pitch, void *Y, void *U, void *V, int vertical,
                          int horizontal);
    void (*YUV420_to_BGRA32)(uint8_t *dst, int pitch, void *Y, void *U, void *V); /* NULL as in the reference */
};
/* Replacements for get_dct_ops(16) / get_cs_ops(16) (utils/idct.c:829-832,
 * utils/colorspace.c:788-791).  Only the 16-bit tables exist (that is what
 * format/jpg.c:467-468 asks for); NULL for other depths or without a device. */
const struct ffhip_dct_ops *ffhip_get_dct_ops(int component_bits);
const struct ffhip_cs_ops *ffhip_get_cs_ops(int component_bits);
/* HEVC DST-VII 4x4, same signature and rounding as idct_4x4_hevc (utils/idct.h:25,
 * utils/idct.c:36-55).  Kept as its own entry: the reference back-ends overloaded
 * accl_ops.idct_4x4 with three different transforms.
 * Every block operation of (1) and (2) and this one -- copy in, one launch, copy out, synchronous -- goes through ONE small device staging
 * buffer: calls from several host threads are serialised inside the library, a whole operation at a time ("Threads and streams" above). */
void ffhip_idct_4x4_hevc(const int16_t *in, int16_t *out, int bitdepth, bool epp);

/* ------------------------------------------ (3) batched device-resident API */

/* One batch = n_images pictures of identical geometry.  Coefficient planes are
 * what the entropy decoder of format/jpg.c produces per data unit
 * (decode_data_unit, jpg.c:521-539): quantised, natural order, int16, 64 per
 * block; blocks of a component are in MCU order,
 *     block index = mcu * (h_c * v_c) + vi * h_c + hi,   mcu = my * mcu_cols + mx
 * the per-MCU scratch order the reference feeds to idct_8x8 / YUV_to_BGRA32
 * (jpg.c:545-547, colorspace.c:148).  Chroma is one block per MCU (the
 * reference's colour converter supports nothing else, colorspace.c:149-150).
 * Image i starts at plane + i * blocks_per_image_c * 64. */
typedef struct ffhip_jpeg_geom {
    int32_t mcu_cols, mcu_rows; /* MCUs per row / column                     */
    int32_t ncomp;              /* 1 (grey: U = V = zeros, jpg.c:501,552) or 3 */
    int32_t h, v;               /* luma sampling factors, h*v <= 4 data units per MCU: what the reference's MCU
                                   scratch Y[3][64*4] holds (jpg.c:501) and YUV_to_BGRA32_16bit (colorspace.c:143-150)
                                   converts -- 1x1, 2x1, 1x2, 2x2, 4x1 (4:1:1), 1x4, 3x1, 1x3 */
    int32_t qt_id[3];           /* DQT slot per component, 0..3               */
} ffhip_jpeg_geom;

/* dequant (jpg.c:247-253) + idct_8x8_16 (idct.c:512-534) + YUV_to_BGRA32_16bit
 * (colorspace.c:133-172) for a whole batch.  All pointers are DEVICE pointers.
 *   d_quant       uint16 [4][64] natural order per image (jpg.h:121-130 `dqt.tdata`),
 *                 image i at d_quant + i*quant_stride (elements); stride 0 = shared
 *   d_bgra        B,G,R,0xFF bytes; pixel (x,y) of image i at
 *                 d_bgra + i*image_stride + y*pitch + 4*x ; coded size is
 *                 (8*h*mcu_cols) x (8*v*mcu_rows); pitch >= 4*width, multiple of 16
 *   d_workspace   scratch of ffhip_jpeg_workspace_bytes(geom, n) bytes: 0 (pass NULL) for every
 *                 layout an encoder writes -- 4:2:0, 4:4:4, 4:2:2, 4:4:0, 4:1:1 (h = 4), its
 *                 transpose (v = 4) and grey run fully fused -- and non-zero only for one component
 *                 with h*v > 1 blocks per MCU and for the three-block pairs (h or v = 3)
 *   stream        hipStream_t (NULL = default stream); the call only enqueues.  Every device operand is STREAM-ORDERED: the planes, d_quant
 *                 and d_workspace are read, and d_bgra and d_workspace written, at the call's place in `stream` -- work the caller
 *                 enqueued there in front of the call may produce them, work behind it may overwrite them. */
int ffhip_jpeg_recon_batch(const ffhip_jpeg_geom *geom, int n_images, const int16_t *d_coef_y,
                           const int16_t *d_coef_u, const int16_t *d_coef_v,
                           const uint16_t *d_quant, int64_t quant_stride, uint8_t *d_bgra,
                           int64_t pitch, int64_t image_stride, void *d_workspace,
                           size_t workspace_bytes, void *stream);
size_t ffhip_jpeg_workspace_bytes(const ffhip_jpeg_geom *geom, int n_images);
/* Mixed batches: pictures that differ in size, planes, quantiser tables, output and pitch, and in layout, in one call.
 * One launch per layout class present (4:2:0, 4:4:4, 4:2:2, 4:4:0, h4v1, h1v4, grey), each picture reconstructed
 * by the same fused kernel body as ffhip_jpeg_recon_batch with n = 1 -- byte for byte the same output.  Per item:
 *   geom          its geometry; the two-pass layouts (grey with h*v > 1, h or v = 3) are refused
 *   d_coef_*      its MCU-order planes (layout as ffhip_jpeg_recon_batch, n = 1; d_coef_u / _v NULL for grey)
 *   d_quant       uint16 [4][64] natural order
 *   d_bgra        its coded-size BGRA picture; pitch >= 4 x coded width, a multiple of 16, pitch x 16 < 2^31
 *   size          the kernels index a picture by UNITS of its layout class: at most 4096 units in a picture row and 2^20 in a picture
 *                 (the exact range of their reciprocal-multiply division).  A unit is 4 MCUs of 4:2:0, h4v1 and h1v4, 8 MCUs of
 *                 4:2:2, 4:4:0 and grey, 16 MCUs of 4:4:4, a last partial unit of a row counting as one.  In MCUs:
 *                   mcu_cols <= 16384 (4:2:0, h4v1, h1v4), 32768 (4:2:2, 4:4:0, grey), 65536 (4:4:4)
 *                   ceil(mcu_cols / MCUs per unit) x mcu_rows <= 2^20: 256 MCU rows at the widest picture, 2^20 at one unit per row
 *                 (FFHIP_JPEG_STRIPS=1 halves the unit of 4:4:4, 4:2:2 and 4:4:0 and with it their mcu_cols; =2 doubles grey's)
 * Every device pointer 16-byte aligned.  `items` is a HOST array; every check is made before anything is enqueued
 * (FFHIP_EINVAL, on a machine without a device too; FFHIP_ENODEV there for good arguments).  Only enqueues on `stream`;
 * the records and the per-workgroup table are library scratch of the stream.  `items` is read before the call returns; what its
 * device pointers name (planes, d_quant, d_bgra) is stream-ordered, as for ffhip_jpeg_recon_batch.  The records go up through pinned
 * staging of the stream: a second call on a stream that has not reached the first one's upload waits on the host for that upload
 * (not for the whole stream), and a call with more items than the stream's scratch holds synchronises the stream to grow it.  The same
 * holds for every *_items call below. */
typedef struct ffhip_jpeg_item {
    ffhip_jpeg_geom geom;
    const int16_t *d_coef_y, *d_coef_u, *d_coef_v;
    const uint16_t *d_quant;
    uint8_t *d_bgra;
    int64_t pitch;
} ffhip_jpeg_item;
int ffhip_jpeg_recon_items(const ffhip_jpeg_item *items, int n, void *stream);
/* The BGRA layout this library recommends to a caller that owns its output buffer: *pitch = the reference's row pitch
 * (4 bytes x the coded width, format/jpg.c:484-486) + 1024 bytes, *image_stride = pitch x coded height.  The fused kernels
 * write 16 rows of a macroblock row at once, and with rows exactly 15 360 bytes apart (a 3840-pixel row) the rate depends on
 * where the buffer landed in physical memory (5.7-5.9 or 6.2-6.6 TB/s: DESIGN.md 5); a kibibyte more per row is the one
 * pitch that never measured slower and recovers 0.15-0.26 TB/s on the slow placements.  The drop-in path keeps the
 * reference's pitch, and every entry point takes whatever pitch the caller passes. */
int ffhip_bgra_layout(const ffhip_jpeg_geom *geom, int64_t *pitch, int64_t *image_stride);

/* Same computation from HOST buffers (copies in, runs, copies out, synchronises): what a patched
 * format/jpg.c would call per picture.  The device staging is library scratch kept between calls
 * (grown on demand, released by ffhip_shutdown); calls from several host threads are serialised
 * inside the library (one picture at a time, like the reference's decode loop; "Threads and streams" above) -- a host that wants
 * pictures in flight side by side uses the device-pointer entry above with its own buffers and streams. */
int ffhip_jpeg_recon_batch_host(const ffhip_jpeg_geom *geom, int n_images, const int16_t *coef_y,
                                const int16_t *coef_u, const int16_t *coef_v,
                                const uint16_t *quant, int64_t quant_stride, uint8_t *bgra,
                                int64_t pitch, int64_t image_stride);

/* Name and timing of the dominant kernel of the last ffhip_jpeg_recon_batch call
 * geometry class, for bench.py's roofline object. */
const char *ffhip_jpeg_kernel_name(const ffhip_jpeg_geom *geom);

/* ---- planar YUV -> BGRA (WebP frame / HEVC picture colour conversion) ----
 * Same arguments as the reference functions, plus a batch dimension; all pointers are
 * DEVICE pointers, strides in samples (planes) or bytes (pitch, image_stride).
 *   ffhip_yuv420_to_bgra     == YUV420_to_BGRA32        (utils/colorspace.c:291-329; format/webp.c:1868)
 *   ffhip_yuv420_to_bgra_16  == YUV420_to_BGRA32_16bit  (utils/colorspace.c:628-669; coding/hevc.c:7260-7270)
 *   ffhip_yuv400_to_bgra_16  == YUV400_to_BGRA32_16bit  (utils/colorspace.c:715-742; coding/hevc.c:7271-7277)
 * Image i reads planes at +i*plane_stride_* and writes at d_bgra + i*image_stride.  Only enqueue; planes and d_bgra are stream-ordered.
 * Limits (FFHIP_EINVAL beyond them, checked before the device is): the block size even and >= 2; width = cols x block a multiple of 4
 * with 4 x width <= 2^31 - 1 (it has to fit `pitch`); height = rows x block <= 524280 (4:2:0) or 262140 (4:0:0), the 65535 workgroups a
 * launch has in y; y_stride >= width, uv_stride >= width / 2; pitch >= 4 x width; d_bgra, pitch and image_stride multiples of 16;
 * n_images <= 65535.  Plane strides are free: 0 converts one set of planes n_images times. */
int ffhip_yuv420_to_bgra(uint8_t *d_bgra, int pitch, const uint8_t *d_y, const uint8_t *d_u,
                         const uint8_t *d_v, int y_stride, int uv_stride, int mbrows, int mbcols,
                         int n_images, int64_t plane_stride_y, int64_t plane_stride_uv,
                         int64_t image_stride, void *stream);
int ffhip_yuv420_to_bgra_16(uint8_t *d_bgra, int pitch, const int16_t *d_y, const int16_t *d_u,
                            const int16_t *d_v, int y_stride, int uv_stride, int ctbrows, int ctbcols,
                            int ctbsize, int n_images, int64_t plane_stride_y,
                            int64_t plane_stride_uv, int64_t image_stride, void *stream);
int ffhip_yuv400_to_bgra_16(uint8_t *d_bgra, int pitch, const int16_t *d_y, int y_stride,
                            int ctbrows, int ctbcols, int ctbsize, int n_images,
                            int64_t plane_stride_y, int64_t image_stride, void *stream);

/* ---- HEIF image grid ----
 * ffhip_heif_grid_parse reads the ImageGrid item payload exactly as decode_grid_items does
 * (format/heif.c:273-298: version, flags, rows_minus_one, columns_minus_one, then 16- or 32-bit
 * big-endian output_width/height by flags & 1); host only.
 * ffhip_heif_grid_compose places rows*cols decoded BGRA tiles (tile j of the row-major `dimg`
 * list at d_tiles + j*tile_stride, tile_pitch bytes per row, all tile_w x tile_h) on the canvas
 * at (j % cols * tile_w, j / cols * tile_h), cropped to out_w x out_h.  NEW behaviour: the
 * reference decodes every tile into the same buffer (heif.c:305) and never places them.  Only enqueues; d_tiles and d_canvas are
 * stream-ordered. */
/* The picture buffer the reference's HEVC decoder allocates per slice and hands to the colour converter
 * (coding/hevc.c:7223-7236, 7258-7277): one int16 buffer of 2*size samples, Y at 0, Cb at `u_offset`, Cr at
 * `v_offset`; what ffhip_hevc_intra_recon / ffhip_yuv420_to_bgra_16 take as their plane pointers, strides and
 * ctb counts.  Host only. */
typedef struct ffhip_hevc_layout {
    int32_t height;              /* pic_height_in_luma_samples rounded up to 4                      */
    int32_t y_stride, uv_stride; /* width rounded up to 4; half of it                               */
    int64_t size;                /* height * y_stride: samples of the luma plane                    */
    int64_t u_offset, v_offset;  /* size and size * 3 / 2 (samples)                                 */
    int32_t pitch;               /* BGRA row bytes: ((y_stride * 32 + 31) >> 5) << 2                */
    int32_t ctbrows, ctbcols;    /* divceil(height, ctb), divceil(width, ctb)                       */
} ffhip_hevc_layout;
int ffhip_hevc_picture_layout(int pic_width, int pic_height, int ctb_log2, ffhip_hevc_layout *out);

typedef struct ffhip_heif_grid {
    uint8_t version, flags;
    uint16_t rows, cols;
    uint32_t output_width, output_height;
} ffhip_heif_grid;
int ffhip_heif_grid_parse(const uint8_t *item, size_t length, ffhip_heif_grid *out);
int ffhip_heif_grid_compose(uint8_t *d_canvas, int64_t canvas_pitch, int out_w, int out_h,
                            const uint8_t *d_tiles, int64_t tile_pitch, int64_t tile_stride,
                            int tile_w, int tile_h, int rows, int cols, void *stream);

/* ---- VP8 (WebP lossy) residual stage, batched over macroblocks ----
 * Replaces, for n_mb macroblocks at once, what vp8_decode_residual_block does between
 * the token parse and the predictor (format/webp.c:1147-1196): dequantisation (the
 * `absValue * quant` int16 store of webp.c:1061), IWHT_long / IWHT_fast of the Y2 block
 * (webp.c:1067-1106) and idct_4x4_16 (utils/idct.c:100-151) of every block that has
 * more than one token or a non-zero DC (webp.c:1172,1188).  DEVICE pointers:
 *   d_levels   int16 [n_mb][25][16]  quantised levels at their raster position (zig-zag
 *              placement done); blocks 0-15 Y, 16-19 U, 20-23 V, 24 Y2
 *   d_mbinfo   uint8 [n_mb][32]      [0..24] token count per block (the return value of
 *              vp8_get_coefficients), [25] 1 if intra_y_mode != B_PRED (has Y2),
 *              [26] segment id (0..3)
 *   d_quant    uint16 [4][8]         per segment y1_dc,y1_ac,y2_dc,y2_ac,uv_dc,uv_ac,0,0
 *              (struct WEBP_decoder, format/webp.h:276-287)
 *   d_residual int16 [n_mb][384]     the `coeffs` array vp8_prerdict_mb consumes
 * d_levels and d_residual 16-byte aligned, d_mbinfo and d_quant 4-byte aligned. */
int ffhip_vp8_residual_batch(long long n_mb, const int16_t *d_levels, const uint8_t *d_mbinfo,
                             const uint16_t *d_quant, int16_t *d_residual, void *stream);

/* ---- VP8 in-loop deblocking filter for batches of key frames ----
 * The second MB loop of vp8_decode (format/webp.c:1856-1866): loopfilter() (webp.c:1686-1752)
 * with its simple and normal filters (webp.c:1480-1684) on the 8-bit Y/U/V planes that
 * ffhip_vp8_predict_recon wrote, before ffhip_yuv420_to_bgra.
 *   filter_type  0 none, 1 simple, 2 normal  (webp.c:1852-1853)
 *   d_modes      the same [n_images][n_mb][20] records; [0] intra_y_mode, [18] segment_id
 *   d_filters    uint8 [4 segments][2 (i16x16, i4x4)][3] = sub_limit, inter_limit, hev_thresh
 *                (struct vp8_filter as calculate_filter_control_parameter leaves it,
 *                webp.c:1756-1803, format/webp.h:289-293)
 * Only enqueues (the row form; FFHIP_VP8_LF_MODE=levels synchronises).  d_modes, d_filters and the planes, which are filtered in place,
 * are all stream-ordered: there is no host copy of the modes here, nothing of them is looked at when the call is made. */
/* The frame-header fields calculate_filter_control_parameter (format/webp.c:1756-1803) reads, as the reference's
 * header parser leaves them (format/webp.h:160-230), and the derivation itself on the host: the per-segment
 * {sub_limit, inter_limit, hev_thresh} triples ffhip_vp8_loopfilter takes as d_filters, and the filter_type
 * argument (0 none, 1 simple, 2 normal; webp.c:1757-1759, 1852-1853). */
typedef struct ffhip_vp8_filter_header {
    uint8_t filter_type;          /* frame header bit: 1 = simple filter, 0 = normal                    */
    uint8_t loop_filter_level;    /* 0..63, 0 = no filtering                                            */
    uint8_t sharpness_level;      /* 0..7                                                               */
    uint8_t segmentation_enabled; /* segmentation.segmentation_enabled                                  */
    uint8_t segment_feature_mode; /* 1: lf_update_value is absolute, 0: a delta to loop_filter_level    */
    int8_t lf_update_value[4];    /* segmentation.lf[s].lf_update_value                                 */
    uint8_t loop_filter_adj_enable;
    int8_t mode_ref_lf_delta0;    /* mb_lf_adjustments.mode_ref_lf_delta_update[0] (intra frame)        */
    int8_t mb_mode_delta0;        /* mb_lf_adjustments.mb_mode_delta_update[0] (B_PRED macroblocks)     */
    uint8_t nbr_partitions;       /* 1, 2, 4 or 8: the reference derives the triples inside its loop over the DCT
                                     PARTITIONS (webp.c:1905-1915), so only segments 0 .. nbr_partitions-1 get any; the
                                     others keep zeros = "no filtering" (a reference defect, kept; its write past
                                     filters[3] with 8 partitions is not reproduced)                            */
} ffhip_vp8_filter_header;
/* host only; filters = uint8 [4 segments][2 (i16x16, i4x4)][3], zeroed first like the reference's calloc'ed decoder */
int ffhip_vp8_filter_params(const ffhip_vp8_filter_header *hdr, uint8_t *filters /* [4][2][3] */, int *filter_type);
int ffhip_vp8_loopfilter(int mbcols, int mbrows, int n_images, int filter_type, const uint8_t *d_modes,
                         const uint8_t *d_filters, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                         int64_t plane_stride_y, int64_t plane_stride_uv, void *stream);
/* ffhip_vp8_predict_recon followed by ffhip_vp8_loopfilter as ONE call (the frame loop of format/webp.c:1833-1866: predict
 * every macroblock, then filter the frame): same arguments, same bytes.  The two row kernels run side by side -- the filter
 * on a stream of the library's own, forked from and joined back into `stream` -- with the filter's rows following the
 * prediction's through its per-row progress counters (a macroblock is filtered once the prediction has finished its right
 * neighbour in the row below: the prediction reads reconstructed, not filtered, samples), so the two dependency chains
 * overlap instead of adding up.  filter_type 0 = prediction only.  FFHIP_VP8_FUSE=0: one after the other.
 * The call is REPEATED by ffhip_stream_sync when it could not finish (batches of up to 2^17 macroblocks): on a device shared with other
 * work one of the two kernels can be kept from becoming resident next to the other, and a bounded wait then runs out.  The two kernels report
 * that in a pinned word of the CALL's own (nobody else's abort sets the retry off); the library keeps a copy of the one thing of the planes'
 * former contents the prediction reads (their last luma column, for the wrapped H_PRED read of predict.c:346-353) and of the call's arguments;
 * ffhip_stream_sync on `stream` then restores that column, runs prediction and filter one after the other, waits, and returns FFHIP_RETRIED
 * (> 0) with the bytes of an undisturbed call in the planes -- or FFHIP_EIO when the repeat failed too, or when the call is no longer the last
 * VP8 prediction / filter call enqueued on `stream`.  FFHIP_RETRIED is not FFHIP_OK on purpose: whatever the CALLER enqueued on `stream` behind
 * the call (a copy, a kernel of its own, ffhip_yuv420_to_bgra) has already consumed the planes of the aborted run and must be enqueued again;
 * the library knows this only of its own stages (ffhip_vp8_decode_frames repeats its colour conversion as part of the retry, and still says
 * FFHIP_RETRIED for the sake of what the caller put behind IT).  Contract: the call's inputs (d_modes, d_residual, d_resmap, d_filters) and
 * planes stay valid and unchanged until ffhip_stream_sync(stream) has returned.  FFHIP_VP8_NO_RETRY=1: FFHIP_EIO, planes unspecified, as
 * before round 4. */
int ffhip_vp8_predict_loopfilter(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes,
                                 const int16_t *d_residual, int64_t residual_stride, const int32_t *d_resmap,
                                 int filter_type, const uint8_t *d_filters, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                                 int64_t plane_stride_y, int64_t plane_stride_uv, void *stream);

/* ---- HEVC residual stage, batched over transform units of one size ----
 * For n_tu TUs of size nTbS x nTbS (4, 8, 16 or 32): scale_transform_coefficients
 * (coding/hevc.c:3743-3816) followed by transform_scaled_coeffients (hevc.c:3888-3956,
 * 1-D kernels of hevc.c:3819-3885), i.e. the non-bypass branch of scale_and_transform
 * (hevc.c:4224-4240); the bypass and transform-skip branches (hevc.c:4209-4236) are
 * selected per TU.  DEVICE pointers:
 *   d_level    int16 [n_tu][nTbS*nTbS]  TransCoeffLevel, row-major x + y*nTbS (the layout
 *              of the reference's d[] / r[]; its TransCoeffLevel[cIdx][x][y] is x-major)
 *   d_tuinfo   uint8 [n_tu][4]   [0] qP, [1] flags: 1 = luma intra 4x4 -> idct_4x4_hevc
 *              (DST-VII, utils/idct.c:36-55), 2 = transform_skip_flag, 4 = cu_transquant_bypass,
 *              8 = rotateCoeffs; [2] scaling matrixId (0..5); [3] 0
 *   d_scaling  uint8 [6][nTbS*nTbS] ScalingFactor[sizeId][matrixId] row-major, or NULL for
 *              scaling_list_enabled_flag == 0 (m = 16)
 *   bitdepth   BitDepthY or BitDepthC of the component the TUs belong to; epp =
 *              extended_precision_processing_flag
 *   d_residual int16 [n_tu][nTbS*nTbS]  r[] as construct_pic_pior_to_filtering consumes it
 * Two rules here are the reference's and not H.265's, on conformant streams too (tests/hevc_spec.py names them, DESIGN.md 4.23
 * measures them): the 4x4 DST rounds with `shift - 1` in both passes where the standard has 1 << (shift - 1)
 * (dst_round_is_shift_minus_1), and a transform-skipped block is d << tsShift without the bdShift step of 8.6.2
 * (ts_without_bdshift).
 * Only enqueues; d_level, d_tuinfo, d_scaling and d_residual are stream-ordered. */
int ffhip_hevc_residual_batch(int nTbS, long long n_tu, const int16_t *d_level, const uint8_t *d_tuinfo,
                              const uint8_t *d_scaling, int bitdepth, int epp, int16_t *d_residual,
                              void *stream);

/* ---- VP8 intra prediction + residual add for batches of key frames ----
 * What vp8_prerdict_mb does for every macroblock of vp8_decode's loop (format/webp.c:1833-1851):
 * pred_luma + pred_chrome (format/predict.c:426-645) with the residual of
 * ffhip_vp8_residual_batch, written into 8-bit Y/U/V planes of stride 16*mbcols / 8*mbcols.
 *   h_modes / d_modes  the SAME uint8 [n_images][mbrows*mbcols][20] records on the host (used
 *                      to schedule the dependency wavefronts) and on the device:
 *                      [0] intra_y_mode (0 DC, 1 TM, 2 V, 3 H, 4 B_PRED), [1] intra_uv_mode,
 *                      [2..17] imodes[16] (4x4 modes 0..9), [18..19] 0  (format/webp.h:243-256).
 *                      A y / uv mode out of range -- or, in a B_PRED record, a 4x4 mode above 9 (the
 *                      reference indexes a table of ten predictors with it) -- is FFHIP_EINVAL: from this call for batches of up
 *                      to 2^17 macroblocks (checked on the host copy), for larger ones from the next
 *                      ffhip_stream_sync (checked by a kernel in front of the prediction: the planes
 *                      are then left untouched)
 *   d_residual         int16 [n_images][.][384], image i at + i*residual_stride (elements)
 *   d_resmap           int32 [n_images][n_mb] residual row used by each macroblock, or NULL for
 *                      the identity; the reference keeps the PREVIOUS macroblock's coefficients
 *                      when mb_skip_coeff is set (webp.c:1207-1223) -- map skipped MBs there
 *   d_y/d_u/d_v        planes, image i at + i*plane_stride_*; their initial contents and the
 *                      bytes before them matter exactly where the reference's 16x16 V_PRED /
 *                      H_PRED read raw memory at the top row / left column (predict.c:338-353):
 *                      bytes before a plane read as 0.
 * Enqueues ONE launch on `stream`: a wave per macroblock row, rows chained through progress
 * counters inside the launch, as many waves as the device can hold at once -- the
 * frames of a batch run side by side, so throughput grows with the batch up to a few hundred frames; should a wave's bounded wait ever run out, the next
 * ffhip_stream_sync on any stream returns FFHIP_EIO.  FFHIP_VP8_PRED_MODE=levels selects the older
 * one-launch-per-wavefront-level form.  Scratch is kept per stream: calls on different streams (or
 * host threads with their own streams) may be in flight together; calls on one stream are ordered ("Threads and streams" above).
 * Operands: d_modes, d_residual, d_resmap and the planes (their former contents included) are STREAM-ORDERED -- the kernel reads them at
 * the call's place in `stream`, so work enqueued there in front of the call may produce them.  h_modes is read when the call is made
 * (the check above; nothing is scheduled from it in the row form) and must hold the records d_modes holds once `stream` reaches the call.
 * The same holds for ffhip_vp8_predict_loopfilter and ffhip_vp8_decode_frames (there also d_filters, stream-ordered). */
int ffhip_vp8_predict_recon(int mbcols, int mbrows, int n_images, const uint8_t *h_modes,
                            const uint8_t *d_modes, const int16_t *d_residual, int64_t residual_stride,
                            const int32_t *d_resmap, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                            int64_t plane_stride_y, int64_t plane_stride_uv, void *stream);

/* ---- the VP8 key-frame chain of a batch as ONE call: prediction + loop filter + colour conversion ----
 * The frame loop of vp8_decode (format/webp.c:1833-1868: vp8_prerdict_mb for every macroblock, loopfilter for every
 * macroblock, YUV420_to_BGRA32) with the residual of ffhip_vp8_residual_batch; the same bytes as
 * ffhip_vp8_predict_loopfilter on zero-initialised planes followed by ffhip_yuv420_to_bgra.  Arguments as there:
 *   h_modes / d_modes, d_residual, residual_stride, d_resmap   as ffhip_vp8_predict_recon (h_modes may be NULL for
 *                      batches of more than 2^17 macroblocks: those are checked on the device)
 *   filter_type, d_filters                                      as ffhip_vp8_loopfilter
 *   d_bgra, pitch, image_stride                                 as ffhip_yuv420_to_bgra: 16*mbrows rows of 16*mbcols pixels
 *   d_y / d_u / d_v    NULL, or planes (stride 16*mbcols / 8*mbcols, image i at + i*plane_stride_*) that receive the
 *                      filtered samples as well.  The planes are OUTPUTS only here: where the reference's 16x16 H_PRED reads
 *                      raw memory left of a row's first pixel (predict.c:346-353) it finds the last pixel of the row above
 *                      and, below it, samples not reconstructed yet -- 0, as in the freshly allocated planes of vp8_decode.
 * Batches of at least half as many frames as the device has CUs run as ONE kernel in which a workgroup owns a frame, its
 * waves the frame's macroblock rows, and a wave predicts, filters and converts its macroblock before anything is stored
 * (every pixel is written once, as BGRA); smaller batches run the three stages (row kernels, then the colour
 * kernel: a single frame's critical path is shorter there).  FFHIP_VP8_FRAMES=fused|rows forces either.
 * Stream order: as ffhip_vp8_predict_recon.  The row form is a side-by-side call and has ffhip_vp8_predict_loopfilter's contract (inputs
 * and planes unchanged until ffhip_stream_sync has returned, FFHIP_RETRIED); the frame kernel is never repeated, and work enqueued behind
 * it may overwrite its inputs.  A caller that does not know the form (ffhip_vp8_decode_frames_form) keeps to the row form's rule. */
/* which form ffhip_vp8_decode_frames takes for a batch of n_images on the current device: 1 the frame kernel, 0 the row kernels + colour kernel
 * (half the device's compute units and more take the frame kernel; FFHIP_VP8_FRAMES / FFHIP_VP8_FRAMES_MIN move that) */
int ffhip_vp8_decode_frames_form(int n_images);
int ffhip_vp8_decode_frames(int mbcols, int mbrows, int n_images, const uint8_t *h_modes, const uint8_t *d_modes,
                            const int16_t *d_residual, int64_t residual_stride, const int32_t *d_resmap, int filter_type,
                            const uint8_t *d_filters, uint8_t *d_bgra, int pitch, int64_t image_stride, uint8_t *d_y,
                            uint8_t *d_u, uint8_t *d_v, int64_t plane_stride_y, int64_t plane_stride_uv, void *stream);
/* Mixed batches: key frames that differ in size, quantisers, loop filter, output and pitch, in one call.  Each item gets the
 * BGRA bytes of ffhip_vp8_residual_batch (levels form only) followed by ffhip_vp8_decode_frames(n_images = 1) on that item
 * alone.  Per item:
 *   mbcols, mbrows   its size in macroblocks (fewer than 2^23 of them)
 *   h_modes          host copy of its [n_mb][20] mode records (checked here), or NULL: checked by ONE kernel in front of the
 *                    decode for all such items; a bad record then gives FFHIP_EINVAL from the next ffhip_stream_sync and no
 *                    item's output is written
 *   d_modes          device [n_mb][20], format as ffhip_vp8_predict_recon, 4-byte aligned
 *   the residual     EITHER d_levels (16-byte aligned) + d_mbinfo (4-byte aligned) + quant (HOST values, as d_quant of
 *                    ffhip_vp8_residual_batch): the call runs the residual stage with this item's quantisers into library
 *                    scratch (768 B per macroblock) -- OR d_residual ([rows][384], 4-byte aligned; d_levels NULL)
 *   d_resmap         [n_mb] residual row of each macroblock (below n_mb), or NULL for the identity; as ffhip_vp8_predict_recon
 *   filter_type      0 none, 1 simple, 2 normal; filters: HOST values, as ffhip_vp8_filter_params leaves them
 *   d_bgra, pitch    16*mbrows rows of 16*mbcols pixels, `pitch` bytes apart: 16-byte aligned, pitch >= 64*mbcols, a
 *                    multiple of 16, pitch*16*mbrows < 2^31.  Only those pixels are written, not the pitch's padding
 * `items` is a HOST array; fewer than 2^30 macroblocks in all.  Every check is made before anything is enqueued (FFHIP_EINVAL,
 * on a machine without a device too; FFHIP_ENODEV there for good arguments).  Only enqueues on `stream`.  Always the one-kernel
 * frame form of ffhip_vp8_decode_frames (one launch per filter type and residual-map form present, frames dealt to workgroups
 * largest first): there is no row form and no FFHIP_RETRIED, so one or two frames decode with the frame kernel's latency, not
 * the row kernels'.  BGRA only (no planes).  Residual scratch, descriptor tables and line slots are library scratch of the
 * stream.  `items` (with h_modes, quant and filters) is read before the call returns; d_modes, d_levels, d_mbinfo, d_residual, d_resmap
 * and d_bgra are stream-ordered, an h_modes must hold what its d_modes holds once `stream` reaches the call. */
typedef struct ffhip_vp8_item {
    int mbcols, mbrows;
    const uint8_t *h_modes;
    const uint8_t *d_modes;
    const int16_t *d_levels;
    const uint8_t *d_mbinfo;
    uint16_t quant[4][8];
    const int16_t *d_residual;
    const int32_t *d_resmap;
    int filter_type;
    uint8_t filters[4][2][3];
    uint8_t *d_bgra;
    int64_t pitch;
} ffhip_vp8_item;
int ffhip_vp8_decode_items(const ffhip_vp8_item *items, int n, void *stream);

/* ---- lossy WebP files: the VP8 front end (container, frame header, bool decoder) in front of ffhip_vp8_decode_items ----
 * The contract is the reference's WEBP_load (format/webp.c:2002 on; WEBP_read_frame :1872-1926, read_vp8_ctl_partition :897-935,
 * vp8_decode_mb_header :1277-1450, vp8_get_coefficients :992-1064, vp8_decode_residual_block / _data :1125-1225,
 * coding/booldec.c), bit for bit on the BGRA it produces -- not RFC 6386; ffhip_vp8_bool.h lists where the two differ. */
#define FFHIP_EWEBP_LOSSLESS (-1001)    /* a VP8L chunk: these calls do not decode lossless WebP (the reference has a stub); the "lossless WebP" calls below do */
#define FFHIP_EWEBP_ANIMATION (-1002)   /* the VP8X animation flag, or an ANIM / ANMF chunk in front of the frame      */
#define FFHIP_EWEBP_INTER_FRAME (-1003) /* the frame tag says "not a key frame" (webp.c:1877-1880)                     */

/* The frame-header fields read_dequantization (format/webp.c:458-548) reads, as the reference's header parser leaves them
 * (format/webp.h:157-197), and the derivation itself on the host: the uint16 [4 segments][8] = y1_dc, y1_ac, y2_dc, y2_ac, uv_dc,
 * uv_ac, 0, 0 that ffhip_vp8_item.quant and ffhip_vp8_residual_batch's d_quant take.  As the reference HAS it:
 *   - absolute or delta is switched by update_mb_segmentation_map, not by segment_feature_mode (webp.c:518-522): map updated =
 *     the update value IS the index, map kept = it is added to y_ac_qi;
 *   - the index is a uint16_t: a negative one wraps and clamp(., 127) then gives index 127, not 0 (a delta applied to a small
 *     non-negative index still clamps to 0: that sum is an int);
 *   - without segmentation only segment 0 is derived, the others stay zero (webp.c:515);
 *   - y2_dc is doubled and capped at 132, y2_ac is x 155 / 100, floored at 8 (webp.c:527-543). */
typedef struct ffhip_vp8_quant_header {
    uint8_t y_ac_qi; /* 0..127 */
    int8_t y_dc_delta, y2_dc_delta, y2_ac_delta, uv_dc_delta, uv_ac_delta;
    uint8_t segmentation_enabled;
    uint8_t update_mb_segmentation_map;
    int8_t quantizer_update_value[4]; /* segmentation.quant[s].quantizer_update_value */
} ffhip_vp8_quant_header;
/* host only */
int ffhip_vp8_dequant_factors(const ffhip_vp8_quant_header *hdr, uint16_t *quant /* [4][8] */);

/* What the frame header of a file says: the picture, and the per-frame arguments of ffhip_vp8_item. */
typedef struct ffhip_webp_info {
    int32_t width, height;   /* what WEBP_load puts into struct pic (webp.c:2069-2076): the VP8X canvas fields when there is such a
                                chunk (read as stored, without the format's "+ 1"), otherwise the frame's size rounded UP to a
                                multiple of 4 */
    int32_t mbcols, mbrows;  /* the decoded picture is 16*mbcols x 16*mbrows */
    int32_t filter_type;     /* 0 none, 1 simple, 2 normal */
    int32_t nbr_partitions;  /* 1, 2, 4 or 8 token partitions.  (8 overflow the reference's own p[4] and bt[4] arrays, webp.h:268,
                                webp.c:1904, so there is no reference output to pin them: such files are decoded by the rule of the
                                others, and the tests hold host parser, kernels and oracle chain against each other on them.) */
    uint16_t quant[4][8];    /* ffhip_vp8_dequant_factors of quant_header */
    uint8_t filters[4][2][3]; /* ffhip_vp8_filter_params of filter_header (nbr_partitions passed through: its kept defect depends on it) */
    ffhip_vp8_quant_header quant_header;
    ffhip_vp8_filter_header filter_header;
} ffhip_webp_info;

/* Host only.  The chunk walk of WEBP_load as it is (webp.c:2016-2066): `VP8X` and `ALPH` are accepted only at the reference's
 * fixed struct sizes (size fields 10 and 1), unknown chunks are skipped by their size without the padding byte, the first `VP8 `
 * chunk ends the walk; then the key-frame tag, the start code and the 14-bit sizes.  Any of the four outputs may be NULL.
 * FFHIP_EWEBP_* for lossless, animated and inter-frame files, FFHIP_EINVAL for anything else that is not a lossy WebP. */
int ffhip_webp_probe(const uint8_t *file, size_t len, int *width, int *height, int *mbcols, int *mbrows);

/* Host only: one file -> what ffhip_vp8_decode_items takes, into CALLER memory sized from the probe (n_mb = mbcols * mbrows):
 *   modes   uint8 [n_mb][20]      the mode records ([18] = segment id)
 *   levels  int16 [n_mb][25][16]  mbinfo uint8 [n_mb][32]   as ffhip_vp8_residual_batch reads them
 *   resmap  int32 [n_mb]          the residual row each macroblock shows: its own, or for a macroblock with mb_skip_coeff the
 *                                 last CODED macroblock's in decode order, across row ends too -- the reference leaves the previous
 *                                 coefficients in place (webp.c:1207-1223, the array lives outside both loops, :1830).  A skipped
 *                                 macroblock in front of every coded one reads an uninitialised stack array in the reference: it
 *                                 gets its own (all-zero) row here, and that case is UNPINNED.
 *   n_mb_cap                      macroblocks the four arrays have room for (FFHIP_EINVAL when the file has more)
 * info receives the header.  Row y takes its tokens from partition y & (nbr_partitions - 1) (webp.c:1836); the `top` contexts carry
 * across rows, `left` starts at zero in every row; a skipped macroblock clears contexts 1-8 always and context 0 only when it is
 * not B_PRED (webp.c:1213-1221).  A partition that is asked for a byte beyond its length is FFHIP_EINVAL ("truncated": the
 * reference reads one byte of heap there and then exits, utils/bitstream.c:115-120), and no read goes outside [file, file + len).
 * That verdict also meets files libwebp decodes: with segmentation off the reference still reads a segment id per macroblock, with
 * probabilities 0 (webp.c:393, 1291-1294), and in a first partition that ends right behind the last macroblock header -- flat and
 * tiny pictures -- those reads use up bits the encoder never wrote.  It is the reference's rule, kept and named.
 * The last partition ends with the FILE in the reference (webp.c:452-454); here it ends with the `VP8 ` chunk where that is
 * shorter, so bytes of a chunk behind the frame are never taken for tokens. */
typedef struct ffhip_webp_parsed {
    uint8_t *modes;
    int16_t *levels;
    uint8_t *mbinfo;
    int32_t *resmap;
    int64_t n_mb_cap;
    ffhip_webp_info info;
} ffhip_webp_parsed;
int ffhip_webp_parse(const uint8_t *file, size_t len, ffhip_webp_parsed *out);
/* n files over n_threads host threads; status[i] = each file's code, returns the first failure */
int ffhip_webp_parse_batch(const uint8_t *const *files, const size_t *lens, int n, int n_threads, ffhip_webp_parsed *outs, int *status);
/* The same arrays from the DEVICE front end (kernel A: macroblock headers, kernel B: token partitions), copied back into the
 * caller's HOST arrays: lets a test say which half differs from ffhip_webp_parse.  No fall-back: a file the kernels refuse gets
 * their verdict (FFHIP_EINVAL).  Synchronises `stream`. */
int ffhip_webp_parse_device(const uint8_t *const *files, const size_t *lens, int n, ffhip_webp_parsed *outs, int *status, void *stream);

/* Files in, pixels on the device: n lossy WebP files of any sizes in one call, picture i at d_bgra[i] with pitch[i] -- 16*mbrows
 * rows of 16*mbcols pixels as ffhip_webp_probe reports them (the caller probes, then allocates; alignment and pitch as for
 * ffhip_vp8_item).  Host threads parse only the frame header (a few hundred bool decodes, up to prob_skip_false) and derive
 * quantisers and filters; the file bytes go up through pinned staging; kernel A reads the macroblock headers of the first partition
 * into mode records, skip flags and the residual map, kernel B the token partitions into levels and token counts, and
 * ffhip_vp8_decode_items (device-side mode check, no FFHIP_RETRIED) does the rest.  Arithmetic decoding is serial per stream, so a
 * frame is ONE lane's work in either kernel -- a lone lane issues as fast as a full wave, so every frame gets a wave of its own
 * until a part of the batch has more frames than the device has wave slots; only then do several frames share a wave.  Frames with
 * 2, 4 or 8 token partitions are walked row by row by that one lane, which holds all the decoder states: no waits between waves.
 * The batch is processed in PARTS of at most 2^23 macroblocks with the kernels and 2^19 with the host threads.  A part's arrays
 * take 856 bytes per macroblock (levels, token counts, records, maps).  Up to 1 GiB they are library scratch of the stream, kept
 * between calls like every other scratch; a larger part (from some 150 frames of 1080p; 6.7 GiB at the bound) allocates its own and
 * frees them when it is done, so this call leaves no more than 1 GiB standing.  (ffhip_vp8_decode_items behind it keeps its 768
 * bytes of residual per macroblock as that call documents.)  The kernels' parts are that large because a part costs what its
 * LARGEST frame costs one lane, however many frames it holds; the host threads' arrays are mirrored in pinned memory, hence 2^19.
 * FFHIP_WEBP_GPU_ENTROPY=0: n_threads host threads parse the parts instead (the loops of ffhip_webp_parse) and the arrays are
 * uploaded; =1: always the kernels; unset: the kernels for a part worth at least 32 x n_threads of its largest frame (macroblocks
 * of the part / macroblocks of its largest file), the host threads below; FFHIP_WEBP_GPU_MIN_FILES replaces that product.
 * MEASURED with n_threads = 16 on an MI355X: a lane takes 45 us per macroblock of a photograph, a host thread
 * 1.7 us -- 1, 16 and 256 copies of a 1080p stream and the mixed fixture set are faster on the host, 512 and 1 024 copies on the
 * device.  Other thread counts were NOT measured; the threshold scales with n_threads on the assumption that the host threads
 * scale linearly.  The kernels refuse only what the host parser refuses (a partition asked for a byte beyond its length; same
 * source, same lengths), so a file they refuse has its code from them and is not parsed a second time.
 * FFHIP_WEBP_PACK (frames per wave, 1..32) and FFHIP_WEBP_PART_MB (macroblocks per part, both front ends) let tests reach the
 * packed and the many-part forms with small batches.
 * info_out[i] (may be NULL) receives each file's header, status[i] its code: a damaged, truncated, lossless, animated or inter-frame
 * file gets a non-zero code and no promised output bytes, and every other file is still decoded.  Returns the first failure.
 * Every argument check is made before anything is enqueued (FFHIP_EINVAL, on a machine without a device too; FFHIP_ENODEV there
 * for good arguments).  Synchronises `stream`. */
int ffhip_webp_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                   const int64_t *pitch, ffhip_webp_info *info_out, int *status, void *stream);

/* Diagnostics: how many parts of the calling thread's last ffhip_webp_decode_files_device / ffhip_webp_parse_device call went to the
 * kernels (out[0]) and to the host threads (out[1]). */
int ffhip_debug_webp_last_parts(int out[2]);

/* ---- lossy WebP, the second pixel rule: the pixels libwebp gives (opt-in) ----
 * The calls above give the reference's WEBP_load bit for bit, which is not what libwebp, PIL, torchvision or a browser show (DESIGN.md
 * 4.19: twenty named deviations from RFC 6386, one in five valid files refused).  With FFHIP_WEBP_PIXELS_LIBWEBP in `flags` the _ex calls
 * below decode RFC 6386 as libwebp does, sample for sample, and finish with libwebp's fancy upsampler and colour step:
 *   - RIFF chunks are walked with the padding byte of an odd-sized one; the picture is the frame tag's 14-bit width x height, and
 *     mbcols = (width + 15) >> 4, mbrows likewise: 50 x 37 stays 50 x 37 (the default rule says 52 x 40);
 *   - a segment id is read only when segmentation and the map update are on, an unset tree probability is 255, cat6 extra bits are not
 *     wrapped, a skipped macroblock has a zero residual (resmap is the identity);
 *   - quantisers: segment_feature_mode says absolute or delta, a negative index clamps to 0, the cap of 132 sits on the chroma DC factor;
 *     filter parameters: all four segments, one clamp behind the deltas.  ffhip_webp_info.quant and .filters hold these values; the two
 *     header structs are filled as ever (update_mb_segmentation_map is the bit of the stream, 0 without segmentation);
 *   - residual: the int16 store of level x quantiser and of the Y2-derived DC stay (libwebp has them too), the first IDCT pass is plain
 *     int, every block with a non-zero coefficient goes through the IDCT;
 *   - prediction: 16x16 V_PRED / H_PRED take the 127 / 129 borders like every other mode; B_PRED sub-blocks 7, 11 and 15 take the four
 *     samples above-right of the MACROBLOCK; the right-most macroblock takes the last sample above it four times (127 in row 0);
 *   - loop filter, both types: inner edges for B_PRED macroblocks and for those with a non-zero dequantised coefficient;
 *   - colour: libwebp's fancy upsampler (9-3-3-1 on the chroma samples around a pixel) and its 14-bit fixed-point YUV -> RGB, with the
 *     edges taken at the DISPLAY width and height; the alpha byte is 255, as the default rule writes it.
 * Where the first IDCT pass leaves 16 bits there is no single libwebp picture: its C transform keeps int, its SIMD transforms saturate or
 * wrap at 16 bits.  The rule follows the witness, tests/vp8_spec.py with rules=SPEC, i.e. the C transform; no encoder
 * writes such a stream.  A file with an `ALPH` chunk decodes its colour; the alpha plane is ignored unless FFHIP_WEBP_ALPHA asks for it
 * ("lossy WebP, the alpha plane" below).
 * The verdicts stay: FFHIP_EWEBP_LOSSLESS / _ANIMATION / _INTER_FRAME, and FFHIP_EINVAL for a partition asked for a byte beyond its length
 * (under the rule no valid file of the libwebp corpus, tests/golden/webp_libwebp.npz, gets it).
 * flags == 0 is the plain call, bit for bit; any other bit is FFHIP_EINVAL.  Argument errors come before FFHIP_ENODEV, both before the first
 * allocation; FFHIP_WEBP_GPU_ENTROPY, FFHIP_WEBP_PACK, FFHIP_WEBP_PART_MB and FFHIP_WEBP_GPU_MIN_FILES act as in the plain calls. */
#define FFHIP_WEBP_PIXELS_LIBWEBP 0x10u
/* host only */
int ffhip_webp_probe_ex(const uint8_t *file, size_t len, unsigned flags, int *width, int *height, int *mbcols, int *mbrows);
int ffhip_webp_parse_ex(const uint8_t *file, size_t len, unsigned flags, ffhip_webp_parsed *out);
/* the device twin of ffhip_webp_parse_ex (as ffhip_webp_parse_device is ffhip_webp_parse's) */
int ffhip_webp_parse_device_ex(const uint8_t *const *files, const size_t *lens, int n, unsigned flags, ffhip_webp_parsed *outs, int *status,
                               void *stream);
/* ffhip_webp_decode_files_device under `flags` (FFHIP_WEBP_PIXELS_LIBWEBP, with it FFHIP_WEBP_ALPHA).  Buffers as there, with the _ex probe's mbcols and mbrows (pitch >= 64*mbcols, room for
 * 16*mbrows rows), so a caller switches rules without new arithmetic; under the rule only `height` rows of `width` pixels are written.
 * planes: NULL, or [n] triples of device pointers y, u, v (16*mbcols x 16*mbrows and 8*mbcols x 8*mbrows samples, strides 16*mbcols and
 * 8*mbcols, 4-byte aligned): the loop-filtered planes of each file's macroblock grid are delivered too, which lets a caller name the plane and
 * macroblock at which a decode differs.  planes with flags == 0 is FFHIP_EINVAL.  Under the rule the back half is three launches per part and
 * filter type: the residual instance (which also leaves, in byte [19] of each mode record of the call's scratch, whether the macroblock has a
 * non-zero dequantised coefficient), k_vp8_frames_items' libwebp instances, which write planes and no pixels, and k_vp8_upsample_color:
 * libwebp's upsampler reads the chroma row BELOW a pixel row, which is final only once the next macroblock row has been filtered. */
int ffhip_webp_decode_files_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                      const int64_t *pitch, uint8_t *const *planes, unsigned flags, ffhip_webp_info *info_out, int *status,
                                      void *stream);
/* Host only, no device needed: the arithmetic the kernels compile (ffhip_vp8_libwebp_body.h).
 * ffhip_vp8_libwebp_residual_mb: one macroblock's levels [25][16] (raster positions; 16 Y, 4 U, 4 V, Y2), has_y2, and its six factors
 * y1_dc, y1_ac, y2_dc, y2_ac, uv_dc, uv_ac -> residual [24][16] and *any_nz: some block has a non-zero dequantised coefficient.
 * ffhip_webp_libwebp_color: planes y (stride ys) and u, v (stride uvs; (width + 1) / 2 x (height + 1) / 2 samples) -> width x height BGRA
 * pixels, `pitch` bytes a row, alpha 255. */
int ffhip_vp8_libwebp_residual_mb(const int16_t *levels, int has_y2, const uint16_t *factors, int16_t *residual, int *any_nz);
int ffhip_webp_libwebp_color(const uint8_t *y, int64_t ys, const uint8_t *u, const uint8_t *v, int64_t uvs, int width, int height,
                             uint8_t *bgra, int64_t pitch);
/* Diagnostics (tests/tools/bench_webp_pixels.py measures the rule's back half and its colour kernel alone with them; both only enqueue):
 * ffhip_vp8_decode_items under the libwebp rule -- levels items without a residual map, display[i] the picture's size inside its macroblock
 * grid; the call WRITES byte [19] of every record of d_modes -- and k_vp8_upsample_color on planes laid out as ffhip_yuv420_to_bgra takes
 * them (4-byte aligned, strides multiples of 4). */
struct ffhip_size; /* (defined with the resize calls below) */
int ffhip_debug_vp8_decode_items_libwebp(const ffhip_vp8_item *items, int n, const struct ffhip_size *display, void *stream);
int ffhip_debug_vp8_upsample_color(const uint8_t *d_y, const uint8_t *d_u, const uint8_t *d_v, int ys, int uvs, int width, int height,
                                   int n_images, int64_t plane_stride_y, int64_t plane_stride_uv, uint8_t *d_bgra, int64_t pitch,
                                   int64_t image_stride, void *stream);

/* ---- lossy WebP, the alpha plane (opt-in; ffhip_webp_alpha.c, ffhip_webp_alpha_body.h, ffhip_webp_alpha_gpu.hip) ----
 * FFHIP_WEBP_ALPHA is accepted together with FFHIP_WEBP_PIXELS_LIBWEBP by ffhip_webp_decode_files_device_ex and by no other call: without
 * the libwebp bit, and on the probe, parse, parse_device and tensor calls, it is FFHIP_EINVAL as any unknown bit is (a tensor call that
 * keeps alpha is ffhip_webp_decode_files_tensor_alpha, which sets the bit underneath itself).  Without the bit every call keeps its bytes and its verdicts.  With it, a file that has a VP8X chunk with the
 * alpha flag (0x10) set and an ALPH chunk between it and the `VP8 ` chunk gets that plane in byte 3 of its width x height pixels, sample
 * for sample what PIL's Image.open(f).convert("RGBA") gives (libwebp 1.6.0); the colour bytes are those of the unflagged call (no
 * premultiplication).  Every other file is exactly what the unflagged call gives: alpha 255, the same status.  The rule, each line held
 * against PIL (tests/test_webp_alpha_spec.py):
 *   - the chunk walk is the libwebp rule's, padding byte included; the frame tag's width x height is the plane's size;
 *   - ALPH payload byte 0: reserved (2 bits) | pre-processing (2) | filter (2) | compression (2), bits 7..0.  Compression 2 or 3,
 *     pre-processing 2 or 3 and a reserved bit set are refused, an empty payload too; pre-processing 1 changes nothing in the decode;
 *   - compression 0: width x height bytes behind the header byte; fewer are refused, more are ignored;
 *   - compression 1: a VP8L stream without signature and header that starts at the first transform bit ("lossless WebP" below, every
 *     line of it), width and height the picture's; the stored sample is the green byte of each decoded ARGB word;
 *   - filters, sums modulo 256 on the FINISHED plane: 0 none; row 0, or filter 1, the sample to the left, for x = 0 the one above and 0
 *     at (0, 0); filter 2 the sample above; filter 3 clip255(left + above - above left); under 2 and 3 column 0 takes the sample above;
 *   - a stream that asks for bits behind its chunk's end (they read as 0) is refused, as a VP8L file's is -- settled on truncated copies
 *     with ONE exception: libwebp decodes a stream whose only transform is colour indexing, without a colour cache and with one-symbol
 *     red, blue and alpha codes in every group, by a loop of its own, and that loop accepts the image when the LAST token (literal or
 *     copy) is the one that ran over the end.  Such a stream is accepted here too, and the token is what libwebp's reader makes of it:
 *     that reader keeps the chunk's last 8 bytes in a 64-bit window, so a symbol that straddles the end gets zeros and a token that
 *     begins exactly at the end reads those 8 bytes again (ffhip_vp8l.c, tail_*); a stream of fewer than 8 bytes reads zeros.
 * Named deviations, beside the one that the VP8X canvas is not compared with the frame tag: PIL refuses an ALPH chunk in a file without
 * VP8X, an ALPH chunk behind the `VP8 ` chunk, and a second ALPH chunk; here the first two files stay opaque and of several ALPH chunks
 * the first counts -- the flag never makes a container check stricter.  With the VP8X alpha flag clear PIL, too, ignores the chunk.
 * A file whose ALPH chunk is refused gets FFHIP_EINVAL in status[i] and no promised bytes; every other file is delivered; the call returns
 * the first failure.  The stage runs behind the colour, in parts of its own (1 GiB of staging and scratch; FFHIP_WEBP_ALPHA_PART_BYTES
 * replaces the figure): host threads copy raw planes and decode lossless planes' prefix codes into pinned staging, k_vp8l_predict and
 * k_vp8l_finish write the lossless planes into scratch pictures, k_webp_alpha_unfilter (one launch per level of 64 rows; none for
 * filter 0) undoes the filter and k_webp_alpha_merge writes byte 3.  Synchronises `stream`, as the unflagged call does. */
#define FFHIP_WEBP_ALPHA 0x20u
/* Host only, cheap: the chunk walk and the header byte.  *has_alpha 0 with FFHIP_OK for a file the flag would leave opaque (the other
 * three are 0 then); the libwebp rule's probe verdicts for a file it refuses, FFHIP_EINVAL for a refused header byte or a short raw plane. */
int ffhip_webp_alpha_probe(const uint8_t *file, size_t len, int *has_alpha, int *compression, int *filter, int *pre_processing);
/* Host only, no device needed: the whole alpha decode into width x height bytes at `alpha` (pitch >= width; the libwebp rule's probe
 * gives the size), the filter undone by the function the kernel compiles.  It is to FFHIP_WEBP_ALPHA what ffhip_vp8l_picture is to the
 * lossless file call.  FFHIP_EINVAL for everything refused above and for a file without a plane.  No read goes outside file[0 .. len). */
int ffhip_webp_alpha_plane(const uint8_t *file, size_t len, uint8_t *alpha, int64_t pitch);
/* Diagnostics, of the calling thread's last call with FFHIP_WEBP_ALPHA: files with a plane, how many of those were lossless, launches of
 * k_webp_alpha_unfilter, parts. */
int ffhip_debug_webp_alpha_last(int out[4]);
/* Diagnostics (tests/tools/bench_webp_alpha.py): milliseconds of that call's alpha stage, all its parts together -- [0] the host threads'
 * walk, copies and stream decode (wall clock), and, measured by events only while FFHIP_WEBP_ALPHA_TIMES is set (0 otherwise), [1] the
 * upload with the lossless planes' k_vp8l_predict and k_vp8l_finish, [2] k_webp_alpha_unfilter over all its levels, [3]
 * k_webp_alpha_merge. */
int ffhip_debug_webp_alpha_times(double out[4]);

/* ---- HEVC intra prediction + reconstruction for a list of transform units ----
 * decode_intra_block steps 5-10 (coding/hevc.c:4730-4790) for every TU of a picture:
 * intra_sample_prediction (hevc.c:4542-4662: neighbour gathering, reference_sample_substitution
 * :4277-4351, filtering_neighbouring_samples :4355-4426, hevc_intra_planar/DC/angular
 * format/predict.c:651-792), the optional rdpcm residual modification (hevc.c:3960-3977) and
 * construct_pic_pior_to_filtering (hevc.c:4252-4274) into int16 sample planes laid out like
 * the reference's picture (hevc.c:7225-7230).  TUs are listed in decode order; what the
 * reference derives while parsing (neighbour availability by z-scan order / slice / tile,
 * hevc.c:4570-4608) arrives here as bit masks.
 * Order contract: inside each PLANE a TU follows every TU its availability bits point at; how the planes
 * interleave is free (they never read each other here).  The reference's own order -- per coding unit the luma
 * tree, then Cb, then Cr (decode_cu_coded_intra_prediction_mode, hevc.c:5013-5180) -- is taken as it comes:
 * scheduling runs are defined on each plane's own subsequence, and a list that switches planes inside a
 * scheduling window is sorted by plane (a stable device-side copy) in front of the planner. */
typedef struct ffhip_hevc_tu {
    uint16_t x, y;       /* top-left of the TU in samples of its component plane           */
    uint8_t log2_size;   /* 2..5                                                            */
    uint8_t cidx;        /* 0 Y, 1 Cb, 2 Cr                                                 */
    uint8_t pred_mode;   /* predModeIntra: 0 planar, 1 DC, 2..34 angular                    */
    uint8_t flags;       /* FFHIP_TU_*                                                      */
    uint32_t res_offset; /* element offset of the TU's residual block in d_residual         */
    int32_t res_scale;   /* ResScaleVal of 8.6.6 (hevc.c:3494-3497: 0, +-1, +-2, +-4, +-8); used with FFHIP_TU_CCP */
    uint64_t avail_top;  /* bit k: neighbour (x+k, y-1), k = 0..2n-1, is available          */
    uint64_t avail_left; /* bit k: neighbour (x-1, y+k) is available                        */
} ffhip_hevc_tu;
#define FFHIP_TU_CORNER 0x01   /* neighbour (x-1, y-1) available                             */
#define FFHIP_TU_RESIDUAL 0x02 /* numSigCoeff != 0: add the residual block (hevc.c:4737)      */
#define FFHIP_TU_FILTER 0x04   /* 8.4.4.2.3 applies: intra_smoothing_disabled_flag == 0 and
                                  (cIdx == 0 or ChromaArrayType == 3)  (hevc.c:4629-4633)    */
#define FFHIP_TU_STRONG 0x08   /* sps strong_intra_smoothing_enabled_flag                    */
#define FFHIP_TU_NO_BF 0x10    /* disableIntraBoundaryFilter (hevc.c:4642-4648)              */
#define FFHIP_TU_NO_DC_BF 0x20 /* intra_boundary_filtering_disabled_flag (DC edge filter)    */
#define FFHIP_TU_RDPCM 0x40    /* residualDpcm == 1: 8.6.5 on the residual before the add.  Horizontally the
                                  reference's rule, not H.265's: a running sum over the flattened block from index
                                  nTbS on (flag rdpcm_horizontal_runs_on of tests/hevc_spec.py) */
#define FFHIP_TU_CCP 0x80      /* 8.6.6 cross-component prediction after 8.6.5, exactly as the reference
                                  calls it (hevc.c:4750-4756): the "luma" residual it passes is the chroma
                                  block itself, so r += (res_scale * ((r << BitDepthC) >> BitDepthY)) >> 3.
                                  The reference's rule, not H.265's, where rY is the luma residual (flag
                                  ccp_reads_chroma of tests/hevc_spec.py) */
/* h_tus / d_tus: the SAME n_tus records on the host (dependency scheduling) and on the device.
 * d_residual: int16 residual blocks (row-major n*n each) as ffhip_hevc_residual_batch writes
 * them.  Planes: int16, strides in samples; d_cb/d_cr may be NULL for 4:0:0.  ONLY ENQUEUES: h_tus is validated on
 * the host (and the scheduling window chosen from it) -- record by record up to 2^17 TUs; of a larger list the host
 * looks at a sample only (every 64th stretch of 4096 records, every 256th from a million records on) and EVERY record of d_tus is checked by a kernel in front
 * of everything else: a bad record found there refuses the call through the stream (the call returns 0, nothing is
 * written, the next ffhip_stream_sync returns FFHIP_EINVAL; FFHIP_HEVC_HOST_CHECK=1 keeps the whole check on the host) --,
 * the schedule is built on the device (hand-written kernels: no library primitive) and ONE launch follows --
 * TUs grouped by 32x32 window, a wave per group, done flags between groups -- which reads the
 * planner's verdict itself: a list it refuses is decoded by one wave in decode order inside the same launch (slow,
 * exact).  A bounded wait that ever runs out surfaces as FFHIP_EIO from the next ffhip_stream_sync.
 * FFHIP_HEVC_INTRA_MODE=levels selects the older one-launch-per-dependency-level form and FFHIP_HEVC_PLAN=host the
 * host-side planner (both synchronise the stream).  Scratch is kept per stream, as for VP8.
 * Operands: d_tus, d_residual and the planes are STREAM-ORDERED -- every kernel that reads the list (validation, planner, substitution
 * table, per-pixel programs: some on a stream of the library's own, forked from `stream` behind the call's place and joined back) waits for
 * what the caller enqueued on `stream` in front of the call, and `stream` does not pass the call before the last of them has read it.  h_tus
 * is read when the call is made and must hold the records d_tus holds once `stream` reaches the call.  (ffhip_hevc_intra_recon_tiles
 * below asks MORE of d_tus: there it must be complete when the call is made.) */
/* Host only, no device needed: the group schedule ffhip_hevc_intra_recon builds for an already valid
 * list -- out_ticket[i] = ticket of the group of TU i, out_wait[i] = TUs of other groups it waits for
 * (either may be NULL), stats[4] = {groups, luma window log2 used, wait entries, TUs served from the
 * LDS tile}; window_log2 0 = the default.  FFHIP_EINVAL when no window gives a deadlock-free order. */
int ffhip_hevc_intra_plan(const ffhip_hevc_tu *h_tus, long long n_tus, int width_y, int height_y,
                          int width_c, int height_c, int window_log2, uint32_t *out_ticket,
                          uint32_t *out_wait, int32_t *stats);
/* Diagnostics: what the DEVICE planner made of the list of this thread's last ffhip_hevc_intra_recon call (which it waits for):
 * out[0] != 0 the plan was refused and the list decoded by the one-wave serial kernel (exact, slow); out[1] groups; out[3] != 0 the
 * tickets are in decode order (no coding-tree wavefront found); out[4] the widest wavefront; out[5] log2 of the luma scheduling window;
 * out[6] != 0 a record failed the device's validation; out[7] != 0 the list was sorted by plane first (it interleaves the planes inside a
 * window, as the reference's order does).  FFHIP_EINVAL when that call did not use the device planner. */
int ffhip_debug_hevc_plan_result(uint32_t out[8]);
int ffhip_hevc_intra_recon(const ffhip_hevc_tu *h_tus, const ffhip_hevc_tu *d_tus, long long n_tus,
                           const int16_t *d_residual, int16_t *d_y, int16_t *d_cb, int16_t *d_cr,
                           int width_y, int height_y, int y_stride, int width_c, int height_c,
                           int uv_stride, int bitdepth_y, int bitdepth_c, void *stream);

/* The same for a list that is the CONCATENATION of independent pictures sharing one plane set -- the tiles of a HEIF grid, decoded one after
 * the other by the tile loop of format/heif.c:297-309 -- tile k being records [tile_first[k], tile_first[k + 1]) (tile_first[0] = 0; the last tile
 * ends at n_tus).  Same samples as ffhip_hevc_intra_recon on the whole list.  What the call adds is a PIPELINE across the stages of a decoder:
 * the pre-pass (validation, planner, substitution table, per-pixel programs: a third of an eight-picture call) depends on the TU list alone, so it
 * runs on a stream of the library's own WITHOUT waiting for `stream` -- next to whatever the caller enqueued there in front of this call: the
 * residual batches of these tiles, the colour conversion of the picture before -- and only the grouped kernel takes its place in `stream`.
 * Contract: d_tus holds the records WHEN THE CALL IS MADE (uploaded by a blocking copy, or by a copy whose event the host has waited for), not merely
 * by work enqueued on `stream`; h_tus / d_tus stay untouched until `stream` has passed the call.  d_residual and the planes are read and written in
 * `stream` order as always.  Consecutive calls alternate between two sets of library scratch, so the pre-pass of call n + 1 also runs next to the
 * tail of call n's grouped kernel (FFHIP_HEVC_TILE_SCRATCHES=1: one set).  FFHIP_HEVC_TILE_EARLY=0: everything in `stream` order
 * (= ffhip_hevc_intra_recon).  Eight / four / one 8K picture(s) as grids of 135 tiles, whole chain: 103 / 95 / 57 Gpixel/s against 90 / 85 / 48. */
int ffhip_hevc_intra_recon_tiles(const ffhip_hevc_tu *h_tus, const ffhip_hevc_tu *d_tus, long long n_tus,
                                 const long long *tile_first, int n_tiles, const int16_t *d_residual, int16_t *d_y,
                                 int16_t *d_cb, int16_t *d_cr, int width_y, int height_y, int y_stride, int width_c,
                                 int height_c, int uv_stride, int bitdepth_y, int bitdepth_c, void *stream);

/* ffhip_hevc_intra_recon_tiles and the colour conversion of the plane set (YUV420_to_BGRA32_16bit, utils/colorspace.c:628-669, as hevc.c:7260-7270
 * calls it) as ONE call: the tile loop of format/heif.c:297-309 with the conversion behind it.  d_bgra: pixel (x, y) of the plane set at
 * d_bgra + y * pitch + 4 * x (width_y x height_y pixels; 4:2:0: width_c = width_y / 2, height_c = height_y / 2; width_y a multiple of 4, height_y
 * even).  The colour kernel follows the grouped kernel on `stream`, next to the NEXT call's pre-pass on the library's stream.  One tile
 * (n_tiles = 1, tile_first = {0}) is an ordinary picture. */
int ffhip_hevc_decode_tiles(const ffhip_hevc_tu *h_tus, const ffhip_hevc_tu *d_tus, long long n_tus, const long long *tile_first,
                            int n_tiles, const int16_t *d_residual, int16_t *d_y, int16_t *d_cb, int16_t *d_cr, int width_y,
                            int height_y, int y_stride, int width_c, int height_c, int uv_stride, int bitdepth_y, int bitdepth_c,
                            uint8_t *d_bgra, int64_t pitch, void *stream);

/* ---- host-side JPEG front end and BMP sink (plain C, no GPU) ----
 * ffhip_jpeg_probe / ffhip_jpeg_entropy_decode stand where the marker loop, read_dqt,
 * read_compressed_scan and decode_data_unit stand (format/jpg.c:78-105, 255-415, 588-655,
 * 771-855; coding/huffman.c:92-222): a baseline / extended-sequential Huffman scan becomes the
 * MCU-order coefficient planes and natural-order quant tables ffhip_jpeg_recon_batch reads.
 * Progressive, arithmetic, 12-bit, non-interleaved or chroma-subsampling-other-than-1x1 files
 * return FFHIP_EINVAL from these calls (keep the C path); progressive files have entry points of their
 * own further down ("progressive JPEG").  All pointers are HOST pointers. */
int ffhip_jpeg_probe(const uint8_t *file, size_t len, ffhip_jpeg_geom *geom, int *width, int *height);
int ffhip_jpeg_entropy_decode(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect,
                              int16_t *coef_y, int16_t *coef_u, int16_t *coef_v, uint16_t *quant /* [4][64] */);
/* the same for one picture with n_threads host threads: a file with a DRI segment has independent
 * restart intervals (jpg.c:562-573), which are shared out; without one it is a single-thread decode */
int ffhip_jpeg_entropy_decode_mt(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect,
                                 int16_t *coef_y, int16_t *coef_u, int16_t *coef_v, uint16_t *quant,
                                 int n_threads);
/* n files of one geometry over n_threads host threads (with at least twice as many threads as files
 * the threads work inside each picture instead, as above); image i writes planes at
 * + i*blocks*64 and quant at + i*256; status[i] receives each file's code. */
int ffhip_jpeg_entropy_batch(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                             const ffhip_jpeg_geom *geom, int16_t *coef_y, int16_t *coef_u,
                             int16_t *coef_v, uint16_t *quant, int *status);
/* Test hook for the host staging pass of ffhip_jpeg_entropy_batch_gpu (needs no device): unstuffs the entropy-coded
 * bytes src[0..len) into dst (FF 00 -> FF), pads every restart interval to 4 bytes + 4 zero bytes, writes the clean
 * offset of interval k to seg[k] (k < n_seg) and the clean length to *clean_len; returns the number of intervals
 * found (RSTn-separated; another marker or the n_seg-th RSTn ends the scan), or FFHIP_EINVAL.
 * dst must hold len + 8 * n_seg + 64 bytes.  The reference's counterpart is the byte loop of read_compressed_scan
 * (format/jpg.c:588-637). */
int ffhip_jpeg_stage_scan_test(uint8_t *dst, const uint8_t *src, size_t len, uint32_t *seg, uint32_t n_seg, size_t *clean_len);
/* the same, and raw[k] = the bytes of interval k without its padding (what the subsequence decoder cuts into lanes of 2048 / 4096 / 8192 bits) */
int ffhip_jpeg_stage_scan_raw_test(uint8_t *dst, const uint8_t *src, size_t len, uint32_t *seg, uint32_t n_seg, size_t *clean_len, uint32_t *raw);
/* Test hook (needs no device): the two-level look-up table the device Huffman kernels use for table `which` (0..3 DC, 4..7 AC) of a file, 1536 uint16:
 * [0..511] by the next 9 bits: (length << 8) | symbol, or 0x8000 | g for a prefix of longer codes; [512 + 128 g + b] group g by the 7 bits behind
 * the prefix; 0x5000 = no code starts with these bits (a table that holds all its codes says so itself); 0 = take the canonical-code walk.  The
 * reference's counterpart is huffman_decode_symbol (coding/huffman.c:92-222). */
int ffhip_jpeg_lut_test(const uint8_t *file, size_t len, int which, uint16_t *out);

/* The same front end ON the device: decodes straight into DEVICE planes (d_coef_*, d_quant [n][4][64]) laid out for
 * ffhip_jpeg_recon_batch with quant_stride 256; the host only parses headers, finds the RSTn markers and unstuffs the
 * bytes into pinned memory.  files/lens/status are HOST arrays.  Round 5: a lane decodes one SUBSEQUENCE of a restart interval
 * -- of the whole scan, in a file without DRI; 2048, 4096 or 8192 bits, by the bits an MCU takes in the batch (up to 1024, up to 2048, more;
 * FFHIP_JPEG_SYNC_BITS sets it), worked out once per call -- and the lanes are brought into step with each other over a few rounds
 * (Huffman-coded data self-synchronises; DESIGN.md 5 "The subsequence decoder"), so files need no restart markers to decode
 * in parallel, and a batch may mix files with and without.  FFHIP_JPEG_SYNC=0: the kernel of rounds 3-4, one lane per restart
 * interval (a file without DRI is ONE lane's then: for batches of a thousand files or more only); unset, that kernel also takes
 * the batches whose restart intervals are a subsequence or two long by that same figure (a DRI of a few MCUs); =1 keeps the subsequence decoder on those.
 * FFHIP_EINVAL for a file of another geometry, and for a damaged or truncated scan (status[] says which picture; nothing of
 * the batch is to be used then -- ffhip_jpeg_decode_files* fall back to the host decoder).  Synchronises `stream` (the
 * per-picture verdicts come back with it). */
int ffhip_jpeg_entropy_batch_gpu(const uint8_t *const *files, const size_t *lens, int n, int n_threads /* host: header
                                 parsing, marker search, staging */, const ffhip_jpeg_geom *geom, int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant,
                                 int *status, void *stream);

/* Diagnostics: where the calling thread's last ffhip_jpeg_entropy_batch_gpu call spent its time, in microseconds: out[0] header parse,
 * [1] layout, [2] unstuffing + marker search into pinned memory (each part's upload and kernels are enqueued behind it), [3] tables, [4] enqueue,
 * [5] the wait for uploads + clears + kernels, [6] HIP events on the call's stream around everything the call has the device do (the subsequence
 * decoder: uploads waited for, rounds, scan, write pass of all parts; FFHIP_JPEG_SYNC=0: the Huffman kernel alone), [7] the whole call. */
int ffhip_debug_huff_times(double out[8]);

/* Files in, pixels out (f1 + the hot path + f2's producer side): n baseline JPEG files of ONE geometry are
 * entropy-decoded `chunk` pictures at a time (0 = default: 32 pictures, or as many small ones as make 256 MB of BGRA; 8 with the
 * host decoder) -- on the device (ffhip_jpeg_entropy_batch_gpu), or, when that
 * refuses a chunk or FFHIP_JPEG_GPU_ENTROPY=0 says so, by n_threads host threads into pinned memory -- while the
 * previous chunk is copied to the device, reconstructed by one launch and copied back -- a double-buffered
 * pipeline whose steady state is the slower of host entropy decode and PCIe.  bgra is HOST memory,
 * pixel (x, y) of picture i at bgra + i*image_stride + y*pitch + 4*x (coded size, geom_out tells it);
 * status[i] = per-file code, the return value the first failure.  The layout format/jpg.c:851-852 hands
 * to struct pic.  Not for single-component files with several blocks per MCU.  A destination in pinned
 * memory (ffhip_host_malloc, or the caller's own hipHostMalloc / hipHostRegister) receives the device copy
 * directly; a pageable one goes through pinned staging and a threaded copy.  Buffers are kept between calls;
 * one call at a time. */
/* The same with the pixels left ON THE DEVICE (d_bgra, pitch and image_stride as for ffhip_jpeg_recon_batch): for a
 * consumer that lives on the GPU only the compressed bytes cross PCIe.  Files with or without restart markers: one batch, entropy
 * decode on the device (ffhip_jpeg_entropy_batch_gpu: the subsequence decoder by default), each part's reconstruction enqueued behind its
 * write pass (the entropy stage synchronises the stream).  Only when the device decoder refuses the batch with FFHIP_EINVAL (or
 * FFHIP_JPEG_GPU_ENTROPY=0 says so) do host threads decode chunks of a few pictures into pinned memory while the previous chunk is
 * uploaded and reconstructed on a stream of the library's own; `stream` is synchronised first and every picture is in d_bgra when the
 * call returns. */
int ffhip_jpeg_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                   ffhip_jpeg_geom *geom_out, uint8_t *d_bgra, int64_t pitch, int64_t image_stride,
                                   int *status, void *stream);
/* Files of ANY baseline geometry in one call, pixels on the device: picture i at d_bgra[i] with pitch[i] (its coded size, as
 * ffhip_jpeg_probe reports it: the caller probes, then allocates; 16-byte aligned, pitch as for ffhip_jpeg_recon_items).  Headers
 * are parsed on n_threads host threads, the files grouped by layout class, and per class the device entropy decoder runs over
 * pictures of different sizes, with one ffhip_jpeg_recon_items launch behind each part of its write pass; a class the device
 * decoder refuses (or all of them, FFHIP_JPEG_GPU_ENTROPY=0) is decoded by host threads into pinned memory and uploaded.
 * geom_out[i] (may be NULL) receives each file's geometry, status[i] its code: a damaged, truncated, progressive, 12-bit or
 * two-pass-layout file gets a non-zero code and no promised output bytes, and every other file is still decoded.  Returns the
 * first failure.  Synchronises `stream` like ffhip_jpeg_decode_files_device. */
int ffhip_jpeg_decode_files_mixed_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                         uint8_t *const *d_bgra, const int64_t *pitch, ffhip_jpeg_geom *geom_out,
                                         int *status, void *stream);
void *ffhip_host_malloc(size_t bytes); /* pinned host memory */
void ffhip_host_free(void *p);
int ffhip_jpeg_decode_files(const uint8_t *const *files, const size_t *lens, int n, int n_threads, int chunk,
                            ffhip_jpeg_geom *geom_out, uint8_t *bgra, int64_t pitch, int64_t image_stride,
                            int *status);

/* display/bmpwriter.c:19-81: 54-byte header + top-down 32-bit rows; byte-identical files. */
int ffhip_bmp_write(const char *path, const uint8_t *bgra, int width, int height, int64_t pitch);

/* Device-to-device copy kernel (16 B/lane, grid-stride) used by bench.py to
 * calibrate the achievable HBM rate next to the fused kernel. */
int ffhip_copy_calibrate(void *d_dst, const void *d_src, size_t bytes, void *stream);
/* A second calibration for the same purpose: the 4:2:0 fused kernel's own ACCESS PATTERN -- its loads and its stores, same grid, same addresses --
 * with the arithmetic taken out, on the caller's buffers (d_bgra receives meaningless bytes).  The rate of this launch is the ceiling the fused
 * kernel can be read against on exactly this placement of its buffers (DESIGN.md 5 "Round 6").  Arguments as ffhip_jpeg_recon_batch; every layout a fused kernel takes
 * (4:2:0, 4:4:4, 4:2:2, 4:4:0, 4:1:1, its transpose, grey), FFHIP_EINVAL for the others. */
int ffhip_jpeg_pattern_calibrate(const ffhip_jpeg_geom *geom, int n_images, const int16_t *d_coef_y, const int16_t *d_coef_u, const int16_t *d_coef_v,
                                 const uint16_t *d_quant, int64_t quant_stride, uint8_t *d_bgra, int64_t pitch, int64_t image_stride, void *stream);

/* ---- decoded pictures into tensors (ffhip_tensor.hip) ----
 * The decode calls leave the reference's picture: BGRA with a constant alpha byte, the coded size, a pitch.  A program on the GPU reads
 * tensors: RGB or BGR, planar or interleaved, bytes or normalised floats, the display size or a region of it.  This is that last stage. */
#define FFHIP_TENSOR_U8 0
#define FFHIP_TENSOR_F16 1
#define FFHIP_TENSOR_F32 2
typedef struct ffhip_tensor_format {
    int32_t dtype;  /* FFHIP_TENSOR_*                                                                                     */
    int32_t bgr;    /* 0: channels R,G,B   non-zero: B,G,R                                                                */
    int32_t planar; /* non-zero: [3][H][W] (CHW)   0: [H][W][3] (HWC)                                                     */
    float scale[3]; /* per OUTPUT channel: out = (float)byte * scale[c] + bias[c], the product and the sum each rounded   */
    float bias[3];  /* to float (the library is built with -ffp-contract=off); F16: that float converted round-to-nearest- */
                    /* even; U8: the byte itself, scale must be 1 and bias 0.  All six finite                             */
} ffhip_tensor_format;
/* One picture of a batch.  All pointers are DEVICE pointers.
 *   d_bgra, pitch      a picture as the decode calls write it: 4-byte aligned, pitch a multiple of 4
 *   x0, y0, width,     the rectangle to take (width, height >= 1, x0, y0 >= 0); the caller keeps it inside the picture, the call checks
 *   height             what it can: 4 (x0 + width) <= pitch, and (y0 + height) pitch < 2^31 -- the bound of the decode calls' own pictures
 *   d_out              element 0 of the output, aligned to ONE element only (a slice of a larger tensor starts anywhere)
 *   row_stride,        in elements.  HWC: element (y, x, c) at y row_stride + 3 x + c, row_stride >= 3 width, plane_stride unused.
 *   plane_stride       CHW: element (c, y, x) at c plane_stride + y row_stride + x, row_stride >= width,
 *                      plane_stride >= row_stride (height - 1) + width
 * The alpha byte is ignored (ffhip_bgra_to_tensor_items_alpha below keeps it).  Only the width x height elements per channel are written: row padding, plane padding and the bytes around the
 * output stay untouched, whatever the output's alignment (rows are cut along the DESTINATION's 16-byte blocks: whole blocks are stored as
 * one 16-byte store, the partial block at either end of a row element by element). */
typedef struct ffhip_tensor_item {
    const uint8_t *d_bgra;
    int64_t pitch;
    int32_t x0, y0, width, height;
    void *d_out;
    int64_t row_stride, plane_stride;
} ffhip_tensor_item;
/* ONE launch for the whole batch, pictures and outputs of any sizes, all in format *fmt (the twelve combinations of dtype, planar and bgr
 * are instances of one kernel body, chosen here).  `items` is a HOST array; every check is made before anything is enqueued
 * (FFHIP_EINVAL -- an unknown dtype, U8 with a scale other than 1 or a bias other than 0, a scale or bias that is not finite, an item
 * outside what its fields' lines above say --, on a machine without a device too; FFHIP_ENODEV there for good arguments).  n == 0 is
 * FFHIP_OK.  Only enqueues on `stream`; the records and the per-workgroup table are library scratch of the stream. */
int ffhip_bgra_to_tensor_items(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, void *stream);

/* ---- alpha into the tensors (ffhip_alpha_body.h, ffhip_tensor.hip) ----
 * PNG, lossless WebP and lossy WebP with an ALPH chunk decode to BGRA with real alpha; the call above ignores that byte.  This record
 * tells the sink -- and, through the _alpha file calls, the whole chain -- what to make of it.  Integers only, every step held against
 * PIL (tests/test_tensor_alpha_capi.py); c, p, g, a are bytes, div255(t) = (t + 128 + ((t + 128) >> 8)) >> 8 = floor(t / 255 + 1/2):
 *   premultiply         p = div255(c a)                                  (PIL convert("RGBa"))
 *   un-premultiply      a == 0 ? 0 : floor(255 p / a)                    (PIL RGBa -> RGBA; exact for p <= a, at most 255)
 *   over g, straight    div255(c a + g (255 - a))                        (PIL Image.alpha_composite onto an opaque background)
 *   over g, premult.    p + div255(g (255 - a))                          (p <= a: at most 255)
 * A source that claims to be premultiplied and is not (p > a) gives bytes saturated at 255, never anything outside its element.
 *   FFHIP_ALPHA_DROP           three channels, the alpha byte ignored: ffhip_bgra_to_tensor_items
 *   FFHIP_ALPHA_STRAIGHT       four channels R,G,B,A (bgr: B,G,R,A): the colour as stored, un-premultiplied where the source is premultiplied
 *   FFHIP_ALPHA_PREMULTIPLIED  four channels, the colour p: premultiplied here where the source is straight
 *   FFHIP_ALPHA_OVER           three channels, the colour composited over `background`
 * Float outputs: the colour channels take fmt's scale and bias, applied to the byte the rule gives; the alpha channel takes alpha_scale
 * and alpha_bias by the same two-rounding expression.  U8 needs alpha_scale 1 and alpha_bias 0; both finite. */
#define FFHIP_ALPHA_DROP 0
#define FFHIP_ALPHA_STRAIGHT 1
#define FFHIP_ALPHA_PREMULTIPLIED 2
#define FFHIP_ALPHA_OVER 3
typedef struct ffhip_tensor_alpha {
    int32_t mode;                 /* FFHIP_ALPHA_*                                                                       */
    int32_t source_premultiplied; /* 0: the pictures are straight BGRA, as the decode calls leave them; 1: premultiplied */
    uint8_t background[4];        /* B,G,R,unused: FFHIP_ALPHA_OVER                                                      */
    float alpha_scale, alpha_bias;
} ffhip_tensor_alpha;
/* ffhip_bgra_to_tensor_items under *alpha.  alpha == NULL or mode FFHIP_ALPHA_DROP: that call, bit for bit (the rest of the record is not
 * read).  Items as there; with four channels HWC element (y, x, c) is at y row_stride + 4 x + c, row_stride >= 4 width, and CHW has four
 * planes, the alpha plane last.  FFHIP_EINVAL besides that call's: an unknown mode, source_premultiplied other than 0 or 1, an alpha
 * scale or bias that is not finite, U8 with alpha_scale other than 1 or alpha_bias other than 0.  Every check is made before anything is
 * enqueued (FFHIP_EINVAL in front of FFHIP_ENODEV).  Only enqueues on `stream`. */
int ffhip_bgra_to_tensor_items_alpha(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, const ffhip_tensor_alpha *alpha, void *stream);

/* Files in, tensors out.  outs[i] is file i's output (fields as in ffhip_tensor_item); roi[i] the rectangle of its DISPLAY picture to
 * deliver, roi == NULL the whole of it: width x height as ffhip_jpeg_probe reports them, ffhip_webp_info.width x .height (what of it
 * the decoded picture holds) for WebP.  The caller probes, then allocates.
 * The batch is decoded in PARTS by ffhip_jpeg_decode_files_mixed_device / ffhip_webp_decode_files_device into BGRA pictures (coded size,
 * pitch 4 x the coded width) that are library scratch of the stream, ffhip_bgra_to_tensor_items behind each part.  A part's pictures take at
 * most 1 GiB (FFHIP_TENSOR_PART_BYTES replaces the figure: lets tests reach the many-part form with small batches); a single picture
 * larger than that is a part of its own.
 * Per file the semantics of the calls underneath: status[i] receives each file's code -- a file they refuse or find damaged theirs,
 * FFHIP_EINVAL for a rectangle that is empty or leaves the display picture and for an output ffhip_bgra_to_tensor_items would refuse --,
 * nothing of such a file's output is written, every other file is delivered; geom_out / info_out (may be NULL) as underneath.  Returns the
 * first failure.  FFHIP_EINVAL for NULL files, lens, fmt, outs or status and for a format the items call refuses; every check is made
 * before anything is enqueued (on a machine without a device too; FFHIP_ENODEV there for good arguments).  Synchronises `stream`. */
typedef struct ffhip_tensor_out {
    void *d_out;
    int64_t row_stride, plane_stride;
} ffhip_tensor_out;
typedef struct ffhip_rect {
    int32_t x0, y0, width, height;
} ffhip_rect;
int ffhip_jpeg_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                   const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_jpeg_geom *geom_out, int *status, void *stream);
int ffhip_webp_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                   const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_webp_info *info_out, int *status, void *stream);

/* ---- decoded pictures resized on the device (ffhip_resize.hip) ----
 * The tensor stage above keeps every picture's size; a program that trains or infers wants one [N,3,H,W].  This stage resizes BGRA
 * rectangles of any sizes to BGRA pictures of any sizes in one call, by a rule that is integers only, so that every
 * implementation of it gives the same bytes.  Each axis alone, n_in source samples -> n_out output samples:
 *   S = 2 n_out (FFHIP_RESIZE_BILINEAR: two taps) or 2 max(n_in, n_out) (FFHIP_RESIZE_ANTIALIAS: the triangle widens with the shrink
 *   factor, as PIL's and torch's antialias=True).  For output o, c = (2 o + 1) n_in; source sample k is a tap iff
 *   d_k = |(2 k + 1) n_out - c| < S and 0 <= k < n_in (taps outside are dropped, never read; the taps are a run first .. first + count - 1).
 *   r_k = S - d_k, R their sum, q_k = floor((4096 r_k + floor(R / 2)) / R); 4096 - sum(q) is added to the tap of the largest r (the
 *   lowest k on a tie): sum(q) == 4096.  Every q is >= 0: where a run of many hundred taps rounds up more often than its largest weight
 *   can pay for (ANTIALIAS 1080 -> 1: 41 too many, the largest weight 7), that tap becomes 0 and what is still owed is taken from the
 *   taps that follow in the same order -- falling r, the lowest k on a tie --, each down to 0 at most.  No run of up to 224 taps needs it.
 * A byte of output pixel (ox, oy) is (sum_y sum_x qy qx v[y][x] + 2^23) >> 24: one rounding, no clamp needed (at most 255 2^24 + 2^23).
 * All four bytes of a pixel are filtered alike: a constant alpha stays constant, equal sizes on both axes are a copy.  For pictures with
 * real alpha that is the wrong rule -- the colour stored under transparent pixels reaches the edges --: ffhip_bgra_resize_items_premultiplied. */
#define FFHIP_RESIZE_BILINEAR 0
#define FFHIP_RESIZE_ANTIALIAS 1
#define FFHIP_RESIZE_MAX_SIDE 16384 /* of a source rectangle and of an output: (2 k + 1) n_out stays below 2^30 */
/* The rule for one output index, on the HOST (no device needed; the kernels run the same function): returns the tap count of output `o`,
 * *first = its first source sample, q[0 .. min(count, cap) - 1] the weights, each in 0..4096 (q may be NULL when cap is 0).  FFHIP_EINVAL for n_in or
 * n_out outside 1..16384, an unknown filter, o outside 0..n_out-1, first == NULL, cap < 0. */
int ffhip_resize_axis_taps(int n_in, int n_out, int filter, int o, int *first, uint16_t *q, int cap);
/* One picture of a batch.  All pointers are DEVICE pointers.
 *   d_src, src_pitch   a BGRA picture as the decode calls write it: 4-byte aligned, pitch a multiple of 4
 *   x0, y0, width,     the source rectangle (x0, y0 >= 0; width, height in 1..16384); the caller keeps it inside the picture, the call
 *   height             checks what it can: 4 (x0 + width) <= src_pitch, and (y0 + height) src_pitch < 2^31
 *   d_dst, dst_pitch   the output picture: 4-byte aligned, dst_pitch a multiple of 4, >= 4 out_width and <= 2^40
 *   out_width,         in 1..16384
 *   out_height
 * Only the out_width x out_height pixels are written (one dword store each): the row padding of the destination stays untouched.
 * Source and destination must not overlap. */
typedef struct ffhip_resize_item {
    const uint8_t *d_src;
    int64_t src_pitch;
    int32_t x0, y0, width, height;
    uint8_t *d_dst;
    int64_t dst_pitch;
    int32_t out_width, out_height;
} ffhip_resize_item;
/* The whole batch, rectangles and outputs of any sizes, in ONE resize launch behind one small launch that writes the batch's tap tables
 * (the rule above, per item and axis) and its per-workgroup table.  `items` is a HOST array; every check is made before anything is
 * enqueued (FFHIP_EINVAL -- n < 0, NULL items with n > 0, a filter other than the two above, an item outside what its fields' lines above
 * say --, on a machine without a device too; FFHIP_ENODEV there for good arguments).  n == 0 is FFHIP_OK.  Only enqueues on `stream`; the
 * records, the per-workgroup table and the tap tables are library scratch of the stream. */
int ffhip_bgra_resize_items(const ffhip_resize_item *items, int n, int filter, void *stream);
/* The same call for pictures with real alpha: the source is STRAIGHT BGRA, every pixel is premultiplied (p = div255(c a), "alpha into the
 * tensors" above) as its row is staged, the rule above runs unchanged over the four premultiplied bytes, and the destination is
 * PREMULTIPLIED BGRA (p <= a holds for every output pixel: the weights are non-negative and sum to 4096, and the rounding is monotone).
 * The colour stored under transparent pixels therefore never reaches the output, which it does through the call above.  An opaque
 * picture gives that call's bytes.  Items, checks and scratch as there. */
int ffhip_bgra_resize_items_premultiplied(const ffhip_resize_item *items, int n, int filter, void *stream);

/* Files in, tensors of chosen sizes out: ffhip_*_decode_files_tensor with the resize between the decoder and the tensor stage.  roi[i]
 * (roi == NULL: the whole display picture) is file i's SOURCE rectangle, out_size[i] the size it is resized to by `filter`, and outs[i]
 * is laid out for out_size[i].  Per part: the decode call, ffhip_bgra_resize_items into BGRA pictures of the target sizes (pitch
 * 4 x out width; library scratch of the stream), ffhip_bgra_to_tensor_items; a part's decoded and resized pictures together keep the
 * part budget of the calls above.  Per file as above, and status[i] = FFHIP_EINVAL also for a rectangle side or an out_size side
 * outside 1..16384 and for an output ffhip_bgra_to_tensor_items would refuse for out_size[i]: nothing of that file is written, the
 * others are delivered.  FFHIP_EINVAL for what the calls above refuse, for NULL out_size (n > 0) and for an unknown filter, before
 * anything is enqueued (on a machine without a device too; FFHIP_ENODEV there for good arguments).  Synchronises `stream`. */
typedef struct ffhip_size {
    int32_t width, height;
} ffhip_size;
int ffhip_jpeg_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                           const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                           ffhip_jpeg_geom *geom_out, int *status, void *stream);
int ffhip_webp_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                           const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                           ffhip_webp_info *info_out, int *status, void *stream);

/* ---- JPEG pictures at 1/2, 1/4 and 1/8 size straight from the coefficients (ffhip_jpeg_scaled.hip) ----
 * A loader that shrinks camera pictures to a few hundred pixels does not need them at full size first.  With the denominator d in 1, 2, 4, 8
 * and N = 8 / d, a block of a component becomes N x N samples by the steps of the full-size path (format/jpg.c:247-253, utils/idct.c:512-534)
 * with an N-point matrix in place of the 8-point one (what libjpeg's scale_num / 8 and PIL's draft() do):
 *   1. F[v][u] = (int16)(coef[8 v + u] * quant[8 v + u])                          for u, v < N (natural order)
 *   2. c[y][u] = (int16)((sum_v T_N[y][v] F[v][u] + 1024) >> 11)
 *   3. s[y][x] = max(0, (sum_u T_N[x][u] c[y][u] + (257 << 17)) >> 18)
 * all sums int32; T_N[x][u] = round(8192 sqrt(2) alpha(u) cos((2 x + 1) u pi / 2 N)): T_1 = [[8192]], T_2 = [[8192, 8192], [8192, -8192]],
 * T_4 = [[8192, 10703, 8192, 4433], [8192, 4433, -8192, -10703], [8192, -4433, -8192, 10703], [8192, -10703, 8192, -4433]].  No sum can leave
 * int32 (the largest row of |T_4| is 31 520, the inputs are int16) and a sample is at most 4068: the full-size path's upper clamp cannot bind.
 * A DC-only block gives, at every N, the value the full-size path gives each of its 64 pixels.
 * The picture at denominator d: coded size (N h mcu_cols) x (N v mcu_rows), display size ceil(W / d) x ceil(H / d); pixel (x, y) of an MCU takes
 * sample (y % N, x % N) of luma block (y / N) h + x / N and sample (y / v, x / h) of the MCU's one chroma block (the replication of
 * utils/colorspace.c:148-150); B, G, R, 0xFF by the full-size path's conversion, grey files with its U = V = 0.
 * d = 1 is the full-size path itself, byte for byte: it is routed to the full-size kernels. */
/* Host only, no device needed: the block rule.  out receives the N x N samples row-major, N = 8 / denom, denom 2, 4 or 8 (FFHIP_EINVAL for 1:
 * the 8 x 8 rule is the full-size kernels' and ffhip_get_dct_ops's).  The kernel runs the same function (ffhip_jpeg_scaled_body.h). */
int ffhip_jpeg_scaled_block(const int16_t *coef /* [64] */, const uint16_t *quant /* [64] */, int denom, int16_t *out /* [N][N] */);
/* Host only.  *w = ceil(width / denom), *h = ceil(height / denom): the display size at that denominator. */
int ffhip_jpeg_scaled_size(int width, int height, int denom, int *w, int *h);
/* Host only.  A rectangle of the FULL-SIZE display picture (inside width x height, not empty) mapped onto the picture at `denom`:
 * x0' = x0 / d, x1' = min(ceil(W / d), ceil((x0 + w) / d)), likewise y.  Its edges may lie up to d - 1 source pixels outside the request. */
int ffhip_jpeg_scaled_rect(int width, int height, int denom, const ffhip_rect *roi, ffhip_rect *out);
/* Host only.  The largest d in 8, 4, 2, 1 at which a rect_w x rect_h rectangle at the origin, mapped as above (ceil(rect_w / d) x
 * ceil(rect_h / d); a rectangle elsewhere maps to at least that), is still at least out_w x out_h; 1 when none is (a target larger than
 * the rectangle).  FFHIP_EINVAL for a side below 1. */
int ffhip_jpeg_scale_choose(int rect_w, int rect_h, int out_w, int out_h);
/* Luma blocks side by side that one workgroup of the reduced kernel covers (a wave is that wide; its four waves take four rows) */
#define FFHIP_JPEG_SCALED_WG_BLOCKS 64
int ffhip_jpeg_scaled_wg_blocks(void);
/* ffhip_jpeg_recon_items with a denominator per item: item i is written at 1 / denom[i] of its size.  Per item as there, except
 *   d_bgra, pitch   the SCALED coded picture, (8 / d) h mcu_cols x (8 / d) v mcu_rows: 16-byte aligned, pitch >= 4 x that width and a
 *                   multiple of 16.  Nothing beyond 4 x the scaled coded width of a row is written
 * One launch per denominator present (2, 4, 8: one kernel, generic over the seven fused layout classes; the two-pass layouts stay
 * refused), and the items of denominator 1 through ffhip_jpeg_recon_items.  `items` and `denom` are HOST arrays; every check is made
 * before anything is enqueued (FFHIP_EINVAL -- a denominator other than 1, 2, 4, 8 included --, on a machine without a device too;
 * FFHIP_ENODEV there for good arguments).  Only enqueues on `stream`. */
int ffhip_jpeg_recon_items_scaled(const ffhip_jpeg_item *items, const int *denom, int n, void *stream);
/* ffhip_jpeg_decode_files_mixed_device with a denominator per file: picture i at d_bgra[i] at its SCALED coded size (pitch[i] as for
 * ffhip_jpeg_recon_items_scaled).  Probe, entropy decode and write pass are the unscaled call's; the denominators travel to the
 * reconstruction behind the device entropy decoder's parts and to the one behind the host threads' upload.  FFHIP_EINVAL for NULL denom
 * and for a denominator other than 1, 2, 4, 8, before anything else. */
int ffhip_jpeg_decode_files_mixed_device_scaled(const uint8_t *const *files, const size_t *lens, int n, int n_threads,
                                                uint8_t *const *d_bgra, const int64_t *pitch, const int *denom,
                                                ffhip_jpeg_geom *geom_out, int *status, void *stream);
/* ffhip_jpeg_decode_files_tensor_resized with a denominator per file.
 *   denom[i]     1, 2, 4, 8, or 0: "choose" -- ffhip_jpeg_scale_choose of the file's rectangle and out_size[i] (needs out_size: FFHIP_EINVAL
 *                without).  denom_out[i] (may be NULL) receives the denominator used, 0 for a file the probe refused
 *   roi          stays in FULL-SIZE display coordinates (NULL: the whole picture), is checked there, and is mapped as
 *                ffhip_jpeg_scaled_rect says: the resize (or, without one, the tensor stage) reads the mapped rectangle, whose edges may lie
 *                up to d - 1 source pixels outside the request
 *   out_size     may be NULL: the tensor then has the mapped rectangle's size, outs[i] is laid out for it, `filter` is still checked
 * The parts of the batch are sized by the SCALED coded pictures (pitch 4 x the scaled coded width rounded up to 16 bytes).  All 1: the
 * bytes of the unscaled calls. */
int ffhip_jpeg_decode_files_tensor_scaled(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                          const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                          const int *denom, int *denom_out, ffhip_jpeg_geom *geom_out, int *status, void *stream);
/* Diagnostics: the parts the calling thread's last ffhip_*_decode_files_tensor* call cut its batch into, counted from the moment the call has
 * probed its files: 0 where it then returned before its first part (a missing device, a failed allocation).  A call refused for its
 * arguments before that, or one of no files, leaves the count as it was. */
int ffhip_debug_tensor_last_parts(void);

/* ---- EXIF orientation: decoded pictures upright (ffhip_exif.c, ffhip_orient.hip) ----
 * A camera stores the sensor's picture and says in the EXIF orientation tag (0x0112, 1..8) how to hold it; the decoders above deliver the
 * STORED picture S, Ws x Hs, as the reference does (it skips APP1, format/jpg.c:836-840).  The UPRIGHT picture U of orientation o:
 *   o   U size    U[y][x] =                  o   U size    U[y][x] =
 *   1   Ws x Hs   S[y][x]                    5   Hs x Ws   S[x][y]
 *   2   Ws x Hs   S[y][Ws-1-x]               6   Hs x Ws   S[Hs-1-x][y]
 *   3   Ws x Hs   S[Hs-1-y][Ws-1-x]          7   Hs x Ws   S[Hs-1-x][Ws-1-y]
 *   4   Ws x Hs   S[Hs-1-y][x]               8   Hs x Ws   S[x][Ws-1-y]
 * (what PIL.ImageOps.exif_transpose and torchvision's apply_exif_orientation deliver).  Pure pixel movement: no byte changes its value. */
/* Host only, no device needed.  The orientation tag of a JPEG file: the marker segments behind SOI are walked up to the first SOS or EOI,
 * the first APP1 whose payload begins "Exif\0\0" decides; in it the TIFF header ("II*\0" or "MM\0*"), IFD0 and its 12-byte entries, of
 * which the first with tag 0x0112 counts: type SHORT or LONG, count 1, a value in 1..8, read in the file's byte order.  No other IFD is
 * followed.  FFHIP_EINVAL only for a NULL argument; otherwise FFHIP_OK, with *orientation = 1 for no tag, a malformed one or a value outside
 * 1..8: a bad tag never fails a decode.  Nothing outside file[0 .. len) is read, whatever the lengths and offsets in the file say. */
int ffhip_jpeg_exif_orientation(const uint8_t *file, size_t len, int *orientation);
/* The same for a WebP file: the RIFF chunks are walked by their sizes (with the format's padding byte behind an odd one), past the `VP8 `
 * chunk, to the first `EXIF` chunk, whose payload is that TIFF structure, with or without "Exif\0\0" in front. */
int ffhip_webp_exif_orientation(const uint8_t *file, size_t len, int *orientation);
/* Host only.  *uw x *uh = the upright size of a stored w x h picture.  FFHIP_EINVAL for o outside 1..8, a side below 1, a NULL result. */
int ffhip_orient_size(int w, int h, int o, int *uw, int *uh);
/* Host only.  A rectangle of the UPRIGHT picture mapped onto the stored ws x hs picture: the rectangle of S that holds its pixels (under
 * o = 6, (x0, y0, w, h) becomes (y0, hs - x0 - w, h, w)).  Orienting that stored rectangle on its own gives the upright rectangle:
 * orient(S)[upright] == orient(S[stored]).  FFHIP_EINVAL for o outside 1..8, a side of the picture below 1 and for a rectangle that is
 * empty or leaves the upright picture. */
int ffhip_orient_rect(int ws, int hs, int o, const ffhip_rect *upright, ffhip_rect *stored);
/* Host only.  The orientation that undoes o: 1..5 and 7 are their own inverse, 6 and 8 each other's.  FFHIP_EINVAL outside 1..8. */
int ffhip_orient_inverse(int o);
/* One picture of a batch.  All pointers are DEVICE pointers.
 *   d_src, src_pitch   a BGRA picture as the decode calls write it: 4-byte aligned, pitch a multiple of 4
 *   x0, y0, width,     the STORED rectangle to turn (width, height >= 1, x0, y0 >= 0); the caller keeps it inside the picture, the call
 *   height             checks what ffhip_tensor_item's line says: 4 (x0 + width) <= src_pitch, and (y0 + height) src_pitch < 2^31
 *   d_dst, dst_pitch   the upright picture (height x width pixels for orientation 5..8): 4-byte aligned, dst_pitch a multiple of 4,
 *                      >= 4 x the upright width and <= 2^32
 *   orientation        1..8; 1 is a plain copy of the rectangle
 * Only the upright width x height pixels are written (one dword store each): the row padding of the destination stays untouched.
 * Source and destination must not overlap. */
typedef struct ffhip_orient_item {
    const uint8_t *d_src;
    int64_t src_pitch;
    int32_t x0, y0, width, height;
    uint8_t *d_dst;
    int64_t dst_pitch;
    int32_t orientation;
} ffhip_orient_item;
/* The whole batch, rectangles of any sizes and orientations, in ONE launch behind the small launch that writes the per-workgroup table.  A
 * workgroup moves one 64 x 64 tile of a stored rectangle: straight (1..4: mirrored reads, row stores) or through an LDS tile (5..8: rows
 * in, columns out, both sides of memory in runs of 64 dwords).  `items` is a HOST array; every check is made before
 * anything is enqueued (FFHIP_EINVAL -- n < 0, NULL items with n > 0, an item outside what its fields' lines above say --, on a machine
 * without a device too; FFHIP_ENODEV there for good arguments).  n == 0 is FFHIP_OK.  Only enqueues on `stream`; the records and the
 * per-workgroup table are library scratch of the stream. */
int ffhip_bgra_orient_items(const ffhip_orient_item *items, int n, void *stream);
/* Files in, UPRIGHT tensors out: supersets of ffhip_jpeg_decode_files_tensor_scaled and ffhip_webp_decode_files_tensor_resized.
 *   orient[i]    1..8: the orientation to apply, whatever the file says; 0: the file's tag (the functions above).  orient == NULL: every
 *                file's tag.  Any other value: FFHIP_EINVAL for the whole call.  orient_out[i] (may be NULL) receives the value used, 0
 *                for a file the probe refused
 *   roi, out_size, outs   in UPRIGHT coordinates: roi[i] a rectangle of the upright picture (NULL: all of it), out_size[i] the upright
 *                size to resize it to (out_size may be NULL: no resize; `filter` is still checked), outs[i] laid out for the upright result
 *   denom, denom_out (JPEG)   as ffhip_jpeg_decode_files_tensor_scaled; denom may be NULL: every file at full size
 * Decode, reduced decode and resize run in the STORED axes exactly as in the calls above: the rectangle is mapped by ffhip_orient_rect,
 * out_size[i] is swapped for 5..8, ffhip_jpeg_scale_choose and ffhip_jpeg_scaled_rect see those.  Then ffhip_bgra_orient_items moves whole
 * pixels once -- the resized picture where there is a resize, the (mapped) rectangle otherwise -- into part scratch at pitch 4 x upright
 * width, which counts towards the part budget, and the tensor stage reads that.  So the result is, byte for byte, the table above applied
 * to what the calls above deliver for the mapped rectangle and size, and the expensive stages see no more pixels than there.  (The resize
 * rule's tie-break, "the lowest k on a tie", is not mirror-symmetric: resizing the upright picture could differ in a rare last bit.  The
 * result is DEFINED in the stored axes.)  Files of orientation 1 take the way of the calls above; a batch of nothing else issues their
 * launches and gives their bytes.  status[i] = FFHIP_EINVAL also for a rectangle that leaves the UPRIGHT picture and for an output laid
 * out for the un-swapped size where the tensor stage refuses it; that file alone is affected. */
int ffhip_jpeg_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                            const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                            const int *denom, int *denom_out, const int *orient, int *orient_out, ffhip_jpeg_geom *geom_out,
                                            int *status, void *stream);
/* ffhip_webp_decode_files_tensor_oriented with `flags` (0, or FFHIP_WEBP_PIXELS_LIBWEBP: any other bit is FFHIP_EINVAL): the files are probed and
 * decoded under that rule, and the region, resize and orientation stages act on the picture it gives -- under the libwebp rule the frame tag's
 * width x height.  flags == 0 gives the bytes of ffhip_webp_decode_files_tensor_oriented. */
int ffhip_webp_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                      const int *orient, int *orient_out, unsigned flags, ffhip_webp_info *info_out, int *status, void *stream);
int ffhip_webp_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                            const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                            const int *orient, int *orient_out, ffhip_webp_info *info_out, int *status, void *stream);
/* ffhip_webp_decode_files_tensor_ex with the alpha record ("alpha into the tensors" above).  alpha == NULL or mode FFHIP_ALPHA_DROP: that
 * call.  Otherwise `flags` must be FFHIP_WEBP_PIXELS_LIBWEBP (the reference rule has no alpha: FFHIP_EINVAL), the files are decoded with
 * FFHIP_WEBP_ALPHA underneath -- a file without an ALPH plane is opaque, a refused plane is that file's FFHIP_EINVAL --, and the chain
 * carries alpha: the resize is ffhip_bgra_resize_items_premultiplied, the sink ffhip_bgra_to_tensor_items_alpha, told that its source is
 * premultiplied behind a resize.  alpha->source_premultiplied must be 0 (the chain sets it); outs[i] is laid out for the mode's
 * channel count.  Every check is made before anything is enqueued. */
int ffhip_webp_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                         const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                         const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                         ffhip_webp_info *info_out, int *status, void *stream);
/* Diagnostics: the items the calling thread's last ffhip_*_decode_files_tensor* call sent through ffhip_bgra_orient_items, all its parts
 * together: 0 for a batch of orientation 1 only and for the calls without orientation.  Reset where ffhip_debug_tensor_last_parts is. */
int ffhip_debug_orient_last_items(void);

/* ---- progressive JPEG (ffhip_jpeg_progressive.c, ffhip_jpeg_prog_body.h, ffhip_huff_prog_gpu.hip) ----
 * SOF2 files, decoded by ITU-T T.81 Annex G into the SAME coefficient planes a baseline file of the same quantised coefficients gives: the
 * reconstruction behind the planes is the one above, and the tests hold every file against its baseline twin.  (The reference's progressive
 * branches, format/jpg.c:255-415, 512-576, are nothing to be in parity with: DESIGN.md 2.)  Every call above keeps refusing such files; what
 * follows is opt-in.
 * Accepted: 8-bit, Huffman, 1 or 3 components in the layouts of ffhip_jpeg_probe; DC scans interleaved or not, AC scans of one component;
 * DHT and DRI redefined between scans.  FFHIP_EINVAL at parse time, before anything is decoded: arithmetic, 12-bit and lossless files, an AC
 * scan of several components, Ss = 0 with Se != 0, Se < Ss, Se > 63, a progression that breaks G.1.1.1.1 (a first scan with Ah != 0, a later
 * one whose Ah is not the previous Al or whose Al is not Ah - 1), an AC scan of a component before its DC, a DQT behind the first SOS, more
 * than FFHIP_JPEG_MAX_SCANS scans (a bound on hostile files, not on real ones), a table not yet defined, a missing EOI.  An incomplete
 * progression that ends in EOI is valid: a band never sent stays zero, bits never refined stay as they are. */
#define FFHIP_JPEG_MAX_SCANS 128
/* Host only.  ffhip_jpeg_probe for baseline files (*progressive = 0); FFHIP_OK with *progressive = 1 for an accepted progressive file.
 * progressive may be NULL. */
int ffhip_jpeg_probe_any(const uint8_t *file, size_t len, ffhip_jpeg_geom *geom, int *width, int *height, int *progressive);
/* Host only.  The outputs of ffhip_jpeg_entropy_decode in the same layout (MCU-order blocks, natural order inside a block, quant [4][64]
 * de-zigzagged) from a progressive file.  k_max (0..63) = 63 decodes every scan; a scan with Ss > k_max is skipped whole and its
 * coefficients read as zero, a scan with Ss <= k_max is decoded whole (and where such a scan is a refinement that reaches beyond k_max, the
 * scans of its band are kept too: it needs their history).  FFHIP_EINVAL for a file the parse refuses and for a malformed scan: a code that
 * matches no symbol, a DC category above 11, a refinement symbol with s other than 0 or 1, a run that carries k past Se, an EOBRUN larger
 * than the blocks left in its restart interval, more bits consumed than an interval holds, fewer restart intervals than the scan needs.
 * Nothing outside the planes is written whatever the file holds; the planes of a refused file are unspecified. */
int ffhip_jpeg_progressive_decode(const uint8_t *file, size_t len, const ffhip_jpeg_geom *expect, int16_t *coef_y, int16_t *coef_u,
                                  int16_t *coef_v, uint16_t *quant /* [4][64] */, int k_max);
/* The same ON the device, with the plane layout and contract of ffhip_jpeg_entropy_batch_gpu: n progressive files of one geometry into
 * DEVICE planes.  The host parses, unstuffs every kept scan into pinned memory and works out dependency levels (a scan waits for every
 * earlier scan of its file that shares a component and a coefficient with it); the device runs k_jpeg_huff_prog once per level over the
 * whole batch, one lane per (picture, scan, restart interval), behind one clear of the planes.  Verdicts are the host decoder's, file by
 * file, in status[] (the body is shared).  Every argument check comes before anything is enqueued; FFHIP_ENODEV on a machine without a
 * device for good arguments.  Synchronises `stream`. */
int ffhip_jpeg_progressive_batch_gpu(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_jpeg_geom *geom,
                                     int16_t *d_coef_y, int16_t *d_coef_u, int16_t *d_coef_v, uint16_t *d_quant, int k_max, int *status,
                                     void *stream);
/* ffhip_jpeg_decode_files_mixed_device (denom == NULL) / _scaled with flags.  flags = 0 is that call, byte for byte.
 * FFHIP_JPEG_ACCEPT_PROGRESSIVE: files are probed with ffhip_jpeg_probe_any, each layout class is split into its baseline files (the path
 * above, untouched) and its progressive files, and both are reconstructed by the same item kernels.  A file at 1/8, 1/4, 1/2 size is decoded
 * with k_max = 0, 4, 24 (the largest zig-zag index of the leading 1x1, 2x2, 4x4 coefficients): whole AC scans are never read.
 * FFHIP_JPEG_PROGRESSIVE_GPU=1 / =0 forces the device or the host-thread front end for the progressive files (host threads decode into
 * pinned planes, one upload); unset: host threads (DESIGN.md 4.14 says why).  A class the device front end refuses goes to host threads.
 * FFHIP_JPEG_PIXELS_LIBJPEG (below): libjpeg's pixels.  Any other flag bit: FFHIP_EINVAL. */
#define FFHIP_JPEG_ACCEPT_PROGRESSIVE 1u
int ffhip_jpeg_decode_files_mixed_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                            const int64_t *pitch, const int *denom /* may be NULL */, unsigned flags,
                                            ffhip_jpeg_geom *geom_out, int *status, void *stream);
/* ffhip_jpeg_decode_files_tensor_oriented with flags: 0 is that call; with FFHIP_JPEG_ACCEPT_PROGRESSIVE the files are probed with
 * ffhip_jpeg_probe_any and the parts are decoded by ffhip_jpeg_decode_files_mixed_device_ex, so progressive files take part in every stage
 * behind the decode (reduced size with its k_max, orientation, resize, tensor) exactly as their baseline twins do. */
int ffhip_jpeg_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                      const int *denom, int *denom_out, const int *orient, int *orient_out, unsigned flags,
                                      ffhip_jpeg_geom *geom_out, int *status, void *stream);
/* ---- JPEG pictures with libjpeg's pixels (ffhip_jpeg_libjpeg.hip) ----
 * A second, opt-in pixel rule beside the reference's: what libjpeg (and so PIL, torchvision, DALI) makes of the same coefficients, bit for
 * bit -- dequantisation to int32, the "islow" inverse DCT (13-bit constants, pass 1 descaled by 11, pass 2 by 18, + 128, clamped to
 * 0..255), "fancy" chroma upsampling (triangle filters for the ratios 2x1, 1x2 and 2x2 over the component's REAL sample grid
 * ceil(W h_c / h_max) x ceil(H v_c / v_max), a neighbour outside it being the edge sample; replication for 4x1, 1x4 and for grids at
 * most 2 samples wide) and the JFIF matrix in 16-bit fixed point (91881, 22554, 46802, 116130).  All arithmetic is 32-bit and wraps, so
 * the rule is defined for ANY int16 coefficients and uint16 quantisers, and the device equals the host functions on all of them; equal
 * to libjpeg it is for files whose coefficients come from 8-bit samples (beyond that libjpeg's own builds disagree with each other).
 * Files libjpeg would not treat as YCbCr (Adobe APP14 transform 0, component ids R, G, B, four components) are out of scope.
 * The upsampling reads neighbours across block and MCU borders and needs the display size, so these calls take it.
 *
 * Host only, no device needed:
 *   ffhip_jpeg_libjpeg_block    one block: 64 samples, natural order
 *   ffhip_jpeg_libjpeg_picture  a whole picture from HOST planes (layout of ffhip_jpeg_recon_batch, n = 1; quant uint16 [4][64]): writes the
 *                               display rectangle width x height of `bgra` (B, G, R, 0xFF; rows `pitch` bytes apart, pitch >= 4 x width).
 *                               FFHIP_EINVAL for a layout ffhip_jpeg_recon_items refuses, for a size that does not fit the geometry
 *                               (width > 8 h mcu_cols or width <= 8 h (mcu_cols - 1); likewise the height) and for NULL arguments.
 * On the device:
 *   ffhip_jpeg_recon_items_libjpeg  the items of ffhip_jpeg_recon_items plus display[i], item i's display size (it must fit the geometry as
 *                               above).  `items` and `display` are HOST arrays; every check is made before anything is enqueued (FFHIP_EINVAL,
 *                               on a machine without a device too; FFHIP_ENODEV there for good arguments).  Only enqueues on `stream`: two
 *                               launches for the whole batch (k_jpeg_idct_islow: blocks to uint8 sample planes; k_jpeg_upsample_color:
 *                               planes to BGRA) behind the records' upload; records, table and sample planes are library scratch of the
 *                               stream, the operands stream-ordered as for ffhip_jpeg_recon_items.  Inside the display rectangle the bytes
 *                               are the rule's; inside the coded picture but outside it they are written but unspecified; nothing outside
 *                               pitch x coded height is touched. */
int ffhip_jpeg_libjpeg_block(const int16_t *coef, const uint16_t *quant, uint8_t *out);
int ffhip_jpeg_libjpeg_picture(const ffhip_jpeg_geom *g, int width, int height, const int16_t *coef_y, const int16_t *coef_u, const int16_t *coef_v,
                               const uint16_t *quant, uint8_t *bgra, int64_t pitch);
int ffhip_jpeg_recon_items_libjpeg(const ffhip_jpeg_item *items, const ffhip_size *display, int n, void *stream);
/* Flag of ffhip_jpeg_decode_files_mixed_device_ex and ffhip_jpeg_decode_files_tensor_ex: the reconstruction behind every part -- the device
 * entropy decoder's, the host threads' upload, the progressive classes -- is ffhip_jpeg_recon_items_libjpeg with the probed display size.
 * Everything in front of it and behind it is unchanged.  With a denominator other than 1 (0, "choose", included): FFHIP_EINVAL for the
 * whole call, before anything is enqueued (libjpeg's reduced-size transforms are another rule). */
#define FFHIP_JPEG_PIXELS_LIBJPEG 0x10u

/* Diagnostics: the progressive files of the calling thread's last ffhip_jpeg_progressive_decode or ffhip_jpeg_progressive_batch_gpu call, or
 * its last ffhip_jpeg_decode_files_mixed_device_ex or ffhip_jpeg_decode_files_tensor_ex call (all its parts together) that passed
 * FFHIP_JPEG_ACCEPT_PROGRESSIVE -- a call of those two without the flag leaves the record as it was: out[0] progressive files, [1] scans decoded, [2] scans skipped (k_max), [3] levels launched
 * (host front end: the deepest level of each file, summed), [4] the front end taken, 0 host, 1 device (the last class's). */
int ffhip_debug_progressive_last(int out[5]);

/* ---- PNG (ffhip_inflate.c, ffhip_png.c, ffhip_png_body.h, ffhip_png_gpu.hip) ----
 * The pixel rule is the PNG specification (ISO/IEC 15948) as libpng applies it for an 8-bit RGBA output:
 *   - the picture is BGRA at width x height with the file's alpha, 255 where the file has none;
 *   - 16-bit samples become their high byte; grey at 1, 2 and 4 bits is scaled by 255, 85 and 17;
 *   - palette files take their PLTE entries, alpha from tRNS and 255 beyond its length;
 *   - tRNS on grey and RGB: the sample or the triple is compared at the file's own bit depth, alpha 0 on equality, 255 otherwise;
 *   - Adam7 files are de-interlaced, no pixel dropped; gAMA, sRGB, iCCP, bKGD and the APNG chunks are ignored (ancillary chunks are
 *     skipped by their length, without a CRC check); bytes the zlib stream holds beyond the filtered picture are ignored.
 * FFHIP_EINVAL for a file with: a CRC failure on IHDR, PLTE, tRNS, IDAT or IEND; a bad Adler-32; a zlib stream that ends short of the
 * filtered picture; a filter byte above 4; a bit depth its colour type does not have; compression, filter or interlace method bytes out
 * of range; a side of 0 or above 65535; a palette index beyond PLTE; no IEND; a critical chunk other than the four. */
/* Host only.  A zlib-wrapped deflate stream (CM 8, window up to 32 KiB, no preset dictionary; stored, fixed and dynamic blocks) into
 * dst[0 .. cap); *out_len receives the bytes written.  FFHIP_EINVAL for everything it refuses: a bad header or check value, a stream
 * that ends early, over-subscribed code lengths (an incomplete set only as the one-code distance tree zlib accepts), a distance beyond
 * the start of the output, symbols deflate does not have, output beyond cap.  Reads nothing outside src[0 .. len). */
int ffhip_inflate(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len);
typedef struct ffhip_png_info {
    int32_t width, height, bit_depth, color_type, interlace;
    int32_t has_trns;        /* a tRNS chunk that counts: in front of IDAT, of the colour type's length */
    int32_t palette_size;    /* PLTE entries of a colour type 3 file, else 0 */
    int32_t n_passes;        /* sub-images with pixels: 1, or up to 7 of an Adam7 file */
    uint64_t filtered_bytes; /* what the zlib stream has to hold: every pass's rows x (1 + row bytes) */
    int32_t pass_rows[7], pass_row_bytes[7]; /* by Adam7 pass ([0] alone: not interlaced); 0 rows for a pass without pixels */
} ffhip_png_info;
/* Host only, cheap: the header (its CRC checked) and the chunks up to the first IDAT walked by their lengths (no CRC). */
int ffhip_png_probe(const uint8_t *file, size_t len, ffhip_png_info *info);
/* Host only, no device needed: the whole decode into bgra (pitch >= 4 x width), by the functions the kernels compile. */
int ffhip_png_picture(const uint8_t *file, size_t len, uint8_t *bgra, int64_t pitch);
/* As ffhip_jpeg_exif_orientation, from the file's eXIf chunk (the TIFF structure, without "Exif\0\0"). */
int ffhip_png_exif_orientation(const uint8_t *file, size_t len, int *orientation);
/* PNG files of any sizes and kinds in one call: shape and per-file contract of ffhip_webp_decode_files_device.  d_bgra[i] (16-byte aligned,
 * pitch[i] >= 4 x width, a multiple of 16) receives file i's width x height BGRA pixels and nothing else.  Host threads walk the chunks,
 * check the CRCs and inflate straight into pinned staging; k_png_unfilter undoes the row filters (one launch per level of 64 rows) and
 * k_png_expand writes the pictures.  The batch goes in PARTS of at most 1 GiB of filtered bytes (FFHIP_PNG_PART_BYTES replaces the figure),
 * a larger file a part of its own.  status[i] receives each file's code; a refused file writes nothing and every other file is delivered;
 * returns the first failure.  Argument checks come before anything is enqueued: FFHIP_EINVAL for NULL arrays, then FFHIP_ENODEV.
 * Synchronises `stream`. */
int ffhip_png_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                  const int64_t *pitch, ffhip_png_info *info_out, int *status, void *stream);
/* Files to tensors, as ffhip_webp_decode_files_tensor_ex: the display picture is width x height, alpha is dropped by the three-channel
 * sink (ffhip_png_decode_files_tensor_alpha keeps it); out_size == NULL: no resize; orient[i] 1..8, or 0 for the file's eXIf tag,
 * orient == NULL: every file's tag; flags must be 0. */
int ffhip_png_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                  const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                  const int *orient, int *orient_out, unsigned flags, ffhip_png_info *info_out, int *status, void *stream);
/* The same with the alpha record ("alpha into the tensors"): alpha == NULL or mode FFHIP_ALPHA_DROP is the call above; otherwise tRNS and
 * the alpha of colour types 4 and 6 reach the tensors as the mode says, through ffhip_bgra_resize_items_premultiplied where there is a
 * resize.  alpha->source_premultiplied must be 0; outs[i] is laid out for the mode's channel count. */
int ffhip_png_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                        const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                        const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                        ffhip_png_info *info_out, int *status, void *stream);
/* Diagnostics: parts and unfilter levels (launches of k_png_unfilter) of the calling thread's last ffhip_png_decode_files_device. */
int ffhip_debug_png_last(int out[2]);
/* Diagnostics (tests/tools/bench_png.py): milliseconds of that call's stages, all its parts together -- [0] the host threads' chunk walk
 * and inflate (wall clock), and, measured by events only while FFHIP_PNG_TIMES is set (0 otherwise), [1] the upload, [2] k_png_unfilter
 * over all its levels, [3] k_png_expand. */
int ffhip_debug_png_times(double out[4]);

/* ---- PNG, inflate on the device (ffhip_inflate_body.h, ffhip_inflate_model.c, ffhip_inflate_gpu.hip) ----
 * Opt-in: every default keeps its bytes, its stages and its timings.  k_inflate gives one wave to one zlib stream: the serial decode is
 * wave-uniform, the wave stores a run of literals or 64 bytes of a match at a time, and the output itself is the window. */
/* n zlib streams in host memory into n DEVICE buffers, in one launch: the rule, stream for stream, is ffhip_inflate's.  d_dst[i] takes
 * cap[i] bytes (cap[i] == 0 with a NULL d_dst[i] is allowed); out_len[i] and status[i] receive what ffhip_inflate would have given, and
 * the return value is the first non-zero status[i].  Nothing beyond out_len[i] bytes of a destination is written; the bytes of a
 * refused stream's destination are unspecified inside cap[i] and untouched outside it.  FFHIP_EINVAL for n < 0, a NULL array, a NULL
 * src[i] with len[i] > 0 or a NULL d_dst[i] with cap[i] > 0; then FFHIP_ENODEV; both before the first allocation.  n == 0 is FFHIP_OK.
 * Uploads, launches, reads the verdicts back and synchronises `stream`; the staging is the PNG file call's (one call of either at a
 * time per stream). */
int ffhip_inflate_streams_device(const uint8_t *const *src, const size_t *len, int n, uint8_t *const *d_dst, const size_t *cap,
                                 size_t *out_len, int *status, void *stream);
/* png_flags of the two calls below.  FFHIP_PNG_INFLATE_DEVICE: the host threads walk the chunks and check the CRCs as ever, then copy
 * every file's IDAT payloads, joined, into the pinned staging instead of inflating them; one upload carries streams, palettes and
 * records; k_inflate writes the filtered pictures where the host path's upload would have put them and checks every row's filter byte;
 * one copy back and one synchronisation bring the verdicts; k_png_unfilter and k_png_expand run on the files that are still clean.  A
 * palette file whose palette is shorter than its depth's range is inflated by the host threads as ever (its indices are checked on
 * unfiltered rows) and its filtered bytes go up with the rest.  Per-file codes, pictures, "a refused file writes nothing", the cut into
 * parts (the budget sums filtered bytes) and ffhip_debug_png_last are those of the host path.  The switch FFHIP_PNG_INFLATE_GPU=1 sets
 * the bit for every PNG file entry, the ones above included. */
#define FFHIP_PNG_INFLATE_DEVICE 0x1u
/* ffhip_png_decode_files_device with png_flags: 0 is that call byte for byte; unknown bits are FFHIP_EINVAL. */
int ffhip_png_decode_files_device_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                     const int64_t *pitch, ffhip_png_info *info_out, int *status, unsigned png_flags, void *stream);
/* ffhip_png_decode_files_tensor_alpha with png_flags (alpha == NULL: the three-channel call); flags must be 0 as there. */
int ffhip_png_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                     const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                     const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                     unsigned png_flags, ffhip_png_info *info_out, int *status, void *stream);
/* Diagnostics, all parts of the calling thread's last PNG file call: [0] files inflated on the device, [1] files inflated on the
 * host, [2] compressed bytes uploaded, [3] milliseconds of k_inflate plus the copy back, measured by events only while FFHIP_PNG_TIMES is
 * set (0 otherwise) and not part of ffhip_debug_png_times' [1] .. [3]. */
int ffhip_debug_png_inflate(double out[4]);

/* ---- lossless WebP (ffhip_vp8l.c, ffhip_vp8l_body.h, ffhip_vp8l_gpu.hip) ----
 * The reference has a stub here, so the pixel rule is libwebp's: the BGRA picture is width x height of the VP8L header, sample for sample
 * what PIL's Image.open(f).convert("RGBA") gives (libwebp 1.6.0).  Every line below was held against it (tests/test_vp8l_spec.py):
 *   - container: RIFF/WEBP, chunks padded to even sizes, walked up to the first VP8L; a VP8X chunk in front is accepted when its canvas
 *     equals the VP8L header's size and refused otherwise; bytes behind the RIFF size, and bytes of the chunk behind the stream's last bit,
 *     are not looked at; a RIFF size beyond the file is refused;
 *   - header: 0x2f, 14 bits width - 1, 14 bits height - 1, alpha_is_used, a 3-bit version that must be 0;
 *   - alpha is the file's where alpha_is_used is set and 255 otherwise, whatever the stream's samples and whatever the VP8X alpha flag;
 *     colour under alpha 0 is kept as stored;
 *   - transforms: at most one of each type, in any order, undone last to first; each works at the width left by the colour-indexing
 *     transforms in front of it (2, 4 or 8 pixels to a word for palettes of up to 16, 4 and 2 entries); a type given twice is refused;
 *   - predictor: the mode of a block is green & 15 of its pixel, 14 and 15 act as 0 (0xff000000); the 14 modes of the format text; Select
 *     returns L when sum|T - TL| < sum|L - TL| over the four channels, else T; mode 13's half difference truncates toward zero; pixel
 *     (0,0) is predicted by 0xff000000, the rest of row 0 by L, column 0 by T; the TR of a row's last pixel is the first pixel of the
 *     current row;
 *   - cross-colour: the block's pixel holds green_to_red, green_to_blue, red_to_blue in bits 0..7, 8..15, 16..23, signed; a delta is
 *     (multiplier x colour) >> 5; blue takes the red already corrected;
 *   - colour indexing: the palette is stored as differences, per byte, to the entry before; an index beyond the palette gives 0x00000000;
 *   - prefix codes: canonical, written MSB first into the LSB-first stream; code-length code order 17,18,0,1,..5,16,6,..15; repeat symbols
 *     16 (the last non-zero length, 8 at the start, 3..6 times), 17 (zeros, 3..10), 18 (zeros, 11..138), a repeat beyond the alphabet
 *     refused; max_symbol counts the code-length tokens read and is refused beyond the alphabet; a code of ONE symbol, in the simple form
 *     or not, reads no bits; any other code must be complete; a simple code's symbol beyond its alphabet is dropped, which leaves a code
 *     of no symbols: refused;
 *   - five codes a group (green + length prefixes + cache, red, blue, alpha, distance), read green, red, blue, alpha; the meta prefix
 *     image (the picture itself only) gives a block's group in bits 8..23 of its pixel, and a pixel's group is that of its own position,
 *     behind a copy too;
 *   - a length or distance prefix below 4 is value - 1; else extra = (p - 2) >> 1, value = ((2 + (p & 1)) << extra) + bits(extra) + 1;
 *     distance codes 1..120 are libwebp's (dx, dy) table with dist = max(dx + dy x xsize, 1), code k > 120 is k - 120; copies may overlap
 *     their own output; a distance beyond the pixels decoded, or a length beyond the image's end, is refused;
 *   - colour cache: 1..11 bits (0 and 12..15 refused), key (0x1e35a7bd x argb) >> (32 - bits), every pixel -- literal, copied or a cache
 *     hit -- enters it in order;
 *   - a stream that has been asked for a bit behind its chunk's end is refused.
 * FFHIP_EINVAL for everything refused above, for a file that is not RIFF/WEBP or has no VP8L chunk, and for a lossy file (`VP8 `);
 * FFHIP_EWEBP_ANIMATION for the VP8X animation flag or an ANIM / ANMF chunk in front.  No read goes outside file[0 .. len). */
typedef struct ffhip_vp8l_info {
    int32_t width, height, has_alpha;
    int32_t n_transforms, transforms[4]; /* the types in the file's order: 0 predictor, 1 cross-colour, 2 add-green, 3 colour indexing */
    int32_t predictor_bits, cross_bits;  /* block size bits 2..9; 0 without the transform */
    int32_t palette_size, pixels_per_word; /* 0 and 1 without colour indexing */
    int32_t cache_bits, has_meta;        /* of the residual image: its colour cache (0: none), whether it has a meta prefix image */
    int32_t residual_width;              /* the width the entropy-coded image has: width, or the packed width */
} ffhip_vp8l_info;
/* Host only, cheap: the container and the 5-byte header.  has_alpha: the alpha_is_used bit. */
int ffhip_vp8l_probe(const uint8_t *file, size_t len, int *width, int *height, int *has_alpha);
/* Host only, no device needed: the whole decode into bgra (pitch >= 4 x width), the transforms undone by the functions the kernels
 * compile. */
int ffhip_vp8l_picture(const uint8_t *file, size_t len, uint8_t *bgra, int64_t pitch);
/* Host only: the header and the transform list read (their sub-images decoded), and the residual image's first two fields. */
int ffhip_vp8l_read_info(const uint8_t *file, size_t len, ffhip_vp8l_info *info);
/* Lossless WebP files of any sizes in one call: shape and per-file contract of ffhip_png_decode_files_device.  d_bgra[i] (16-byte aligned,
 * pitch[i] >= 4 x width, a multiple of 16) receives file i's width x height BGRA pixels and nothing else.  Host threads decode the prefix
 * codes, copies and colour cache straight into pinned staging -- a file's RESIDUAL image and the block images beside it; k_vp8l_predict
 * undoes the predictor in place (one launch per level of 64 rows), k_vp8l_finish undoes the pointwise transforms behind it, expands a
 * palette and writes the pictures.  A file whose colour indexing is not its first transform is inverted by the host threads and uploaded
 * as pixels.  The batch goes in PARTS of at most 1 GiB of residual bytes (FFHIP_VP8L_PART_BYTES replaces the figure), a larger file a part
 * of its own.  status[i] receives each file's code; a refused file writes nothing and every other file is delivered; returns the first
 * failure.  Argument checks come before anything is enqueued: FFHIP_EINVAL for NULL arrays, then FFHIP_ENODEV.  Synchronises `stream`. */
int ffhip_vp8l_decode_files_device(const uint8_t *const *files, const size_t *lens, int n, int n_threads, uint8_t *const *d_bgra,
                                   const int64_t *pitch, ffhip_vp8l_info *info_out, int *status, void *stream);
/* Files to tensors, as ffhip_png_decode_files_tensor: the display picture is width x height, alpha is dropped by the three-channel sink
 * (ffhip_vp8l_decode_files_tensor_alpha keeps it); out_size == NULL: no resize; orient[i] 1..8, or 0 for the file's EXIF chunk
 * (ffhip_webp_exif_orientation), orient == NULL: every file's tag; flags must be 0. */
int ffhip_vp8l_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                   const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                   const int *orient, int *orient_out, unsigned flags, ffhip_vp8l_info *info_out, int *status, void *stream);
/* The same with the alpha record, as ffhip_png_decode_files_tensor_alpha: a file whose alpha_is_used bit is clear delivers alpha 255. */
int ffhip_vp8l_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                         const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                         const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                         ffhip_vp8l_info *info_out, int *status, void *stream);
/* Diagnostics: parts, launches of k_vp8l_predict, and files inverted on the host, of the calling thread's last
 * ffhip_vp8l_decode_files_device. */
int ffhip_debug_vp8l_last(int out[3]);
/* Diagnostics (tests/tools/bench_vp8l.py): milliseconds of that call's stages, all its parts together -- [0] the host threads' stream
 * decode (wall clock), and, measured by events only while FFHIP_VP8L_TIMES is set (0 otherwise), [1] the upload, [2] k_vp8l_predict over
 * all its levels, [3] k_vp8l_finish. */
int ffhip_debug_vp8l_times(double out[4]);

/* ---- JPEG encoding (ffhip_jpeg_enc.c, ffhip_jpeg_enc_body.h, ffhip_jpeg_enc_gpu.hip) ----
 * Device pictures to baseline JPEG files, byte for byte what libjpeg writes after jpeg_set_quality(q, force_baseline) with its defaults
 * (islow forward DCT, Annex K Huffman tables, no optimisation) -- so PIL's Image.save and torchvision's encode_jpeg.  THE RULE, integers only:
 *  1. Quantiser tables.  q clamped to 1..100; s = 5000 / q for q < 50, else 200 - 2 q; t = clamp((std s + 50) / 100, 1, 255) over Annex K's
 *     luma and chroma tables (T.81 K.1, K.2).  Slot 0 is luma, slot 1 chroma.
 *  2. Colour.  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
 *     Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.  Grey sources skip this step.
 *  3. Edges and chroma -- NOT symmetric.  Horizontally a full-resolution sample beyond the last column is the last column, out to the MCU
 *     width, before downsampling.  Vertically full-resolution rows are replicated only up to a multiple of v; the plane is then downsampled,
 *     and the chroma rows still missing up to the MCU height are copies of the last DOWNSAMPLED row.  h2v2: (a + b + c + d + bias) >> 2 with
 *     bias 1, 2, 1, 2, .. along an output row, from 1 in every row; h2v1: (a + b + bias) >> 1 with bias 0, 1, 0, 1, ...
 *  4. Luma blocks.  Blocks bx < ceil(W / 8), by < ceil(H / 8) are real, computed from the edge-replicated plane.  The other luma blocks of a
 *     last MCU are dummy blocks: all AC coefficients 0, the DC the quantised DC of the previous block in the MCU's block order (after that
 *     block's own substitution).  Chroma is padded as samples by step 3 and has no dummy blocks.
 *  5. Forward DCT, jfdctint.c: samples minus 128; the row pass keeps PASS1_BITS = 2 (outputs 0 and 4 shifted left by 2, the others
 *     DESCALE(.., 11)); the column pass gives outputs 0 and 4 as DESCALE(.., 2), the others DESCALE(.., 15); DESCALE(x, n) =
 *     (x + (1 << (n - 1))) >> n; constants 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172; 32-bit arithmetic.
 *  6. Quantise: with d = 8 t, c = sign(x) ((|x| + (d >> 1)) / d).
 *  7. Entropy coding, T.81 F.1.2 with Annex K's four tables: a DC prediction per component, reset at every restart interval; `restart`
 *     counts MCUs (0: none); an interval's last byte is padded with ones; markers FFD0 + (k & 7); 00 stuffed behind every FF of entropy data.
 *  8. File: SOI; APP0 "JFIF\0" 1.1, units 0, density 1 x 1, no thumbnail; one DQT segment per table; SOF0 with component ids 1, 2, 3; four
 *     DHT segments DC0, AC0, DC1, AC1 (grey: one DQT, two DHT); DRI if restart != 0; SOS; the scan; EOI.
 * Layouts: 4:4:4, 4:2:2 (h2v1), 4:2:0 (h2v2) and grey; sizes 1..65535; restart 0..65535.  Anything else is FFHIP_EINVAL.
 *
 * A source picture is uint8 samples addressed by byte strides: sample c of pixel (x, y) at pixels + y row_stride + x pixel_stride + chan[c],
 * chan = the offsets of R, G, B (channels = 3: CHW, HWC, RGB and BGR tensors are all this one form) or of the one grey sample (channels =
 * 1, the grey layout's only source, and that layout takes no other); or channels = 4: a BGRA picture as the decoders leave it (pixel_stride
 * 4, row_stride the pitch, a multiple of 4, pixels 4-byte aligned, chan ignored), read a pixel a load.  Strides may be negative. */
#define FFHIP_JPEG_ENC_444 0
#define FFHIP_JPEG_ENC_422 1
#define FFHIP_JPEG_ENC_420 2
#define FFHIP_JPEG_ENC_GREY 3
#define FFHIP_EJPEG_NOSPACE (-1101) /* the file does not fit cap: len is the size it needs, nothing at or beyond cap was written */
#define FFHIP_EJPEG_RANGE (-1102)   /* a coefficient Annex K's tables cannot code: an AC magnitude over 1023 or a DC difference beyond +-2047 */
typedef struct ffhip_jpeg_source {
    const uint8_t *pixels;
    int64_t row_stride, pixel_stride; /* bytes */
    int64_t chan[3];
    int32_t channels;                 /* 3, 1, or 4 (BGRA) */
    int32_t width, height;
    int32_t reserved;                 /* 0 */
} ffhip_jpeg_source;
/* Host only, no device needed; what the device calls are held to:
 *   ffhip_jpeg_encode_tables   step 1: quant[2][64], natural order
 *   ffhip_jpeg_encode_block    steps 5 and 6 on 64 samples, natural order in and out
 *   ffhip_jpeg_encode_header   step 8 up to and including SOS: *len = its size (at most FFHIP_JPEG_ENC_HEADER_MAX), written if it fits cap
 *                              (else FFHIP_EJPEG_NOSPACE and nothing written)
 *   ffhip_jpeg_encode_bound    a CERTAIN bound on the file's size, 0 for bad arguments.  A block takes at most 1660 bits: a DC code of up
 *                              to 11 bits (Annex K's longest, chroma's size 11) and 11 bits of magnitude, and 63 AC coefficients of a
 *                              16-bit code and 10 bits of magnitude each (a ZRL only ever stands for coefficients that take nothing).  An
 *                              interval of b blocks is at most ceil(1660 b / 8) bytes, padding included; stuffing at most doubles them (every
 *                              byte FF); each interval ends in a two-byte marker (RSTn, or EOI).  So
 *                                bound = header + sum over intervals (2 ceil(1660 b / 8) + 2)
 *   ffhip_jpeg_encode_picture  a whole picture from HOST pixels to the file's bytes, through the same bodies as the kernels.  *len = the
 *                              file's size; FFHIP_EJPEG_NOSPACE when it exceeds cap (no byte at or beyond out + cap is written; what lies
 *                              below is unspecified then). */
#define FFHIP_JPEG_ENC_HEADER_MAX 640
int ffhip_jpeg_encode_tables(int quality, uint16_t *quant);
int ffhip_jpeg_encode_block(const uint8_t *samples, const uint16_t *quant, int16_t *coef);
int ffhip_jpeg_encode_header(int width, int height, int layout, int quality, int restart, uint8_t *out, size_t cap, size_t *len);
size_t ffhip_jpeg_encode_bound(int width, int height, int layout, int restart);
int ffhip_jpeg_encode_picture(const ffhip_jpeg_source *src, int layout, int quality, int restart, uint8_t *out, size_t cap, size_t *len);
/* On the device, in three calls.  `items` are HOST arrays, read before the call returns; every check is made before anything is enqueued
 * (FFHIP_EINVAL, on a machine without a device too; FFHIP_ENODEV there for good arguments); records, tables, sample planes and streams are
 * library scratch of the stream.
 *
 * ffhip_jpeg_fdct_items: pixels to quantised coefficients (steps 1 to 6), the other direction of ffhip_jpeg_recon_items_libjpeg.  Only
 *   enqueues: k_jpeg_color_downsample (a thread takes the 8 h x v pixels over 8 chroma samples of a row: the source to padded uint8 sample
 *   planes), then k_jpeg_fdct_islow (a thread takes one block, dummy blocks included, both passes in registers).  d_coef_*: int16, 64 a block,
 *   natural order, blocks in MCU order -- the plane layout ffhip_jpeg_recon_items reads, for the geometry mcu_cols = ceil(W / 8 h),
 *   mcu_rows = ceil(H / 8 v); 16-byte aligned; d_coef_u and d_coef_v NULL for grey.  At most 2^31 - 1 blocks a picture.  The source is
 *   stream-ordered, like the planes. */
typedef struct ffhip_jpeg_fdct_item {
    ffhip_jpeg_source src; /* pixels: device */
    int32_t layout, quality;
    int16_t *d_coef_y, *d_coef_u, *d_coef_v;
} ffhip_jpeg_fdct_item;
int ffhip_jpeg_fdct_items(const ffhip_jpeg_fdct_item *items, int n, void *stream);
/* ffhip_jpeg_huff_encode_items: coefficient planes in that layout -- from the call above or from anywhere else -- to whole files (steps 7
 *   and 8; quality only names the header's tables).  d_out[0, cap) receives the file; len_out[i] (host) its size; status[i] (host) FFHIP_OK,
 *   FFHIP_EJPEG_RANGE (the file is unspecified, within cap) or FFHIP_EJPEG_NOSPACE (len_out[i] is the size the file needs; no byte at or
 *   beyond cap is written).  An item's verdict leaves its neighbours alone.  Returns the first item's code that is not FFHIP_OK, else
 *   FFHIP_OK.  Kernels: a thread per block counts its bits (its DC predecessor is read from the planes: nothing is carried); a workgroup per
 *   picture turns the counts into positions with a prefix scan in a loop of its own; a thread per block writes its bits into the zeroed
 *   unstuffed stream (first and last word by atomicOr, the words between by plain stores; an interval's last block adds the padding and the
 *   marker); a workgroup per KiB of that stream counts the FF bytes to stuff; a workgroup per picture sums those; a last kernel copies
 *   header and stuffed stream into d_out.  No kernel waits for another workgroup; every loop runs to a bound known at its entry.
 *   LIMIT: a picture whose ffhip_jpeg_encode_bound reaches 2^32 bytes (some 10.3 M blocks: 220 Mpixel at 4:4:4, 440 at 4:2:0) is FFHIP_EINVAL
 *   here and in ffhip_jpeg_encode_items, though its sizes lie in 1..65535: chunk indices and FF counts are held in 32 bits.
 *   The host entries have no such limit.
 *   The call SYNCHRONISES the stream twice: once behind the positions, to size the streams' scratch by the counted totals and not by the
 *   bound, and once at its end, for len_out and status. */
typedef struct ffhip_jpeg_huff_item {
    int32_t width, height, layout, quality, restart;
    const int16_t *d_coef_y, *d_coef_u, *d_coef_v;
    uint8_t *d_out;
    size_t cap;
} ffhip_jpeg_huff_item;
int ffhip_jpeg_huff_encode_items(const ffhip_jpeg_huff_item *items, int n, size_t *len_out, int *status, void *stream);
/* ffhip_jpeg_encode_items: the file call -- pictures of any sizes, layouts, qualities and restart intervals in one batch.  The batch is cut
 *   into parts by a byte budget over the coefficient planes (1 GiB; a picture beyond it is a part of its own); a part is one
 *   ffhip_jpeg_fdct_items into library scratch and one ffhip_jpeg_huff_encode_items, so the call synchronises the stream twice a part.
 *   len_out, status, the return value and the LIMIT on a picture's bound as above. */
typedef struct ffhip_jpeg_encode_item {
    ffhip_jpeg_source src; /* pixels: device */
    int32_t layout, quality, restart, reserved;
    uint8_t *d_out;
    size_t cap;
} ffhip_jpeg_encode_item;
int ffhip_jpeg_encode_items(const ffhip_jpeg_encode_item *items, int n, size_t *len_out, int *status, void *stream);

/* ---- PNG encoding (ffhip_png_enc.c, ffhip_png_enc_body.h, ffhip_png_enc_gpu.hip; ffhip_deflate.c, ffhip_deflate_body.h,
 *      ffhip_deflate_gpu.hip) ----
 * Pictures to complete PNG files, lossless: the filters and deflate as kernels, the same bodies as host functions.  THE RULE, which host and
 * device share so that their files are equal byte for byte:
 *   PICTURES  8 bits a sample; colour type 0, 4, 2, 6 for 1, 2, 3, 4 channels (grey, grey + alpha, RGB, RGBA); not interlaced; sides 1..65535.
 *             The file: signature, IHDR, the IDAT chunks, IEND; no ancillary chunk.
 *   FILTERS   filter 0..4: that type on every row.  FFHIP_PNG_FILTER_ADAPTIVE: per row the type whose filtered bytes, read as signed 8-bit,
 *             have the smallest sum of absolute values, the lowest type at equal sums.  The row above row 0 and the bpp = channels bytes
 *             left of a row are zeros.  A filtered row is the type byte and width x channels bytes; the filtered picture is the rows end to end.
 *   ZLIB      header 78 01.  The filtered picture is cut into chunks of FFHIP_DEFLATE_CHUNK bytes (the last one shorter; an empty input is one
 *             empty chunk).  A chunk becomes ONE deflate block: dynamic Huffman, or stored when the dynamic block is not shorter in bytes (an
 *             empty chunk is stored).  A chunk starts at a byte boundary: every chunk but the last is followed by an empty stored block (three
 *             zero header bits behind the block's last bit, zeros to the byte boundary, 00 00 FF FF); the last chunk's block has BFINAL and
 *             is padded with zeros.  The Adler-32 of the input, big-endian, ends the stream.
 *   PARSE     within a chunk, by steps of 64 positions.  Position p (its match may be min(258, bytes left in the chunk) long) tries, in this
 *             order, distances 1, 2, 3, 4 (where the stream has that many bytes in front of p, earlier chunks included; a match of 3 or more
 *             counts) and then, when 4 bytes are left, the LATEST position of an EARLIER step of this chunk whose 4 bytes have the same hash
 *             ((little-endian word x 2654435761) >> 20; a match of 4 or more counts).  The longest wins, the first tried among equals;
 *             a position a token of an earlier step covers tries nothing.  Then greedy: from the first uncovered position, a position
 *             with a match emits it and skips its length, any other emits its byte.  Length 258 is symbol 285.
 *   CODES     frequencies of the chunk's tokens, end-of-block once.  Lengths: Huffman's algorithm on the used symbols sorted by (frequency,
 *             symbol), two queues, leaf before inner node at equal weight; while a length exceeds the limit (15, and 7 for the code-length
 *             alphabet) every used frequency becomes (f + 1) / 2 and the tree is built again.  One used symbol gets one bit; a block without
 *             a match has one distance code (symbol 0) of one bit.  HLIT, HDIST, HCLEN are the smallest the lengths allow.  The lengths of
 *             both alphabets, as one sequence, are run-length coded run by run of equal values: a non-zero value once, then 16 for 6, ...,
 *             3 of the rest, then singly; zeros by 18 for 138 .. 11, then 17 for 10 .. 3, then singly.  Codes are canonical.
 *   CHUNKS    one IDAT per deflate chunk (the first holds the zlib header in front), then an IDAT of the four Adler bytes, then IEND.
 * Every choice is a function of the input bytes alone. */
#define FFHIP_DEFLATE_CHUNK 16384
#define FFHIP_PNG_FILTER_ADAPTIVE 5
#define FFHIP_EPNG_NOSPACE (-1201)     /* the file does not fit cap: len is the size it needs, nothing at or beyond cap was written */
#define FFHIP_EDEFLATE_NOSPACE (-1202) /* the same for a zlib stream */
/* A uint8 picture by byte strides, either of which may be negative: sample c of pixel (x, y) is pixels[y row_stride + x pixel_stride +
 * chan[c]], c in file order (grey, A / R, G, B, A).  A BGRA picture as the decoders leave it: pixel_stride 4, chan {2, 1, 0, 3}; with
 * channels 3 and chan {2, 1, 0} its alpha is dropped.  Strides and offsets lie within +-2^30; reserved 0. */
typedef struct ffhip_png_source {
    const uint8_t *pixels;
    int64_t row_stride, pixel_stride;
    int64_t chan[4];
    int32_t channels, width, height, reserved;
} ffhip_png_source;
/* Host entries; they need no device.
 *   ffhip_deflate              src[0, len) to a zlib stream under the rule: *out_len its size; FFHIP_EDEFLATE_NOSPACE when that exceeds cap (no
 *                              byte at or beyond dst + cap is written)
 *   ffhip_deflate_bound        a CERTAIN bound: 2 + len + 4, 5 bytes a chunk for the stored form, 5 for each empty stored block between chunks
 *   ffhip_deflate_code_lengths the length rule alone: n <= 288 frequencies (their sum below 2^32), limit 1..15 with 2^limit >= n
 *   ffhip_png_filtered_size    height x (1 + width x channels), 0 for bad arguments
 *   ffhip_png_filter_picture   the filtered picture, ffhip_png_filtered_size bytes (*len; FFHIP_EPNG_NOSPACE and nothing written when that
 *                              exceeds cap); filter 0..4 or FFHIP_PNG_FILTER_ADAPTIVE
 *   ffhip_png_encode_bound     a CERTAIN bound on the file, 0 for bad arguments: 33 bytes of signature and IHDR, 12 an IDAT, the deflate bound
 *                              of the filtered size, 12 for the IDAT around the Adler-32, 12 of IEND
 *   ffhip_png_encode_picture   HOST pixels to the file; *len its size; FFHIP_EPNG_NOSPACE when that exceeds cap (no byte at or beyond out + cap
 *                              is written) */
int ffhip_deflate(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len);
size_t ffhip_deflate_bound(size_t len);
int ffhip_deflate_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *lengths);
size_t ffhip_png_filtered_size(int width, int height, int channels);
int ffhip_png_filter_picture(const ffhip_png_source *src, int filter, uint8_t *out, size_t cap, size_t *len);
size_t ffhip_png_encode_bound(int width, int height, int channels);
int ffhip_png_encode_picture(const ffhip_png_source *src, int filter, uint8_t *out, size_t cap, size_t *len);
/* On the device.  The arrays are HOST arrays, read before the call returns; every check is made before anything is enqueued (FFHIP_EINVAL, on
 * a machine without a device too; FFHIP_ENODEV there for good arguments); n == 0 is FFHIP_OK.  Kernels: k_png_filter (a wave per row: the five
 * sums by a wave reduction, the row above read from the source again, 16-byte stores inside the row), k_deflate_chunks (a workgroup of one
 * wave per chunk: the body above, head table in LDS, tokens in scratch), a workgroup per picture or stream that scans the chunks' sizes,
 * joins the Adler parts and writes the verdict, and a copy kernel with every store under cap.  No kernel waits for another workgroup.
 * Sizes are held in 32 bits: an input whose bound reaches 2^32 bytes is FFHIP_EINVAL in both calls (the host entries have no such limit).
 *
 * ffhip_deflate_streams_device: n DEVICE buffers d_src[i][0, len[i]) to n zlib streams in d_dst[i][0, cap[i]), the twin of
 *   ffhip_inflate_streams_device.  out_len[i], status[i] (FFHIP_OK or FFHIP_EDEFLATE_NOSPACE: out_len[i] is the size needed, no byte at or
 *   beyond cap[i] is written) as ffhip_deflate gives them; a stream's verdict leaves its neighbours alone; returns the first code that is
 *   not FFHIP_OK.  SYNCHRONISES the stream once a part (below), at the part's end. */
int ffhip_deflate_streams_device(const uint8_t *const *d_src, const size_t *len, int n, uint8_t *const *d_dst, const size_t *cap,
                                 size_t *out_len, int *status, void *stream);
/* ffhip_png_encode_items: pictures of any sizes, channel counts and source forms in one batch, byte for byte ffhip_png_encode_picture's
 *   files.  The batch is cut into parts by a byte budget over the filtered bytes (256 MiB -- a filtered byte takes six of scratch -- and at
 *   most 4096 pictures; a picture beyond the budget is a part of its own); the call SYNCHRONISES the stream once a part.  len_out, status
 *   (FFHIP_OK or FFHIP_EPNG_NOSPACE) and the return value as above.  ffhip_deflate_streams_device cuts its streams by the same budget and
 *   synchronises once a part too. */
typedef struct ffhip_png_encode_item {
    ffhip_png_source src; /* pixels: device */
    int32_t filter, reserved;
    uint8_t *d_out;
    size_t cap;
} ffhip_png_encode_item;
int ffhip_png_encode_items(const ffhip_png_encode_item *items, int n, size_t *len_out, int *status, void *stream);

/* ---- Lossless WebP encoding (ffhip_vp8l_enc.c, ffhip_vp8l_enc_body.h, ffhip_vp8l_enc_gpu.hip) ----
 * Pictures to complete lossless WebP files (RIFF / WEBP / VP8L): transforms, parse and prefix codes as kernels, the same body as host
 * functions.  There is no byte-for-byte target outside the library: THE RULE is its own, a function of the input bytes alone, and host and
 * device share it so that their files are equal byte for byte.
 *   PICTURES    8 bits a sample, 1..4 channels (grey, grey + alpha, RGB, RGBA) by byte strides, sides 1..16384.  A pixel is the ARGB word
 *               alpha << 24 | red << 16 | green << 8 | blue; grey is R = G = B, a missing alpha 255.  The header's alpha bit is set for 2
 *               and 4 channels, its version is 0.  Colour under transparent pixels is kept.  The file: "RIFF", its size, "WEBP", "VP8L",
 *               the chunk's size, the byte 2F, the bits; a zero byte behind an odd chunk, so the file's size is even.
 *   TRANSFORMS  flags FFHIP_VP8L_ENC_SUBTRACT_GREEN and FFHIP_VP8L_ENC_PREDICT, either, both or none.  With both, green is subtracted from
 *               red and blue first and prediction runs over that picture; the file lists them in this order.  With none the ARGB words are
 *               coded as they are.  Prediction has square tiles of 1 << FFHIP_VP8L_ENC_TILE_BITS pixels.  A tile's mode 0..13 is the one with
 *               the smallest sum, over the tile's pixels and their four channels, of the absolute values of the residual bytes (pixel less
 *               prediction, modulo 256) read as signed; the lowest mode at equal sums.  What the format fixes counts the same for every mode:
 *               the first pixel against FF000000, the top row from the left, the left column from above; the rightmost pixel's top-right
 *               neighbour is its row's first pixel.  Neighbours are the (green-subtracted) source's own pixels.  The sub-image holds one
 *               pixel a tile, FF000000 | mode << 8, coded as literals.
 *   PARSE       the residual picture in scan order is cut into chunks of FFHIP_VP8L_ENC_CHUNK pixels, the last one shorter; a chunk is parsed
 *               without another chunk's tokens, by steps of 64 positions.  A position tries distance 1, then distance width (the pixel above;
 *               with width 1 the two are one candidate), where the picture has that many pixels in front of it, earlier chunks' included; a
 *               match may run to the chunk's end and counts from 3 pixels on.  The longest wins, the first tried among equals; a position a
 *               token of an earlier step covers tries nothing.  Then greedy: from the first uncovered position, a position with a match emits
 *               it and skips its length, any other emits its word as a literal.  The distance codes are the smallest that decode to the
 *               distance: 1 for the pixel above, 2 for the pixel to the left (any other distance would be distance + 120).  No colour cache.
 *   CODES       one group of five prefix codes for the picture and one for the sub-image, no meta prefix image: green with the 24 length
 *               prefixes (280 symbols), red, blue, alpha (256), distance (40); frequencies over all tokens of the image.  Lengths by the
 *               rule of ffhip_deflate_code_lengths, limit 15.  An alphabet with no used symbol is written as the simple code of symbol 0, one
 *               with one or two used symbols, all below 256, as the simple code of those (the lower first; a first symbol above 1 takes 8
 *               bits).  Any other is a normal code: its lengths, all of them (no max_symbol), under the 19-symbol code (the same rule, limit 7,
 *               as few of its lengths as the format's order allows, at least 4), run by run of equal values: zeros as 18 for 138 .. 11, then
 *               17 for 10 .. 3, then singly; a value v once unless it is the last non-zero value written (8 at the start), then 16 for
 *               6 .. 3 of the rest, then singly.  Codes are canonical.  A code with ONE used symbol has the empty word.
 *   BOUND       4096 bytes for the head and the tables of both groups, 2 a tile, 60 bits a pixel, 2 bytes.  Bit positions are held in 64 bits.
 * Every choice is a function of the input bytes alone. */
#define FFHIP_VP8L_ENC_SUBTRACT_GREEN 0x1
#define FFHIP_VP8L_ENC_PREDICT 0x2
#define FFHIP_VP8L_ENC_TILE_BITS 4
#define FFHIP_VP8L_ENC_CHUNK 4096
#define FFHIP_EVP8L_NOSPACE (-1301) /* the file does not fit cap: len is the size it needs, nothing at or beyond cap was written */
/* The source is the PNG encoder's record. */
typedef ffhip_png_source ffhip_vp8l_source;
/* Host entries; they need no device.
 *   ffhip_vp8l_encode_bound     a CERTAIN bound on the file (BOUND above), 0 for bad arguments
 *   ffhip_vp8l_encode_residual  the TRANSFORMS alone: residual[height][width] ARGB words as the file codes them, and with
 *                               FFHIP_VP8L_ENC_PREDICT modes[tile rows][tile columns], a byte a tile (modes may be NULL without the flag)
 *   ffhip_vp8l_encode_picture   HOST pixels to the file; *len its size; FFHIP_EVP8L_NOSPACE when that exceeds cap (no byte at or beyond
 *                               out + cap is written) */
size_t ffhip_vp8l_encode_bound(int width, int height);
int ffhip_vp8l_encode_residual(const ffhip_vp8l_source *src, int flags, uint32_t *residual, uint8_t *modes);
int ffhip_vp8l_encode_picture(const ffhip_vp8l_source *src, int flags, uint8_t *out, size_t cap, size_t *len);
/* ffhip_vp8l_encode_items: pictures of any sizes, channel counts, source forms and flags in one batch, byte for byte
 *   ffhip_vp8l_encode_picture's files.  The arrays are HOST arrays, read before the call returns; every check is made before anything is
 *   enqueued (FFHIP_EINVAL, on a machine without a device too; FFHIP_ENODEV there for good arguments); n == 0 is FFHIP_OK.  len_out[i],
 *   status[i] (FFHIP_OK or FFHIP_EVP8L_NOSPACE: len_out[i] is the size needed, no byte at or beyond cap is written); a picture's verdict leaves
 *   its neighbours alone; returns the first code that is not FFHIP_OK.  The batch is cut into parts by a budget over the pixels (64 Mi pixels
 *   -- a pixel takes sixteen bytes of scratch -- and at most 4096 pictures; a picture beyond the budget is a part of its own); the call
 *   SYNCHRONISES the stream once a part.  Kernels: k_vp8l_enc_predict (a wave per tile: the 14 sums by a wave reduction, the residual words
 *   16 bytes a store where the row allows), k_vp8l_enc_parse (a wave per chunk: candidates, the uniform greedy walk, the histogram in LDS,
 *   then integer atomics into the picture's counters), k_vp8l_enc_codes (a wave per picture: lengths, codes, the file's head), k_vp8l_enc_count
 *   and k_vp8l_enc_write (a wave per chunk: its tokens' bits counted, then written by atomicOr into zeroed words), k_vp8l_enc_scan (a workgroup
 *   per picture: the chunks' bit positions, the sizes, the verdict) and a copy kernel with every store under cap.  No kernel waits for
 *   another workgroup. */
typedef struct ffhip_vp8l_encode_item {
    ffhip_vp8l_source src; /* pixels: device */
    int32_t flags, reserved;
    uint8_t *d_out;
    size_t cap;
} ffhip_vp8l_encode_item;
int ffhip_vp8l_encode_items(const ffhip_vp8l_encode_item *items, int n, size_t *len_out, int *status, void *stream);

/* ---- Lossy WebP encoding (ffhip_vp8_enc.c, ffhip_vp8_enc_body.h, ffhip_vp8_enc_gpu.hip) ----
 * Pictures to complete lossy WebP files (RIFF / WEBP / "VP8 ": one VP8 key frame, RFC 6386): colour, prediction, transforms, quantiser,
 * tokens and the bool coder as kernels, the same body as host functions.  There is no byte-for-byte target outside the library -- libwebp's
 * choices are rate-distortion searches -- so THE RULE is its own, a function of the input bytes alone, and host and device share it so that
 * their files are equal byte for byte.  What the rule promises of the file: every decoder of RFC 6386 gives exactly the reconstruction below.
 *   PICTURES    uint8 samples by byte strides in the JPEG encoder's source record, 1 or 3 channels (grey is R = G = B); four channels (alpha)
 *               are FFHIP_EINVAL.  Sides 1..16383.  The file: "RIFF", its size, "WEBP", "VP8 ", the chunk's size, the frame: the 10-byte
 *               key-frame head (scale 0), the first partition, the partition sizes, the token partitions; a zero byte behind an odd chunk.
 *               No VP8X chunk.
 *   COLOUR      libwebp's fixed-point matrix.  Y = (16839 R + 33059 G + 6420 B + (16 << 16) + (1 << 15)) >> 16 per pixel.  For chroma r, g, b
 *               are the PLAIN sums over a 2 x 2 cell -- this is not libwebp's gamma-aware averaging -- with the last column and row
 *               repeated beyond the right and bottom edge: U = (-9719 r - 19081 g + 28800 b + (128 << 18) + (1 << 17)) >> 18,
 *               V = (28800 r - 24116 g - 4684 b + (128 << 18) + (1 << 17)) >> 18, both clamped to 0..255.  The planes are padded to whole
 *               macroblocks by repeating their last column and row.
 *   QUANTISER   quality 0..100 gives y_ac_qi by a table of 101 entries (ffhip_vp8_encode_quality_index: libwebp's 127 (1 - cbrt(l))
 *               evaluated once); the five deltas are 0, there are no segments.  The six steps are RFC 6386's for that index as a decoder
 *               derives them: Y2 DC twice the DC step, Y2 AC 155 / 100 of the AC step and 8 at least, chroma DC 132 at most (what
 *               ffhip_vp8_dequant_factors gives up to index 69; above it that function has the reference's cap on Y2 DC, which no other
 *               decoder has).  level = sign(c) min(2047, (|c| + bias) / step), the exact quotient; bias = step >> 1 for every DC and the
 *               whole Y2 block, (3 step) >> 3 for AC.
 *   TRANSFORMS  over source less prediction, libwebp's forward pair.  The 4 x 4 DCT, rows first, with a0 = d0 + d3, a1 = d1 + d2,
 *               a2 = d1 - d2, a3 = d0 - d3: (a0 + a1) 8, (a2 2217 + a3 5352 + 1812) >> 9, (a0 - a1) 8, (a3 2217 - a2 5352 + 937) >> 9; then
 *               columns, the same butterflies over t[i], t[4 + i], t[8 + i], t[12 + i]: (a0 + a1 + 7) >> 4,
 *               ((a2 2217 + a3 5352 + 12000) >> 16) + (a3 != 0), (a0 - a1 + 7) >> 4, (a3 2217 - a2 5352 + 51000) >> 16.  The Y2 WHT over the
 *               sixteen luma DCs before they are quantised: rows a0 = x0 + x2, a1 = x1 + x3, a2 = x1 - x3, a3 = x0 - x2 giving a0 + a1,
 *               a3 + a2, a3 - a2, a0 - a1; columns a0 = t[i] + t[8 + i], a1 = t[4 + i] + t[12 + i], a2 = t[4 + i] - t[12 + i],
 *               a3 = t[i] - t[8 + i] giving (a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1 at i, 4 + i, 8 + i, 12 + i.
 *   MODES       every macroblock is 16 x 16 with a Y2 block, never B_PRED.  The luma mode is the one of DC, TM, V, H (numbered 0, 1, 2, 3)
 *               with the smallest sum of squared differences between source and prediction, the lowest number at equal sums; the chroma
 *               mode the same over U and V together.  Predictions are RFC 6386's, with its rows of 127 and columns of 129 at the frame's
 *               edges, and are built from the encoder's RECONSTRUCTION, never from the source.
 *   RECONSTRUCTION  RFC 6386's dequantisation (16-bit products), inverse WHT and inverse DCT with clamping: the picture the next macroblock
 *               predicts from, and what a decoder shows when filter is 0.
 *   HEADER      colour space 0, clamp 0, no segmentation, the normal loop filter with sharpness 0 and no deltas; its level is `filter`
 *               0..63, or for -1 min(63, (5 y_ac_qi) >> 4).  Token partitions: the largest power of two <= min(8, macroblock rows).  No
 *               coefficient probability update.  mb_no_skip_coeff = 1 with prob_skip_false = clamp((256 coded + total / 2) / total, 1, 255);
 *               a macroblock whose 25 blocks are all zero is skipped.
 *   TOKENS      RFC 6386 section 13 under the default probabilities; contexts from the neighbours' non-zero flags; an end-of-block behind a
 *               block's last non-zero level; row y goes to partition y & (partitions - 1).  The bool coder and its flush (four bytes) are
 *               section 7.3's.
 *   LIMITS      a first partition over 2^19 - 1 bytes or a token partition over 2^24 - 1 bytes is FFHIP_EVP8_PARTITION for that picture
 *               (its length is 0, nothing is written).
 *   BOUND       a coded bit moves the coder by 7 bits at most, whatever its probability (the range stays within 128..255 and a split is 1
 *               at least), so no look at the default tables can ask more; a flush adds 4 bytes.  The frame header is 1094 coded bits, a
 *               macroblock's header 7.  A coefficient is 19 coded bits at most: not end-of-block, six tree nodes down to cat6, cat6's eleven
 *               extra bits (they hold a level up to 2047, the clamp), the sign.  A block is 16 x 19 + 1, a luma block behind Y2 15 x 19 + 1:
 *               7321 a macroblock.  bound = 30 + ceil(7 (1094 + 7 n) / 8) + 4 + 3 (partitions - 1) + sum over partitions
 *               (ceil(7 x 7321 n_p / 8) + 4) + 1, some 25 bytes a pixel.
 * Every choice is a function of the input bytes alone. */
#define FFHIP_EVP8_NOSPACE (-1401)   /* the file does not fit cap: len is the size it needs, nothing at or beyond cap was written */
#define FFHIP_EVP8_PARTITION (-1402) /* a partition is longer than the frame can say (LIMITS) */
/* Host entries; they need no device.  cols = ceil(width / 16), rows = ceil(height / 16), n = cols x rows.
 *   ffhip_vp8_encode_quality_index  y_ac_qi of a quality, FFHIP_EINVAL beyond 0..100
 *   ffhip_vp8_encode_bound          a CERTAIN bound on the file (BOUND above), 0 for bad arguments
 *   ffhip_vp8_encode_planes         COLOUR alone: y[16 rows][16 cols], u and v [8 rows][8 cols], padding included
 *   ffhip_vp8_encode_mbs            MODES, levels and RECONSTRUCTION: ymode[n], uvmode[n], levels[n][25][16] (raster positions inside a block;
 *                                   16 Y, 4 U, 4 V, Y2: the decoders' layout), recon_y / _u / _v as the planes above, unfiltered
 *   ffhip_vp8_encode_picture        HOST pixels to the file; *len its size; FFHIP_EVP8_NOSPACE when that exceeds cap (no byte at or beyond
 *                                   out + cap is written; below it lie the file's first cap bytes) */
int ffhip_vp8_encode_quality_index(int quality);
size_t ffhip_vp8_encode_bound(int width, int height);
int ffhip_vp8_encode_planes(const ffhip_jpeg_source *src, uint8_t *y, uint8_t *u, uint8_t *v);
int ffhip_vp8_encode_mbs(const ffhip_jpeg_source *src, int quality, uint8_t *ymode, uint8_t *uvmode, int16_t *levels, uint8_t *recon_y, uint8_t *recon_u,
                         uint8_t *recon_v);
int ffhip_vp8_encode_picture(const ffhip_jpeg_source *src, int quality, int filter, uint8_t *out, size_t cap, size_t *len);
/* ffhip_vp8_encode_items: pictures of any sizes, channel counts, source forms, qualities and filter levels in one batch, byte for byte
 *   ffhip_vp8_encode_picture's files.  The arrays are HOST arrays, read before the call returns; every check is made before anything is
 *   enqueued (FFHIP_EINVAL, on a machine without a device too; FFHIP_ENODEV there for good arguments); n == 0 is FFHIP_OK.  len_out[i],
 *   status[i] (FFHIP_OK; FFHIP_EVP8_NOSPACE: len_out[i] is the size needed, no byte at or beyond cap is written; FFHIP_EVP8_PARTITION); a
 *   picture's verdict leaves its neighbours alone; returns the first code that is not FFHIP_OK.  The batch is cut into parts by a budget over
 *   the pixels of the macroblock grids (32 Mi pixels -- a pixel takes 32 bytes of scratch: 3 of planes, 3.2 of levels, modes and masks, 25.1 of
 *   the partitions' bound -- and at most 4096 pictures; a picture beyond the budget is a part of its own); the call SYNCHRONISES the stream
 *   once a part.  Kernels: k_vp8_enc_color (a thread per 2 x 2 cell: the padded planes), k_vp8_enc_mb (a wave per macroblock, ONE LAUNCH PER
 *   ANTI-DIAGONAL of the part's largest grid, cols + rows - 1 of them: a macroblock reads the reconstruction of its left, upper and upper-left
 *   neighbours only; the eight sums by a wave reduction, a block a lane for the transforms), k_vp8_enc_parts (a lane per partition of a
 *   picture, the first partition included: it tokenises as it codes), k_vp8_enc_scan (a thread per picture: sizes, head, verdict) and
 *   k_vp8_enc_copy with every store under cap.  No kernel waits for another workgroup. */
typedef struct ffhip_vp8_encode_item {
    ffhip_jpeg_source src; /* pixels: device */
    int32_t quality, filter;
    uint8_t *d_out;
    size_t cap;
} ffhip_vp8_encode_item;
int ffhip_vp8_encode_items(const ffhip_vp8_encode_item *items, int n, size_t *len_out, int *status, void *stream);

/* ---- batches over the GPUs of one node, from C (ffhip_shard.hip) ----
 * The reference decodes one image at a time on one thread (format/jpg.c:458-585) and has no collective of any kind
 * (SURVEY 2.1); images are independent, so a batch shards into contiguous image ranges -- one process and one GPU
 * per rank -- with no data-path exchange.  The only collective is the batch close: ONE ncclAllGather (RCCL over
 * xGMI) of a 32-byte record per rank, which is also the batch barrier.  RCCL is bound at run time (dlopen; a copy
 * already in the process is reused), so one-GPU callers never need it. */
typedef struct ffhip_batch_record {
    int32_t rank;      /* who                                                                   */
    int32_t status;    /* 0, or the FFHIP_E* code of the rank's first failing call              */
    int64_t first;     /* the rank's image range [first, first + count)                         */
    int64_t count;
    uint64_t checksum; /* sum of the rank's per-image checksums (ffhip_bgra_checksum), mod 2^64 */
} ffhip_batch_record;
#define FFHIP_COMM_ID_BYTES 128
/* contiguous image range of `rank` out of `world`; sizes differ by at most one */
int ffhip_shard_range(long long n_images, int rank, int world, long long *first, long long *count);
/* rank 0: a fresh communicator id (ncclGetUniqueId); the host program hands its 128 bytes to the other ranks */
int ffhip_comm_unique_id(void *id128);
/* every rank, on its own device (after ffhip_init): ncclCommInitRank; NULL on failure */
void *ffhip_comm_init_rank(const void *id128, int rank, int world);
void ffhip_comm_destroy(void *comm);
/* Enqueues the all-gather of this rank's record behind what `stream` holds, synchronises `stream` and fills
 * h_records[world] in rank order.  comm == NULL with world == 1: the one-GPU case (stream sync + own record). */
int ffhip_batch_close(void *comm, int rank, int world, long long first, long long count, int status,
                      uint64_t checksum, ffhip_batch_record *h_records, void *stream);
/* host only: 1 when the records tile [0, n_images) exactly, record r is rank r's and every status is 0 */
int ffhip_batch_complete(const ffhip_batch_record *records, int world, long long n_images);
/* per image the sum over its 32-bit pixels p[i] (row-major over width x height) of p[i] * ((i & 0xffff) + 1), mod
 * 2^64, into d_sums[n_images] (device): lets a rank vouch for gigabytes of output with 8 bytes per image */
int ffhip_bgra_checksum(const uint8_t *d_bgra, int64_t pitch, int64_t image_stride, int width, int height,
                        int n_images, uint64_t *d_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FFPIC_HIP_H */
