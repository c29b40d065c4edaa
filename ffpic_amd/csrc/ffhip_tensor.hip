/*
 * ffhip_tensor.hip -- the last stage between the decoders and a program that reads tensors: BGRA pictures as the decode calls leave
 * them -> RGB / BGR, CHW / HWC, uint8 / float16 / float32, cropped to a rectangle, in one launch for a whole mixed batch
 * (ffhip_bgra_to_tensor_items), and the file calls built on it (ffhip_jpeg_decode_files_tensor, ffhip_webp_decode_files_tensor, and
 * their _resized forms with ffhip_bgra_resize_items between the decoder and this stage, their _oriented forms with
 * ffhip_bgra_orient_items in front of this stage).
 * The layout of the work is described in ffhip_tensor_body.h.
 */
#include "ffhip_items.h"
#include "ffhip_jpeg_scaled_body.h"
#include "ffhip_orient_body.h"
#include "ffhip_tensor_body.h"
#include "ffhip_jpeg_prog_internal.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace {

struct TensorArgs {
    const TensorItemDesc *desc;
    const u32 *wg_item; /* per workgroup of the call: its item */
    u32 wg_base;        /* the launch's first workgroup */
    TensorScale s;
};

/* A workgroup takes FFHIP_TENSOR_WG_UNITS consecutive units of one item, lane l the units l, l + 256, ...: a wave's 64 lanes store 64
 * consecutive 16-byte blocks of a run (or of the runs that follow each other in a narrow picture). */
template <int DT, bool PLANAR, bool BGR> __global__ __launch_bounds__(FFHIP_TENSOR_WG_THREADS) void k_bgra_to_tensor(TensorArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const TensorItemDesc d = a.desc[item];
    const u32 base = (wg - d.first_wg) * FFHIP_TENSOR_WG_UNITS + threadIdx.x;
#pragma unroll 2
    for (int i = 0; i < FFHIP_TENSOR_UNITS_PER_LANE; i++) {
        const u32 t = base + (u32)i * FFHIP_TENSOR_WG_THREADS;
        if (t >= d.total) break;
        tensor_unit<DT, PLANAR, BGR>(d, a.s, t);
    }
}

typedef void (*TensorKernel)(TensorArgs);
template <int DT> TensorKernel tensor_kernel_of(bool planar, bool bgr)
{
    return planar ? (bgr ? k_bgra_to_tensor<DT, true, true> : k_bgra_to_tensor<DT, true, false>)
                  : (bgr ? k_bgra_to_tensor<DT, false, true> : k_bgra_to_tensor<DT, false, false>);
}
TensorKernel tensor_kernel(const ffhip_tensor_format *f)
{
    const bool planar = f->planar != 0, bgr = f->bgr != 0;
    return f->dtype == FFHIP_TENSOR_U8 ? tensor_kernel_of<FFHIP_TENSOR_U8>(planar, bgr)
         : f->dtype == FFHIP_TENSOR_F16 ? tensor_kernel_of<FFHIP_TENSOR_F16>(planar, bgr)
                                        : tensor_kernel_of<FFHIP_TENSOR_F32>(planar, bgr);
}

int tensor_elem_size(int dtype) { return dtype == FFHIP_TENSOR_U8 ? 1 : (dtype == FFHIP_TENSOR_F16 ? 2 : 4); }

bool tensor_format_ok(const ffhip_tensor_format *f)
{
    if (!f || f->dtype < FFHIP_TENSOR_U8 || f->dtype > FFHIP_TENSOR_F32) return false;
    for (int c = 0; c < 3; c++) {
        if (!isfinite(f->scale[c]) || !isfinite(f->bias[c])) return false;
        if (f->dtype == FFHIP_TENSOR_U8 && (f->scale[c] != 1.0f || f->bias[c] != 0.0f)) return false;
    }
    return true;
}

/* an item the call takes under format f; fills its record (first_wg aside) */
bool tensor_item_desc(const ffhip_tensor_item &it, const ffhip_tensor_format *f, TensorItemDesc *out)
{
    const int es = tensor_elem_size(f->dtype);
    if (it.width < 1 || it.height < 1 || it.x0 < 0 || it.y0 < 0) return false;
    if (!it.d_bgra || ((uintptr_t)it.d_bgra & 3) || it.pitch < 4 || (it.pitch & 3)) return false;
    /* source offsets stay within 31 bits, as the decode calls' own pictures do (pitch x rows < 2^31), and the rectangle within the pitch */
    if (4LL * ((long long)it.x0 + it.width) > it.pitch || ((long long)it.y0 + it.height) * it.pitch > 0x7fffffffLL) return false;
    if (!it.d_out || ((uintptr_t)it.d_out & (uintptr_t)(es - 1))) return false;
    const long long run_len = f->planar ? it.width : 3LL * it.width;
    if (it.row_stride < run_len) return false;
    __int128 span = (__int128)it.row_stride * (it.height - 1) + run_len; /* elements from the first to behind the last of a plane (HWC: of the tensor) */
    if (f->planar) {
        if ((__int128)it.plane_stride < span) return false;
        span += (__int128)it.plane_stride * 2;
    }
    if (span * es > ((__int128)1 << 62)) return false; /* element offsets are 64-bit in the kernel */
    const long long runs = (f->planar ? 3LL : 1LL) * it.height;
    const long long units = (run_len * es + 15) / 16 + 1;
    if (runs * units > 0xffffffffLL) return false; /* a unit's index is 32-bit */
    memset(out, 0, sizeof(*out));
    out->src = it.d_bgra + (long long)it.y0 * it.pitch + 4LL * it.x0;
    out->dst = (uint8_t *)it.d_out;
    out->pitch = it.pitch;
    out->row_stride = it.row_stride;
    out->plane_stride = f->planar ? it.plane_stride : 0;
    out->width = it.width;
    out->height = it.height;
    out->units = (u32)units;
    out->total = (u32)(runs * units);
    out->n_wgs = (u32)((runs * units + FFHIP_TENSOR_WG_UNITS - 1) / FFHIP_TENSOR_WG_UNITS);
    return true;
}

} // namespace

extern "C" int ffhip_bgra_to_tensor_items(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, void *stream)
{
    if (n < 0 || (n > 0 && !items) || !tensor_format_ok(fmt)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    /* the records, every item's workgroups behind those of the items before it */
    std::vector<TensorItemDesc> desc((size_t)n);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (!tensor_item_desc(items[i], fmt, &desc[(size_t)i])) return FFHIP_EINVAL;
        desc[(size_t)i].first_wg = (u32)total;
        total += desc[(size_t)i].n_wgs;
    }
    if (total > 0xffffffffULL) return FFHIP_EINVAL; /* the table's entries are 32-bit workgroup indices */
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    hipStream_t st = (hipStream_t)stream;
    /* device scratch: the records, then the per-workgroup table; pinned staging for the records.  Both per stream */
    const TensorItemDesc *d_desc = nullptr;
    u32 *d_table = nullptr;
    const int rc = ffhip_items_upload(SCRATCH_TENSOR_ITEMS, stream, desc, total, &d_desc, &d_table);
    if (rc) return rc;
    const TensorKernel kernel = tensor_kernel(fmt);
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        TensorArgs a;
        a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
        for (int c = 0; c < 3; c++) { a.s.scale[c] = fmt->scale[c]; a.s.bias[c] = fmt->bias[c]; }
        hipLaunchKernelGGL(kernel, dim3(grid_x), dim3(FFHIP_TENSOR_WG_THREADS), 0, st, a);
    });
}

/* ---- files in, tensors out ---- */
namespace {

struct TensorPicture { int coded_w, coded_h, width, height; int64_t pitch; }; /* what a decode call writes; what the file displays (inside it); its row bytes */
thread_local int g_tensor_last_parts = 0; /* ffhip_debug_tensor_last_parts */
thread_local int g_orient_last_items = 0; /* ffhip_debug_orient_last_items */
/* decodes files [first, first + cnt) into d_bgra[k] with pitch[k]: the call underneath, its per-file codes into status + first */
typedef std::function<int(int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch)> TensorDecode;

size_t tensor_part_budget()
{
    const char *v = FFHIP_ENV("FFHIP_TENSOR_PART_BYTES");
    const long long b = v ? atoll(v) : 0;
    return b > 0 ? (size_t)b : (size_t)1 << 30;
}

struct TensorResize { const ffhip_size *out_size; int filter; }; /* out_size == NULL: every file keeps its rectangle's size */

/* pic[i] is valid where status[i] == 0 (the probe's verdict).  orient == NULL: the calls without orientation.  Otherwise orient[i] in 1..8
 * where status[i] == 0, and roi and rs.out_size are the STORED ones (mapped and swapped by the caller): decode and resize run as without,
 * and a file of another orientation than 1 goes through ffhip_bgra_orient_items -- its resized picture, or its rectangle -- into part
 * scratch at pitch 4 x upright width, which the sink then reads whole; outs[i] is laid out for the upright size */
int tensor_files_run(int n, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs, const ffhip_rect *roi, const TensorResize &rs,
                     const std::vector<TensorPicture> &pic, const int *orient, int *status, void *stream, const TensorDecode &decode)
{
    const ffhip_size *out_size = rs.out_size;
    g_tensor_last_parts = 0; /* a call that returns before its first part has taken none */
    g_orient_last_items = 0;
    auto turned = [&](int i) { return orient && !status[i] && orient[i] != 1; };
    /* the items, with a stand-in for the picture's address: everything about rectangle and output is checked before anything is enqueued */
    std::vector<ffhip_tensor_item> item((size_t)n);
    std::vector<int> mine((size_t)n, FFHIP_OK); /* the code this call gives a file the decoder takes */
    for (int i = 0; i < n; i++) {
        if (status[i]) continue;
        const TensorPicture &p = pic[(size_t)i];
        const ffhip_rect r = roi ? roi[i] : ffhip_rect{0, 0, p.width, p.height};
        ffhip_tensor_item &it = item[(size_t)i];
        it.d_bgra = (const uint8_t *)(uintptr_t)256; it.pitch = p.pitch;
        it.x0 = r.x0; it.y0 = r.y0; it.width = r.width; it.height = r.height;
        it.d_out = outs[i].d_out; it.row_stride = outs[i].row_stride; it.plane_stride = outs[i].plane_stride;
        TensorItemDesc d;
        bool ok = r.x0 >= 0 && r.y0 >= 0 && r.width >= 1 && r.height >= 1 && (long long)r.x0 + r.width <= p.width && (long long)r.y0 + r.height <= p.height;
        if (ok && out_size) { /* the rectangle is the resize's source; the sink takes the whole resized picture */
            const ffhip_size &o = out_size[i];
            ok = r.width <= FFHIP_RESIZE_MAX_SIDE && r.height <= FFHIP_RESIZE_MAX_SIDE && o.width >= 1 && o.width <= FFHIP_RESIZE_MAX_SIDE &&
                 o.height >= 1 && o.height <= FFHIP_RESIZE_MAX_SIDE;
            it.pitch = 4LL * o.width; it.x0 = 0; it.y0 = 0; it.width = o.width; it.height = o.height;
        }
        if (ok && turned(i)) { /* the sink takes the whole upright picture; what it checked of the source, the stage checks of its own */
            const bool swap = FFHIP_ORIENT_TRANSPOSE(orient[i]);
            ok = ((long long)it.y0 + it.height) * it.pitch <= 0x7fffffffLL;
            const int uw = swap ? it.height : it.width, uh = swap ? it.width : it.height;
            it.pitch = 4LL * uw; it.x0 = 0; it.y0 = 0; it.width = uw; it.height = uh;
        }
        if (!ok || !tensor_item_desc(it, fmt, &d)) mine[(size_t)i] = FFHIP_EINVAL;
    }
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = tensor_part_budget();
    auto bytes_of = [&](int i) { return status[i] ? (size_t)0 : ((size_t)pic[(size_t)i].pitch * pic[(size_t)i].coded_h + 255) & ~(size_t)255; };
    /* the resized picture of a file that gets one */
    auto resized_of = [&](int i) { return !out_size || status[i] || mine[(size_t)i] ? (size_t)0 : ((size_t)4 * out_size[i].width * out_size[i].height + 255) & ~(size_t)255; };
    /* the upright picture of a file that gets one */
    auto upright_of = [&](int i) { return !turned(i) || mine[(size_t)i] ? (size_t)0 : ((size_t)4 * item[(size_t)i].width * item[(size_t)i].height + 255) & ~(size_t)255; };
    for (int first = 0; first < n;) {
        /* a part: files while their pictures fit the budget; a picture larger than the budget is a part of its own */
        int cnt = 0;
        size_t bytes = 0, resized = 0, upright = 0;
        while (first + cnt < n && (cnt == 0 || bytes + resized + upright + bytes_of(first + cnt) + resized_of(first + cnt) + upright_of(first + cnt) <= budget)) {
            resized += resized_of(first + cnt);
            upright += upright_of(first + cnt);
            bytes += bytes_of(first + cnt++);
        }
        uint8_t *base = (uint8_t *)ffhip_scratch(SCRATCH_TENSOR_BGRA, stream, bytes / 4 + 64);
        if (!base) return FFHIP_ENOMEM;
        std::vector<uint8_t *> d_bgra((size_t)cnt);
        std::vector<int64_t> pitch((size_t)cnt);
        size_t at = 0;
        for (int k = 0; k < cnt; k++) { /* (a file the probe refused: the decoder refuses it again before it looks at its output) */
            d_bgra[(size_t)k] = base + at;
            pitch[(size_t)k] = status[first + k] ? 0 : pic[(size_t)(first + k)].pitch;
            at += bytes_of(first + k);
        }
        g_tensor_last_parts++;
        const int rc = decode(first, cnt, d_bgra.data(), pitch.data());
        if (rc) { /* a file's code, or the call's own failure */
            bool a_files = false;
            for (int k = 0; k < cnt; k++) a_files = a_files || status[first + k] == rc;
            if (!a_files) return rc;
        }
        uint8_t *small = nullptr; /* the part's resized pictures, pitch 4 x out width */
        if (out_size && !(small = (uint8_t *)ffhip_scratch(SCRATCH_RESIZE_BGRA, stream, resized / 4 + 64))) return FFHIP_ENOMEM;
        uint8_t *turn_to = nullptr; /* the part's upright pictures, pitch 4 x upright width */
        if (upright && !(turn_to = (uint8_t *)ffhip_scratch(SCRATCH_ORIENT_BGRA, stream, upright / 4 + 64))) return FFHIP_ENOMEM;
        std::vector<ffhip_tensor_item> good;
        std::vector<ffhip_resize_item> shrink;
        std::vector<ffhip_orient_item> turn;
        size_t small_at = 0, turn_at = 0;
        for (int k = 0; k < cnt; k++) {
            const int i = first + k;
            if (status[i]) continue;
            if (mine[(size_t)i]) { status[i] = mine[(size_t)i]; continue; }
            item[(size_t)i].d_bgra = d_bgra[(size_t)k];
            const ffhip_rect r = roi ? roi[i] : ffhip_rect{0, 0, pic[(size_t)i].width, pic[(size_t)i].height};
            ffhip_orient_item t; /* what the stage turns where there is no resize: the rectangle of the decoded picture */
            t.d_src = d_bgra[(size_t)k]; t.src_pitch = pitch[(size_t)k];
            t.x0 = r.x0; t.y0 = r.y0; t.width = r.width; t.height = r.height;
            if (out_size) {
                ffhip_resize_item s;
                s.d_src = d_bgra[(size_t)k]; s.src_pitch = pitch[(size_t)k];
                s.x0 = r.x0; s.y0 = r.y0; s.width = r.width; s.height = r.height;
                s.d_dst = small + small_at; s.dst_pitch = 4LL * out_size[i].width;
                s.out_width = out_size[i].width; s.out_height = out_size[i].height;
                shrink.push_back(s);
                item[(size_t)i].d_bgra = s.d_dst;
                small_at += resized_of(i);
                t.d_src = s.d_dst; t.src_pitch = s.dst_pitch;
                t.x0 = 0; t.y0 = 0; t.width = s.out_width; t.height = s.out_height;
            }
            if (turned(i)) {
                t.d_dst = turn_to + turn_at; t.dst_pitch = item[(size_t)i].pitch;
                t.orientation = orient[i];
                turn.push_back(t);
                item[(size_t)i].d_bgra = t.d_dst;
                turn_at += upright_of(i);
            }
            good.push_back(item[(size_t)i]);
        }
        if (out_size) {
            const int rrc = ffhip_bgra_resize_items(shrink.data(), (int)shrink.size(), rs.filter, stream);
            if (rrc) return rrc;
        }
        if (!turn.empty()) {
            const int trc = ffhip_bgra_orient_items(turn.data(), (int)turn.size(), stream);
            if (trc) return trc;
            g_orient_last_items += (int)turn.size();
        }
        const int src = ffhip_bgra_to_tensor_items(good.data(), (int)good.size(), fmt, stream);
        if (src) return src;
        FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO); /* the next part decodes into the same scratch */
        first += cnt;
    }
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}

bool tensor_files_args_ok(const uint8_t *const *files, const size_t *lens, int n, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs, const int *status)
{
    return n >= 0 && tensor_format_ok(fmt) && (n == 0 || (files && lens && outs && status));
}

bool resize_files_args_ok(int n, const ffhip_size *out_size, int filter)
{
    return (filter == FFHIP_RESIZE_BILINEAR || filter == FFHIP_RESIZE_ANTIALIAS) && (n <= 0 || out_size);
}

/* on: the _oriented calls.  orient[i] 1..8 or 0 ("the file's tag"); orient == NULL: every file's tag */
struct TensorOrient { bool on; const int *orient; int *orient_out; };

bool orient_files_args_ok(int n, const TensorOrient &to)
{
    for (int i = 0; to.on && to.orient && i < n; i++)
        if (to.orient[i] < 0 || to.orient[i] > 8) return false;
    return true;
}

/* What the run sees of the caller's upright rectangles and sizes.  Off: the caller's own arrays, nothing else.  On: per file the
 * orientation used, the rectangle mapped by ffhip_orient_rect (an empty one where it leaves the upright picture: the run refuses the
 * file) and the size swapped for 5..8 */
class TensorStored {
public:
    TensorStored(int n, bool on, const ffhip_rect *roi, const ffhip_size *out_size)
        : on_(on), caller_roi_(roi), caller_size_(out_size), o_(on ? (size_t)n : 0, 1), roi_(on && roi ? (size_t)n : 0, ffhip_rect{0, 0, 0, 0}),
          size_(on && out_size ? (size_t)n : 0, ffhip_size{0, 0}) {}
    /* file i: orientation o (0: the probe refused the file), its stored display size w x h */
    void set(int i, int o, int w, int h, int *orient_out)
    {
        if (orient_out) orient_out[i] = o;
        o_[(size_t)i] = o ? o : 1;
        if (!o) return;
        if (caller_roi_ && ffhip_orient_rect(w, h, o, &caller_roi_[i], &roi_[(size_t)i]) != FFHIP_OK) roi_[(size_t)i] = ffhip_rect{0, 0, 0, 0};
        if (caller_size_) {
            const ffhip_size s = caller_size_[i];
            size_[(size_t)i] = FFHIP_ORIENT_TRANSPOSE(o) ? ffhip_size{s.height, s.width} : s;
        }
    }
    const ffhip_rect *roi() const { return on_ && caller_roi_ ? roi_.data() : caller_roi_; }
    const ffhip_size *out_size() const { return on_ && caller_size_ ? size_.data() : caller_size_; }
    const int *orient() const { return on_ ? o_.data() : nullptr; }

private:
    bool on_;
    const ffhip_rect *caller_roi_;
    const ffhip_size *caller_size_;
    std::vector<int> o_;
    std::vector<ffhip_rect> roi_;
    std::vector<ffhip_size> size_;
};

/* the two families' common bodies: rs.out_size == NULL is the call without a resize */
/* denom == NULL: every file at full size, the calls as they were.  Otherwise file i is decoded at 1 / denom[i] of its size (0: the largest
 * denominator at which its rectangle still covers out_size[i], ffhip_jpeg_scale_choose): the picture the run below sees is the SCALED one
 * -- coded and display size, a pitch rounded up to 16 bytes -- and the rectangle is the full-size one mapped onto it */
int jpeg_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs,
                      const ffhip_rect *roi, const TensorResize &rs, const int *denom, int *denom_out, const TensorOrient &to,
                      ffhip_jpeg_geom *geom_out, int *status, void *stream, unsigned flags = 0u)
{
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status) || !orient_files_args_ok(n, to) || (flags & ~(FFHIP_JPEG_ACCEPT_PROGRESSIVE | FFHIP_JPEG_PIXELS_LIBJPEG))) return FFHIP_EINVAL;
    for (int i = 0; denom && i < n; i++) {
        if (denom[i] != 0 ? !jpeg_denom_ok(denom[i]) : !rs.out_size) return FFHIP_EINVAL;
        if ((flags & FFHIP_JPEG_PIXELS_LIBJPEG) && denom[i] != 1) return FFHIP_EINVAL; /* libjpeg's pixels: full size only, "choose" included */
    }
    if (n == 0) return FFHIP_OK;
    std::vector<TensorPicture> pic((size_t)n);
    std::vector<int> den(denom ? (size_t)n : 0, 1);
    std::vector<ffhip_rect> mapped(denom && roi ? (size_t)n : 0);
    TensorStored stored(n, to.on, roi, rs.out_size); /* rectangles and sizes in the stored axes, where the call turns pictures */
    ffhip_parallel_for(n, n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads), [&](int i) {
        const JpegProbed probed = jpeg_probe_file(files[i], lens[i], flags);
        const ffhip_jpeg_geom &g = probed.geom;
        const int w = probed.width, h = probed.height;
        status[i] = probed.status;
        if (geom_out) geom_out[i] = g;
        pic[(size_t)i] = TensorPicture{g.mcu_cols * 8 * g.h, g.mcu_rows * 8 * g.v, w, h, 4LL * g.mcu_cols * 8 * g.h};
        if (to.on) {
            int o = to.orient ? to.orient[i] : 0;
            if (!status[i] && o == 0) ffhip_jpeg_exif_orientation(files[i], lens[i], &o);
            stored.set(i, status[i] ? 0 : o, w, h, to.orient_out);
        }
        if (!denom) return;
        if (denom_out) denom_out[i] = 0;
        if (roi) mapped[(size_t)i] = ffhip_rect{0, 0, 0, 0}; /* an empty rectangle: the run refuses the file */
        if (status[i]) return;
        const ffhip_rect r = roi ? stored.roi()[i] : ffhip_rect{0, 0, w, h};
        const bool r_ok = r.x0 >= 0 && r.y0 >= 0 && r.width >= 1 && r.height >= 1 && (long long)r.x0 + r.width <= w && (long long)r.y0 + r.height <= h;
        int d = denom[i];
        if (d == 0) {
            const ffhip_size &o = stored.out_size()[i];
            d = r_ok && o.width >= 1 && o.height >= 1 ? ffhip_jpeg_scale_choose(r.width, r.height, o.width, o.height) : 1;
        }
        den[(size_t)i] = d;
        if (denom_out) denom_out[i] = d;
        const int N = 8 / d;
        const int cw = N * g.h * g.mcu_cols, chh = N * g.v * g.mcu_rows;
        pic[(size_t)i] = TensorPicture{cw, chh, jpeg_scaled_len(w, d), jpeg_scaled_len(h, d), (4LL * cw + 15) & ~15LL};
        if (roi && r_ok) mapped[(size_t)i] = jpeg_scaled_rect_of(w, h, d, r);
    });
    int prog_total[5] = {0, 0, 0, 0, 0}; /* the parts' ffhip_debug_progressive_last, summed (the front end: the last part's) */
    const int rc = tensor_files_run(n, fmt, outs, denom && roi ? mapped.data() : stored.roi(), TensorResize{stored.out_size(), rs.filter}, pic, stored.orient(), status, stream,
                            [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        const int prc = jpeg_decode_files_mixed(files + first, lens + first, cnt, n_threads, d_bgra, pitch, denom ? den.data() + first : nullptr, flags,
                                                geom_out ? geom_out + first : nullptr, status + first, stream);
        if (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) { /* only then has the part written the thread's record */
            int last[5];
            ffhip_debug_progressive_last(last);
            for (int q = 0; q < 4; q++) prog_total[q] += last[q];
            prog_total[4] = last[4];
        }
        return prc;
    });
    if (flags & FFHIP_JPEG_ACCEPT_PROGRESSIVE) ffhip_prog_note_last(prog_total);
    return rc;
}

int webp_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs,
                      const ffhip_rect *roi, const TensorResize &rs, const TensorOrient &to, ffhip_webp_info *info_out, int *status, void *stream)
{
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status) || !orient_files_args_ok(n, to)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    std::vector<TensorPicture> pic((size_t)n);
    TensorStored stored(n, to.on, roi, rs.out_size);
    for (int i = 0; i < n; i++) {
        int w = 0, h = 0, c = 0, r = 0;
        status[i] = files[i] && lens[i] ? ffhip_webp_probe(files[i], lens[i], &w, &h, &c, &r) : FFHIP_EINVAL;
        /* the loader's size is the container's word (ffhip_webp_info): what of it the decoded picture holds */
        pic[(size_t)i] = TensorPicture{16 * c, 16 * r, w < 16 * c ? w : 16 * c, h < 16 * r ? h : 16 * r, 64LL * c};
        if (to.on) {
            int o = to.orient ? to.orient[i] : 0;
            if (!status[i] && o == 0) ffhip_webp_exif_orientation(files[i], lens[i], &o);
            stored.set(i, status[i] ? 0 : o, pic[(size_t)i].width, pic[(size_t)i].height, to.orient_out);
        }
    }
    return tensor_files_run(n, fmt, outs, stored.roi(), TensorResize{stored.out_size(), rs.filter}, pic, stored.orient(), status, stream, [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        return ffhip_webp_decode_files_device(files + first, lens + first, cnt, n_threads, d_bgra, pitch, info_out ? info_out + first : nullptr,
                                              status + first, stream);
    });
}

} // namespace

extern "C" int ffhip_jpeg_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                              const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{nullptr, 0}, nullptr, nullptr, TensorOrient{false, nullptr, nullptr}, geom_out, status, stream);
}

extern "C" int ffhip_webp_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                              const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_webp_info *info_out, int *status, void *stream)
{
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{nullptr, 0}, TensorOrient{false, nullptr, nullptr}, info_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                      ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (!resize_files_args_ok(n, out_size, filter)) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, nullptr, nullptr, TensorOrient{false, nullptr, nullptr}, geom_out, status, stream);
}

extern "C" int ffhip_webp_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                      ffhip_webp_info *info_out, int *status, void *stream)
{
    if (!resize_files_args_ok(n, out_size, filter)) return FFHIP_EINVAL;
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, TensorOrient{false, nullptr, nullptr}, info_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_scaled(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                     const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                     const int *denom, int *denom_out, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS) return FFHIP_EINVAL;
    if (n > 0 && !denom) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, denom, denom_out, TensorOrient{false, nullptr, nullptr}, geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                       const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                       const int *denom, int *denom_out, const int *orient, int *orient_out,
                                                       ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, denom, denom_out, TensorOrient{true, orient, orient_out},
                             geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                 const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                 const int *denom, int *denom_out, const int *orient, int *orient_out, unsigned flags,
                                                 ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, denom, denom_out, TensorOrient{true, orient, orient_out},
                             geom_out, status, stream, flags);
}

extern "C" int ffhip_webp_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                       const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                       const int *orient, int *orient_out, ffhip_webp_info *info_out, int *status, void *stream)
{
    if (filter != FFHIP_RESIZE_BILINEAR && filter != FFHIP_RESIZE_ANTIALIAS) return FFHIP_EINVAL;
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, roi, TensorResize{out_size, filter}, TensorOrient{true, orient, orient_out}, info_out, status, stream);
}

extern "C" int ffhip_debug_tensor_last_parts(void) { return g_tensor_last_parts; }
extern "C" int ffhip_debug_orient_last_items(void) { return g_orient_last_items; }
