/*
 * ffhip_tensor.hip -- the last stage between the decoders and a program that reads tensors: BGRA pictures as the decode calls leave
 * them -> RGB / BGR, CHW / HWC, uint8 / float16 / float32, cropped to a rectangle, in one launch for a whole mixed batch
 * (ffhip_bgra_to_tensor_items), and the file calls built on it (ffhip_jpeg_decode_files_tensor, ffhip_webp_decode_files_tensor, ffhip_png_decode_files_tensor, ffhip_vp8l_decode_files_tensor, their
 * _alpha forms that carry the alpha byte through the chain, and
 * their _resized forms with ffhip_bgra_resize_items between the decoder and this stage, their _oriented forms with
 * ffhip_bgra_orient_items in front of this stage).
 * The layout of the work is described in ffhip_tensor_body.h.
 */
#include "ffhip_staged.h" /* ffhip_part_budget */
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

/* The forms with alpha: the same deal of units, NC channels under policy AP.  A kernel of their own, so that the twelve
 * instances above keep their argument block and their instructions */
struct TensorAlphaArgs {
    const TensorItemDesc *desc;
    const u32 *wg_item;
    u32 wg_base;
    TensorScale s;
    TensorAlpha al;
};
template <int DT, bool PLANAR, bool BGR, int NC, int AP> __global__ __launch_bounds__(FFHIP_TENSOR_WG_THREADS) void k_bgra_to_tensor_alpha(TensorAlphaArgs a)
{
    const u32 wg = a.wg_base + blockIdx.x;
    const u32 item = __builtin_amdgcn_readfirstlane(a.wg_item[wg]);
    const TensorItemDesc d = a.desc[item];
    const u32 base = (wg - d.first_wg) * FFHIP_TENSOR_WG_UNITS + threadIdx.x;
#pragma unroll 2
    for (int i = 0; i < FFHIP_TENSOR_UNITS_PER_LANE; i++) {
        const u32 t = base + (u32)i * FFHIP_TENSOR_WG_THREADS;
        if (t >= d.total) break;
        tensor_unit<DT, PLANAR, BGR, NC, AP>(d, a.s, t, a.al);
    }
}

typedef void (*TensorAlphaKernel)(TensorAlphaArgs);
template <int DT, bool PLANAR, bool BGR> TensorAlphaKernel tensor_alpha_kernel_as(int policy)
{
    switch (policy) {
    case TENSOR_ALPHA_KEEP: return k_bgra_to_tensor_alpha<DT, PLANAR, BGR, 4, TENSOR_ALPHA_KEEP>;
    case TENSOR_ALPHA_PREMUL: return k_bgra_to_tensor_alpha<DT, PLANAR, BGR, 4, TENSOR_ALPHA_PREMUL>;
    case TENSOR_ALPHA_UNPREMUL: return k_bgra_to_tensor_alpha<DT, PLANAR, BGR, 4, TENSOR_ALPHA_UNPREMUL>;
    case TENSOR_ALPHA_OVER_S: return k_bgra_to_tensor_alpha<DT, PLANAR, BGR, 3, TENSOR_ALPHA_OVER_S>;
    default: return k_bgra_to_tensor_alpha<DT, PLANAR, BGR, 3, TENSOR_ALPHA_OVER_P>;
    }
}
template <int DT> TensorAlphaKernel tensor_alpha_kernel_of(bool planar, bool bgr, int policy)
{
    return planar ? (bgr ? tensor_alpha_kernel_as<DT, true, true>(policy) : tensor_alpha_kernel_as<DT, true, false>(policy))
                  : (bgr ? tensor_alpha_kernel_as<DT, false, true>(policy) : tensor_alpha_kernel_as<DT, false, false>(policy));
}
TensorAlphaKernel tensor_alpha_kernel(const ffhip_tensor_format *f, int policy)
{
    const bool planar = f->planar != 0, bgr = f->bgr != 0;
    return f->dtype == FFHIP_TENSOR_U8 ? tensor_alpha_kernel_of<FFHIP_TENSOR_U8>(planar, bgr, policy)
         : f->dtype == FFHIP_TENSOR_F16 ? tensor_alpha_kernel_of<FFHIP_TENSOR_F16>(planar, bgr, policy)
                                        : tensor_alpha_kernel_of<FFHIP_TENSOR_F32>(planar, bgr, policy);
}

/* a record with a mode other than DROP: does anything of it take part */
bool tensor_alpha_on(const ffhip_tensor_alpha *a) { return a && a->mode != FFHIP_ALPHA_DROP; }
int tensor_channels(const ffhip_tensor_alpha *a) { return tensor_alpha_on(a) && a->mode != FFHIP_ALPHA_OVER ? 4 : 3; }
/* the policy a mode comes to with a straight or a premultiplied source */
int tensor_alpha_policy(const ffhip_tensor_alpha *a)
{
    const bool pre = a->source_premultiplied != 0;
    if (a->mode == FFHIP_ALPHA_STRAIGHT) return pre ? TENSOR_ALPHA_UNPREMUL : TENSOR_ALPHA_KEEP;
    if (a->mode == FFHIP_ALPHA_PREMULTIPLIED) return pre ? TENSOR_ALPHA_KEEP : TENSOR_ALPHA_PREMUL;
    return pre ? TENSOR_ALPHA_OVER_P : TENSOR_ALPHA_OVER_S;
}
bool tensor_alpha_ok(const ffhip_tensor_alpha *a, const ffhip_tensor_format *f)
{
    if (!tensor_alpha_on(a)) return true; /* the rest of the record is not read */
    if (a->mode < FFHIP_ALPHA_DROP || a->mode > FFHIP_ALPHA_OVER || (a->source_premultiplied != 0 && a->source_premultiplied != 1)) return false;
    if (!isfinite(a->alpha_scale) || !isfinite(a->alpha_bias)) return false;
    return !(f->dtype == FFHIP_TENSOR_U8 && (a->alpha_scale != 1.0f || a->alpha_bias != 0.0f));
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

/* an item the call takes under format f, its picture's address aside (the file calls plan their items before their pictures have one);
 * fills its record (src and first_wg aside) */
bool tensor_item_layout(const ffhip_tensor_item &it, const ffhip_tensor_format *f, int nc, TensorItemDesc *out)
{
    const int es = tensor_elem_size(f->dtype);
    if (it.width < 1 || it.height < 1 || it.x0 < 0 || it.y0 < 0) return false;
    if (it.pitch < 4 || (it.pitch & 3)) return false;
    /* source offsets stay within 31 bits, as the decode calls' own pictures do (pitch x rows < 2^31), and the rectangle within the pitch */
    if (4LL * ((long long)it.x0 + it.width) > it.pitch || ((long long)it.y0 + it.height) * it.pitch > 0x7fffffffLL) return false;
    if (!it.d_out || ((uintptr_t)it.d_out & (uintptr_t)(es - 1))) return false;
    const long long run_len = f->planar ? it.width : (long long)nc * it.width;
    if (it.row_stride < run_len) return false;
    __int128 span = (__int128)it.row_stride * (it.height - 1) + run_len; /* elements from the first to behind the last of a plane (HWC: of the tensor) */
    if (f->planar) {
        if ((__int128)it.plane_stride < span) return false;
        span += (__int128)it.plane_stride * (nc - 1);
    }
    if (span * es > ((__int128)1 << 62)) return false; /* element offsets are 64-bit in the kernel */
    const long long runs = (f->planar ? (long long)nc : 1LL) * it.height;
    const long long units = (run_len * es + 15) / 16 + 1;
    if (runs * units > 0xffffffffLL) return false; /* a unit's index is 32-bit */
    memset(out, 0, sizeof(*out));
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

/* an item the call takes under format f; fills its record (first_wg aside) */
bool tensor_item_desc(const ffhip_tensor_item &it, const ffhip_tensor_format *f, int nc, TensorItemDesc *out)
{
    if (!it.d_bgra || ((uintptr_t)it.d_bgra & 3) || !tensor_item_layout(it, f, nc, out)) return false;
    out->src = it.d_bgra + (long long)it.y0 * it.pitch + 4LL * it.x0;
    return true;
}

/* both items calls: alpha NULL or of mode DROP is the three-channel call */
int tensor_items(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, const ffhip_tensor_alpha *alpha, void *stream)
{
    if (n < 0 || (n > 0 && !items) || !tensor_format_ok(fmt) || !tensor_alpha_ok(alpha, fmt)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    const int nc = tensor_channels(alpha);
    /* the records, every item's workgroups behind those of the items before it */
    std::vector<TensorItemDesc> desc((size_t)n);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (!tensor_item_desc(items[i], fmt, nc, &desc[(size_t)i])) return FFHIP_EINVAL;
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
    if (tensor_alpha_on(alpha)) {
        const TensorAlphaKernel kernel = tensor_alpha_kernel(fmt, tensor_alpha_policy(alpha));
        return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
            TensorAlphaArgs a;
            a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
            for (int c = 0; c < 3; c++) { a.s.scale[c] = fmt->scale[c]; a.s.bias[c] = fmt->bias[c]; }
            a.al.background = (u32)alpha->background[0] | (u32)alpha->background[1] << 8 | (u32)alpha->background[2] << 16;
            a.al.alpha_scale = alpha->alpha_scale; a.al.alpha_bias = alpha->alpha_bias;
            hipLaunchKernelGGL(kernel, dim3(grid_x), dim3(FFHIP_TENSOR_WG_THREADS), 0, st, a);
        });
    }
    const TensorKernel kernel = tensor_kernel(fmt);
    return ffhip_items_launch(0, total, [&](unsigned grid_x, u32 wg_base) {
        TensorArgs a;
        a.desc = d_desc; a.wg_item = d_table; a.wg_base = wg_base;
        for (int c = 0; c < 3; c++) { a.s.scale[c] = fmt->scale[c]; a.s.bias[c] = fmt->bias[c]; }
        hipLaunchKernelGGL(kernel, dim3(grid_x), dim3(FFHIP_TENSOR_WG_THREADS), 0, st, a);
    });
}

} // namespace

extern "C" int ffhip_bgra_to_tensor_items(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, void *stream)
{
    return tensor_items(items, n, fmt, nullptr, stream);
}

extern "C" int ffhip_bgra_to_tensor_items_alpha(const ffhip_tensor_item *items, int n, const ffhip_tensor_format *fmt, const ffhip_tensor_alpha *alpha,
                                                void *stream)
{
    return tensor_items(items, n, fmt, alpha, stream);
}

/* ---- files in, tensors out ---- */
namespace {

struct TensorPicture { int coded_w, coded_h, width, height; int64_t pitch; }; /* what a decode call writes; what the file displays (inside it); its row bytes */
struct TensorProbe { int code; TensorPicture pic; };                          /* a codec's word on a file: pic (at full size) is valid where code == 0 */
typedef int (*TensorTag)(const uint8_t *file, size_t len, int *orientation);   /* a codec's reader of the EXIF orientation */
thread_local int g_tensor_last_parts = 0; /* ffhip_debug_tensor_last_parts */
thread_local int g_orient_last_items = 0; /* ffhip_debug_orient_last_items */
/* decodes files [first, first + cnt) into d_bgra[k] with pitch[k]: the call underneath, its per-file codes into status + first */
typedef std::function<int(int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch)> TensorDecode;

/* What an entry point was asked for behind the files, the format and the outputs.  roi and out_size are the caller's: UPRIGHT axes, full
 * size.  out_size == NULL: every file keeps its rectangle's size.  denom == NULL: every file at full size; otherwise file i at
 * 1 / denom[i], 0 for the largest denominator at which its rectangle still covers out_size[i].  oriented: the calls that turn pictures
 * upright, orient[i] 1..8 or 0 ("the file's tag"), orient == NULL: every file's tag */
struct TensorOptions {
    explicit TensorOptions(const ffhip_rect *r) : roi(r) {}
    TensorOptions &resize(const ffhip_size *s, int f) { out_size = s; filter = f; return *this; }
    TensorOptions &scale(const int *d, int *d_out) { denom = d; denom_out = d_out; return *this; }
    TensorOptions &turn(const int *o, int *o_out) { oriented = true; orient = o; orient_out = o_out; return *this; }
    TensorOptions &with(unsigned f) { flags = f; return *this; }
    TensorOptions &keep(const ffhip_tensor_alpha *a) { alpha = a; return *this; }
    TensorOptions &png(unsigned f) { png_flags = f; return *this; }
    const ffhip_rect *roi;
    const ffhip_size *out_size = nullptr;
    int filter = FFHIP_RESIZE_BILINEAR;
    const int *denom = nullptr, *orient = nullptr;
    int *denom_out = nullptr, *orient_out = nullptr;
    bool oriented = false;
    unsigned flags = 0u;
    unsigned png_flags = 0u; /* the PNG calls': FFHIP_PNG_INFLATE_DEVICE */
    const ffhip_tensor_alpha *alpha = nullptr; /* NULL or mode DROP: three channels, the alpha byte ignored.  Otherwise the resize is the
                                                * premultiplying one and the sink is told so */
};

/* One file of a call, planned once (tensor_file_plan) and only read afterwards */
struct TensorFile {
    int code = FFHIP_OK;         /* the probe's, or this call's own FFHIP_EINVAL; 0: the file takes part */
    bool refused_here = false;   /* code is this call's: the decoder still gets the file, and its code comes first */
    TensorPicture pic = {};      /* what the decoder writes: the SCALED picture where there is a denominator */
    ffhip_rect rect = {};        /* the rectangle of that picture to deliver: stored axes, mapped by the denominator */
    ffhip_size resized = {0, 0}; /* {0, 0}: no resize; stored axes */
    int orient = 1, denom = 1;   /* 1..8; 1, 2, 4, 8 */
    ffhip_tensor_item sink = {}; /* everything but d_bgra */
    size_t decoded_bytes = 0, resized_bytes = 0, upright_bytes = 0; /* the pictures' places in part scratch, 0 where the stage is not taken */
};

size_t tensor_place(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

/* a BGRA rectangle on its way through a file's stages */
struct TensorView { uint8_t *ptr; int64_t pitch; int x0, y0, width, height; };
TensorView tensor_whole(uint8_t *ptr, int width, int height) { return TensorView{ptr, 4LL * width, 0, 0, width, height}; }

/* File f's stages, from its picture at `decoded` to what the sink reads: the rectangle; where f is resized, *s takes the rectangle to the
 * whole picture at `small`; where f is turned, *t takes that to the whole upright picture at `upright`.  The planner runs it without
 * addresses, the part loop with the part's */
TensorView tensor_chain(const TensorFile &f, uint8_t *decoded, uint8_t *small, uint8_t *upright, ffhip_resize_item *s, ffhip_orient_item *t)
{
    TensorView v{decoded, f.pic.pitch, f.rect.x0, f.rect.y0, f.rect.width, f.rect.height};
    if (f.resized.width) {
        const TensorView to = tensor_whole(small, f.resized.width, f.resized.height);
        *s = ffhip_resize_item{v.ptr, v.pitch, v.x0, v.y0, v.width, v.height, to.ptr, to.pitch, to.width, to.height};
        v = to;
    }
    if (f.orient != 1) {
        const bool swap = FFHIP_ORIENT_TRANSPOSE(f.orient);
        const TensorView to = tensor_whole(upright, swap ? v.height : v.width, swap ? v.width : v.height);
        *t = ffhip_orient_item{v.ptr, v.pitch, v.x0, v.y0, v.width, v.height, to.ptr, to.pitch, f.orient};
        v = to;
    }
    return v;
}

/* File i's record, from the probe's word p and the orientation o it is delivered at (1 where the call turns nothing).  Everything a call
 * decides about a file's rectangle, sizes and output is decided here, without the device; what it writes besides the record is
 * denom_out[i] and orient_out[i] (0 for a file the probe refused) */
TensorFile tensor_file_plan(const TensorProbe &p, int o, int i, const TensorOptions &opts, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs)
{
    TensorFile f;
    f.code = p.code;
    f.pic = p.pic;
    if (opts.oriented && opts.orient_out) opts.orient_out[i] = p.code ? 0 : o;
    if (opts.denom && opts.denom_out) opts.denom_out[i] = 0;
    if (p.code) return f;
    const bool swap = FFHIP_ORIENT_TRANSPOSE(o);
    const int w = p.pic.width, h = p.pic.height, uw = swap ? h : w, uh = swap ? w : h; /* full size: stored, upright */
    const ffhip_rect asked = opts.roi ? opts.roi[i] : ffhip_rect{0, 0, uw, uh};
    bool ok = asked.x0 >= 0 && asked.y0 >= 0 && asked.width >= 1 && asked.height >= 1 && (long long)asked.x0 + asked.width <= uw &&
              (long long)asked.y0 + asked.height <= uh;
    ffhip_rect r = asked; /* in the stored axes */
    if (ok && o != 1) ok = ffhip_orient_rect(w, h, o, &asked, &r) == FFHIP_OK;
    const ffhip_size to = !opts.out_size ? ffhip_size{0, 0} : swap ? ffhip_size{opts.out_size[i].height, opts.out_size[i].width} : opts.out_size[i];
    if (opts.denom) { /* the decoder's picture is the scaled one: sizes rounded up, a pitch rounded up to 16 bytes */
        int d = opts.denom[i];
        if (d == 0) d = ok && to.width >= 1 && to.height >= 1 ? ffhip_jpeg_scale_choose(r.width, r.height, to.width, to.height) : 1;
        if (opts.denom_out) opts.denom_out[i] = d;
        const int cw = p.pic.coded_w / d;
        f.denom = d;
        f.pic = TensorPicture{cw, p.pic.coded_h / d, jpeg_scaled_len(w, d), jpeg_scaled_len(h, d), (4LL * cw + 15) & ~15LL};
        if (ok) r = jpeg_scaled_rect_of(w, h, d, r);
    }
    f.decoded_bytes = tensor_place((size_t)f.pic.pitch * f.pic.coded_h);
    if (ok && opts.out_size) /* the rectangle is the resize's source */
        ok = r.width <= FFHIP_RESIZE_MAX_SIDE && r.height <= FFHIP_RESIZE_MAX_SIDE && to.width >= 1 && to.width <= FFHIP_RESIZE_MAX_SIDE &&
             to.height >= 1 && to.height <= FFHIP_RESIZE_MAX_SIDE;
    if (ok) {
        f.rect = r;
        f.resized = to;
        f.orient = o;
        ffhip_resize_item s;
        ffhip_orient_item t;
        const TensorView v = tensor_chain(f, nullptr, nullptr, nullptr, &s, &t);
        /* what the sink checks of its source, the orient stage checks of its own */
        if (o != 1) ok = ((long long)t.y0 + t.height) * t.src_pitch <= 0x7fffffffLL;
        f.sink = ffhip_tensor_item{nullptr, v.pitch, v.x0, v.y0, v.width, v.height, outs[i].d_out, outs[i].row_stride, outs[i].plane_stride};
        TensorItemDesc d;
        ok = ok && tensor_item_layout(f.sink, fmt, tensor_channels(opts.alpha), &d);
        f.resized_bytes = to.width ? tensor_place((size_t)4 * to.width * to.height) : 0;
        f.upright_bytes = o != 1 ? tensor_place((size_t)4 * v.width * v.height) : 0;
    }
    if (!ok) { /* the file still goes to the decoder, which may have a code of its own for it; no stage behind it takes it */
        f.code = FFHIP_EINVAL;
        f.refused_here = true;
        f.resized_bytes = f.upright_bytes = 0;
    }
    return f;
}

/* a part: files while their pictures fit the budget; a picture larger than the budget is a part of its own */
struct TensorPart { int first, cnt; size_t decoded, resized, upright; };

TensorPart tensor_part_extent(const std::vector<TensorFile> &plan, int first, size_t budget)
{
    TensorPart p{first, 0, 0, 0, 0};
    for (; (size_t)(first + p.cnt) < plan.size(); p.cnt++) {
        const TensorFile &f = plan[(size_t)(first + p.cnt)];
        if (p.cnt && p.decoded + p.resized + p.upright + f.decoded_bytes + f.resized_bytes + f.upright_bytes > budget) break;
        p.decoded += f.decoded_bytes;
        p.resized += f.resized_bytes;
        p.upright += f.upright_bytes;
    }
    return p;
}

/* the part's pictures, one behind the other from *base on, each at its record's pitch.  Returns what ends the call: a decoder return that
 * is none of the part's file codes */
int tensor_part_decode(const std::vector<TensorFile> &plan, const TensorPart &p, const int *status, void *stream, const TensorDecode &decode, uint8_t **base)
{
    *base = (uint8_t *)ffhip_scratch(SCRATCH_TENSOR_BGRA, stream, p.decoded / 4 + 64);
    if (!*base) return FFHIP_ENOMEM;
    std::vector<uint8_t *> d_bgra((size_t)p.cnt);
    std::vector<int64_t> pitch((size_t)p.cnt);
    size_t at = 0;
    for (int k = 0; k < p.cnt; k++) { /* (a file the probe refused: the decoder refuses it again before it looks at its output) */
        const TensorFile &f = plan[(size_t)(p.first + k)];
        d_bgra[(size_t)k] = *base + at;
        pitch[(size_t)k] = f.code && !f.refused_here ? 0 : f.pic.pitch;
        at += f.decoded_bytes;
    }
    g_tensor_last_parts++;
    const int rc = decode(p.first, p.cnt, d_bgra.data(), pitch.data());
    for (int k = 0; rc && k < p.cnt; k++)
        if (status[p.first + k] == rc) return FFHIP_OK; /* a file's code */
    return rc;
}

/* behind the decoder: every file it delivered through its stages, at most one call per stage with the items in file order; a file this
 * call refuses gets its code here */
int tensor_part_enqueue(const std::vector<TensorFile> &plan, const TensorPart &p, uint8_t *base, const TensorOptions &opts, const ffhip_tensor_format *fmt,
                        int *status, void *stream)
{
    uint8_t *small = nullptr; /* the part's resized pictures, pitch 4 x out width */
    if (opts.out_size && !(small = (uint8_t *)ffhip_scratch(SCRATCH_RESIZE_BGRA, stream, p.resized / 4 + 64))) return FFHIP_ENOMEM;
    uint8_t *upright = nullptr; /* the part's upright pictures, pitch 4 x upright width */
    if (p.upright && !(upright = (uint8_t *)ffhip_scratch(SCRATCH_ORIENT_BGRA, stream, p.upright / 4 + 64))) return FFHIP_ENOMEM;
    std::vector<ffhip_resize_item> shrink;
    std::vector<ffhip_orient_item> turn;
    std::vector<ffhip_tensor_item> good;
    good.reserve((size_t)p.cnt);
    for (int k = 0; k < p.cnt; k++) {
        const int i = p.first + k;
        const TensorFile &f = plan[(size_t)i];
        uint8_t *decoded = base;
        base += f.decoded_bytes;
        if (status[i]) continue;
        if (f.refused_here) { status[i] = f.code; continue; }
        ffhip_resize_item s;
        ffhip_orient_item t;
        ffhip_tensor_item sink = f.sink;
        sink.d_bgra = tensor_chain(f, decoded, small, upright, &s, &t).ptr;
        if (f.resized_bytes) { shrink.push_back(s); small += f.resized_bytes; }
        if (f.upright_bytes) { turn.push_back(t); upright += f.upright_bytes; }
        good.push_back(sink);
    }
    const bool with_alpha = tensor_alpha_on(opts.alpha);
    if (opts.out_size) {
        const int rc = with_alpha ? ffhip_bgra_resize_items_premultiplied(shrink.data(), (int)shrink.size(), opts.filter, stream)
                                  : ffhip_bgra_resize_items(shrink.data(), (int)shrink.size(), opts.filter, stream);
        if (rc) return rc;
    }
    if (!turn.empty()) {
        const int rc = ffhip_bgra_orient_items(turn.data(), (int)turn.size(), stream);
        if (rc) return rc;
        g_orient_last_items += (int)turn.size();
    }
    if (!with_alpha) return ffhip_bgra_to_tensor_items(good.data(), (int)good.size(), fmt, stream);
    ffhip_tensor_alpha sink_alpha = *opts.alpha;
    sink_alpha.source_premultiplied = opts.out_size ? 1 : 0; /* every file of a call with targets went through the resize */
    return ffhip_bgra_to_tensor_items_alpha(good.data(), (int)good.size(), fmt, &sink_alpha, stream);
}

/* The driver: the planned files part by part -- decode, the stages behind it, one synchronisation (the next part decodes into the same
 * scratch).  status[i] holds the probe's code on entry; behind it the decoder's, then this call's own.  Returns the first file's code */
int tensor_files_run(const std::vector<TensorFile> &plan, const TensorOptions &opts, const ffhip_tensor_format *fmt, int *status, void *stream,
                     const TensorDecode &decode)
{
    g_tensor_last_parts = 0; /* a call that returns before its first part has taken none */
    g_orient_last_items = 0;
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    const size_t budget = ffhip_part_budget(FFHIP_ENV("FFHIP_TENSOR_PART_BYTES"));
    for (int first = 0; (size_t)first < plan.size();) {
        const TensorPart p = tensor_part_extent(plan, first, budget);
        uint8_t *base = nullptr;
        int rc = tensor_part_decode(plan, p, status, stream, decode, &base);
        if (!rc) rc = tensor_part_enqueue(plan, p, base, opts, fmt, status, stream);
        if (rc) return rc;
        FFHIP_CHECK(hipStreamSynchronize((hipStream_t)stream), FFHIP_EIO);
        first += p.cnt;
    }
    for (size_t i = 0; i < plan.size(); i++)
        if (status[i]) return status[i];
    return FFHIP_OK;
}

/* what every entry refuses before it looks at a file */
bool tensor_files_args_ok(const uint8_t *const *files, const size_t *lens, int n, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs, const int *status,
                          const TensorOptions &opts)
{
    if (n < 0 || !tensor_format_ok(fmt) || (n > 0 && !(files && lens && outs && status))) return false;
    if (!tensor_alpha_ok(opts.alpha, fmt) || (tensor_alpha_on(opts.alpha) && opts.alpha->source_premultiplied)) return false;
    if (opts.filter != FFHIP_RESIZE_BILINEAR && opts.filter != FFHIP_RESIZE_ANTIALIAS) return false;
    for (int i = 0; opts.oriented && opts.orient && i < n; i++)
        if (opts.orient[i] < 0 || opts.orient[i] > 8) return false;
    return true;
}

/* the orientation file i is delivered at: the caller's, or the file's tag */
int tensor_orientation(const TensorOptions &opts, int i, const TensorProbe &p, TensorTag tag, const uint8_t *file, size_t len)
{
    if (!opts.oriented) return 1;
    int o = opts.orient ? opts.orient[i] : 0;
    if (!p.code && o == 0) tag(file, len, &o);
    return o;
}

/* The codecs: they differ in their probe and in the call underneath */
int jpeg_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs,
                      const TensorOptions &opts, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    const unsigned flags = opts.flags;
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status, opts) || (flags & ~(FFHIP_JPEG_ACCEPT_PROGRESSIVE | FFHIP_JPEG_PIXELS_LIBJPEG))) return FFHIP_EINVAL;
    for (int i = 0; opts.denom && i < n; i++) {
        if (opts.denom[i] != 0 ? !jpeg_denom_ok(opts.denom[i]) : !opts.out_size) return FFHIP_EINVAL;
        if ((flags & FFHIP_JPEG_PIXELS_LIBJPEG) && opts.denom[i] != 1) return FFHIP_EINVAL; /* libjpeg's pixels: full size only, "choose" included */
    }
    if (n == 0) return FFHIP_OK;
    std::vector<TensorFile> plan((size_t)n);
    ffhip_parallel_for(n, n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads), [&](int i) {
        const JpegProbed probed = jpeg_probe_file(files[i], lens[i], flags);
        const ffhip_jpeg_geom &g = probed.geom;
        status[i] = probed.status;
        if (geom_out) geom_out[i] = g;
        const TensorProbe p{probed.status, TensorPicture{g.mcu_cols * 8 * g.h, g.mcu_rows * 8 * g.v, probed.width, probed.height, 4LL * g.mcu_cols * 8 * g.h}};
        plan[(size_t)i] = tensor_file_plan(p, tensor_orientation(opts, i, p, ffhip_jpeg_exif_orientation, files[i], lens[i]), i, opts, fmt, outs);
    });
    int prog_total[5] = {0, 0, 0, 0, 0}; /* the parts' ffhip_debug_progressive_last, summed (the front end: the last part's) */
    const int rc = tensor_files_run(plan, opts, fmt, status, stream, [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        std::vector<int> den(opts.denom ? (size_t)cnt : 0); /* the part's denominators, as the call underneath reads them */
        for (size_t k = 0; k < den.size(); k++) den[k] = plan[(size_t)first + k].denom;
        const int prc = jpeg_decode_files_mixed(files + first, lens + first, cnt, n_threads, d_bgra, pitch, opts.denom ? den.data() : nullptr, flags,
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
                      const TensorOptions &opts, ffhip_webp_info *info_out, int *status, void *stream)
{
    const unsigned flags = opts.flags; /* FFHIP_WEBP_PIXELS_LIBWEBP: probe and decode under that rule; the planner and the chain do not know */
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status, opts) || (flags & ~FFHIP_WEBP_PIXELS_LIBWEBP)) return FFHIP_EINVAL;
    const bool with_alpha = tensor_alpha_on(opts.alpha);
    if (with_alpha && !(flags & FFHIP_WEBP_PIXELS_LIBWEBP)) return FFHIP_EINVAL; /* the reference rule has no alpha */
    const unsigned decode_flags = flags | (with_alpha ? FFHIP_WEBP_ALPHA : 0u);  /* the probe knows no alpha bit */
    if (n == 0) return FFHIP_OK;
    std::vector<TensorFile> plan((size_t)n);
    for (int i = 0; i < n; i++) {
        int w = 0, h = 0, c = 0, r = 0;
        status[i] = files[i] && lens[i] ? ffhip_webp_probe_ex(files[i], lens[i], flags, &w, &h, &c, &r) : FFHIP_EINVAL;
        /* the loader's size is the container's word (ffhip_webp_info): what of it the decoded picture holds */
        const TensorProbe p{status[i], TensorPicture{16 * c, 16 * r, w < 16 * c ? w : 16 * c, h < 16 * r ? h : 16 * r, 64LL * c}};
        plan[(size_t)i] = tensor_file_plan(p, tensor_orientation(opts, i, p, ffhip_webp_exif_orientation, files[i], lens[i]), i, opts, fmt, outs);
    }
    return tensor_files_run(plan, opts, fmt, status, stream, [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        return ffhip_webp_decode_files_device_ex(files + first, lens + first, cnt, n_threads, d_bgra, pitch, nullptr, decode_flags,
                                                 info_out ? info_out + first : nullptr, status + first, stream);
    });
}

int png_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs,
                     const TensorOptions &opts, ffhip_png_info *info_out, int *status, void *stream)
{
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status, opts) || opts.flags || (opts.png_flags & ~FFHIP_PNG_INFLATE_DEVICE)) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    std::vector<TensorFile> plan((size_t)n);
    for (int i = 0; i < n; i++) {
        ffhip_png_info info = {};
        status[i] = files[i] && lens[i] ? ffhip_png_probe(files[i], lens[i], &info) : FFHIP_EINVAL;
        const int cw = (info.width + 3) & ~3; /* the file call's pictures: rows of whole 16-byte groups */
        const TensorProbe p{status[i], TensorPicture{cw, info.height, info.width, info.height, 4LL * cw}};
        plan[(size_t)i] = tensor_file_plan(p, tensor_orientation(opts, i, p, ffhip_png_exif_orientation, files[i], lens[i]), i, opts, fmt, outs);
    }
    return tensor_files_run(plan, opts, fmt, status, stream, [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        return ffhip_png_decode_files_device_ex(files + first, lens + first, cnt, n_threads, d_bgra, pitch, info_out ? info_out + first : nullptr,
                                                status + first, opts.png_flags, stream);
    });
}

int vp8l_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt, const ffhip_tensor_out *outs,
                      const TensorOptions &opts, ffhip_vp8l_info *info_out, int *status, void *stream)
{
    if (!tensor_files_args_ok(files, lens, n, fmt, outs, status, opts) || opts.flags) return FFHIP_EINVAL;
    if (n == 0) return FFHIP_OK;
    std::vector<TensorFile> plan((size_t)n);
    for (int i = 0; i < n; i++) {
        int w = 0, h = 0, alpha = 0;
        status[i] = files[i] && lens[i] ? ffhip_vp8l_probe(files[i], lens[i], &w, &h, &alpha) : FFHIP_EINVAL;
        const int cw = (w + 3) & ~3; /* the file call's pictures: rows of whole 16-byte groups */
        const TensorProbe p{status[i], TensorPicture{cw, h, w, h, 4LL * cw}};
        plan[(size_t)i] = tensor_file_plan(p, tensor_orientation(opts, i, p, ffhip_webp_exif_orientation, files[i], lens[i]), i, opts, fmt, outs);
    }
    return tensor_files_run(plan, opts, fmt, status, stream, [&](int first, int cnt, uint8_t *const *d_bgra, const int64_t *pitch) {
        return ffhip_vp8l_decode_files_device(files + first, lens + first, cnt, n_threads, d_bgra, pitch, info_out ? info_out + first : nullptr,
                                              status + first, stream);
    });
}

} // namespace

extern "C" int ffhip_jpeg_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                              const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi), geom_out, status, stream);
}

extern "C" int ffhip_webp_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                              const ffhip_tensor_out *outs, const ffhip_rect *roi, ffhip_webp_info *info_out, int *status, void *stream)
{
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi), info_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                      ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (n > 0 && !out_size) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter), geom_out, status, stream);
}

extern "C" int ffhip_webp_decode_files_tensor_resized(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                      const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                      ffhip_webp_info *info_out, int *status, void *stream)
{
    if (n > 0 && !out_size) return FFHIP_EINVAL;
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter), info_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_scaled(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                     const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                     const int *denom, int *denom_out, ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    if (n > 0 && !denom) return FFHIP_EINVAL;
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).scale(denom, denom_out), geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                       const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                       const int *denom, int *denom_out, const int *orient, int *orient_out,
                                                       ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).scale(denom, denom_out).turn(orient, orient_out),
                             geom_out, status, stream);
}

extern "C" int ffhip_jpeg_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                 const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                 const int *denom, int *denom_out, const int *orient, int *orient_out, unsigned flags,
                                                 ffhip_jpeg_geom *geom_out, int *status, void *stream)
{
    return jpeg_files_tensor(files, lens, n, n_threads, fmt, outs,
                             TensorOptions(roi).resize(out_size, filter).scale(denom, denom_out).turn(orient, orient_out).with(flags), geom_out, status, stream);
}

extern "C" int ffhip_webp_decode_files_tensor_oriented(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                       const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                       const int *orient, int *orient_out, ffhip_webp_info *info_out, int *status, void *stream)
{
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out), info_out, status, stream);
}

extern "C" int ffhip_debug_tensor_last_parts(void) { return g_tensor_last_parts; }
extern "C" int ffhip_debug_orient_last_items(void) { return g_orient_last_items; }

extern "C" int ffhip_webp_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                 const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                 const int *orient, int *orient_out, unsigned flags, ffhip_webp_info *info_out, int *status, void *stream)
{
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags), info_out,
                             status, stream);
}

extern "C" int ffhip_png_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                             const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                             const int *orient, int *orient_out, unsigned flags, ffhip_png_info *info_out, int *status, void *stream)
{
    return png_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags), info_out,
                            status, stream);
}

extern "C" int ffhip_vp8l_decode_files_tensor(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                              const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                              const int *orient, int *orient_out, unsigned flags, ffhip_vp8l_info *info_out, int *status, void *stream)
{
    return vp8l_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags), info_out,
                             status, stream);
}

/* the calls with the alpha record: the same code, the existing entries being alpha == NULL */
extern "C" int ffhip_webp_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                    const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                    const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                                    ffhip_webp_info *info_out, int *status, void *stream)
{
    return webp_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags).keep(alpha),
                             info_out, status, stream);
}

extern "C" int ffhip_png_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                   const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                   const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                                   ffhip_png_info *info_out, int *status, void *stream)
{
    return png_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags).keep(alpha),
                            info_out, status, stream);
}

extern "C" int ffhip_png_decode_files_tensor_ex(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                                unsigned png_flags, ffhip_png_info *info_out, int *status, void *stream)
{
    return png_files_tensor(files, lens, n, n_threads, fmt, outs,
                            TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags).keep(alpha).png(png_flags), info_out, status, stream);
}

extern "C" int ffhip_vp8l_decode_files_tensor_alpha(const uint8_t *const *files, const size_t *lens, int n, int n_threads, const ffhip_tensor_format *fmt,
                                                    const ffhip_tensor_out *outs, const ffhip_rect *roi, const ffhip_size *out_size, int filter,
                                                    const int *orient, int *orient_out, unsigned flags, const ffhip_tensor_alpha *alpha,
                                                    ffhip_vp8l_info *info_out, int *status, void *stream)
{
    return vp8l_files_tensor(files, lens, n, n_threads, fmt, outs, TensorOptions(roi).resize(out_size, filter).turn(orient, orient_out).with(flags).keep(alpha),
                             info_out, status, stream);
}
