"""Decoded pictures as torch tensors on the device (include/ffpic_hip.h, "decoded pictures into tensors"): files in, RGB / BGR,
CHW / HWC, uint8 / float16 / float32 tensors out, nothing but the compressed bytes crossing PCIe.  torch is imported when a
function here is called, not with the package: ffpic_amd.ops stays torch-free."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi, ops

_DTYPES = {"uint8": capi.FFHIP_TENSOR_U8, "float16": capi.FFHIP_TENSOR_F16, "float32": capi.FFHIP_TENSOR_F32}


def _dtype_name(dtype):
    name = "uint8" if dtype is None else str(np.dtype(dtype)) if not str(dtype).startswith("torch.") else str(dtype)[6:]
    name = {"half": "float16", "float": "float32"}.get(name, name)
    if name not in _DTYPES:
        raise ValueError(f"dtype {dtype!r}: uint8, float16 or float32")
    return name


def tensor_format(dtype=None, layout="CHW", order="RGB", mean=None, std=None):
    """capi.TensorFormat.  mean / std: per OUTPUT channel on a 0..1 scale; scale = float32(1 / (255 std)), bias = float32(-mean / std),
    computed in doubles and rounded once.  With neither, scale 1 and bias 0: a float output holds the byte values."""
    name = _dtype_name(dtype)
    if layout not in ("CHW", "HWC") or order not in ("RGB", "BGR"):
        raise ValueError("layout is 'CHW' or 'HWC', order 'RGB' or 'BGR'")
    f = capi.TensorFormat()
    f.dtype, f.bgr, f.planar = _DTYPES[name], int(order == "BGR"), int(layout == "CHW")
    if mean is None and std is None:
        scale, bias = [1.0] * 3, [0.0] * 3
    else:
        if name == "uint8":
            raise ValueError("mean / std need a float dtype")
        mean = [0.0] * 3 if mean is None else [float(m) for m in mean]
        std = [1.0] * 3 if std is None else [float(s) for s in std]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one value per channel")
        scale, bias = [1.0 / (255.0 * s) for s in std], [-m / s for m, s in zip(mean, std)]
    for c in range(3):
        f.scale[c], f.bias[c] = scale[c], bias[c]      # ctypes rounds the double to float32, once
    return f


_ALPHA_MODES = {"drop": capi.FFHIP_ALPHA_DROP, "straight": capi.FFHIP_ALPHA_STRAIGHT, "premultiplied": capi.FFHIP_ALPHA_PREMULTIPLIED,
                "over": capi.FFHIP_ALPHA_OVER}


def _alpha_arg(alpha):
    """alpha='drop' | 'straight' | 'premultiplied' | ('over', (r, g, b)) -> (mode name, (r, g, b) or None); anything else: ValueError"""
    if isinstance(alpha, str) and alpha in ("drop", "straight", "premultiplied"):
        return alpha, None
    if isinstance(alpha, (tuple, list)) and len(alpha) == 2 and alpha[0] == "over":
        try:
            rgb = tuple(alpha[1])
        except TypeError:
            rgb = ()
        if len(rgb) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in rgb):
            return "over", tuple(int(v) for v in rgb)
    raise ValueError(f"alpha {alpha!r}: 'drop', 'straight', 'premultiplied' or ('over', (r, g, b)) with bytes r, g, b")


def tensor_alpha(alpha="drop", normalised=False, source_premultiplied=False):
    """capi.TensorAlpha for alpha='drop' | 'straight' | 'premultiplied' | ('over', (r, g, b)).  normalised: the alpha channel of a float
    output is alpha * float32(1 / 255), as the colours are on a 0..1 scale under mean / std; otherwise the byte value.
    source_premultiplied: the pictures the sink reads are premultiplied BGRA (what resize_bgra(..., premultiplied=True) leaves)."""
    mode, rgb = _alpha_arg(alpha)
    a = capi.TensorAlpha()
    a.mode, a.source_premultiplied = _ALPHA_MODES[mode], int(bool(source_premultiplied))
    if rgb:
        a.background[0], a.background[1], a.background[2] = rgb[2], rgb[1], rgb[0]
    a.alpha_scale, a.alpha_bias = (1.0 / 255.0 if normalised else 1.0), 0.0      # ctypes rounds the double to float32, once
    return a


def alpha_channels(alpha="drop"):
    """the channel count of the tensors under alpha=: 4 for 'straight' and 'premultiplied', 3 otherwise"""
    return 4 if _alpha_arg(alpha)[0] in ("straight", "premultiplied") else 3


def alpha_entry_point(codec, alpha="drop", pixels="reference", oriented=False, targets=False):
    """The C entry a files-to-tensors call of codec 'png', 'vp8l' or 'webp' goes through under alpha=: 'drop' is the entry the call took
    before there was the argument; every other value is the codec's _alpha entry, which WebP has under pixels='libwebp' only (the
    reference rule has no alpha: ValueError).  Needs neither torch nor the library."""
    if codec not in ("png", "vp8l", "webp"):
        raise ValueError(f"{codec!r}: 'png', 'vp8l' or 'webp' -- the codecs whose files can have alpha")
    flags = ops.webp_pixel_flags(pixels) if codec == "webp" else 0
    if _alpha_arg(alpha)[0] == "drop":
        return f"ffhip_{codec}_decode_files_tensor" if codec != "webp" else webp_entry_point(pixels, oriented, targets)
    if codec == "webp" and not flags:
        raise ValueError("alpha needs pixels='libwebp': the reference rule decodes no alpha plane")
    return f"ffhip_{codec}_decode_files_tensor_alpha"


def bgra_to_tensors(items, fmt, stream=None, alpha=None):
    """ffhip_bgra_to_tensor_items: `items` a list of capi.TensorItem (device pointers, strides in elements), `fmt` a capi.TensorFormat;
    one launch for the whole batch.  alpha: None, or a capi.TensorAlpha (tensor_alpha) -- ffhip_bgra_to_tensor_items_alpha: four
    channels, or three composited over a background.  Only enqueues on `stream` (a hipStream_t handle; None: the default stream)."""
    L = capi.lib()
    n = len(items)
    arr = (capi.TensorItem * max(n, 1))(*items)
    if alpha is None:
        capi.check(L.ffhip_bgra_to_tensor_items(arr, n, C.byref(fmt), stream), "ffhip_bgra_to_tensor_items")
    else:
        capi.check(L.ffhip_bgra_to_tensor_items_alpha(arr, n, C.byref(fmt), C.byref(alpha), stream), "ffhip_bgra_to_tensor_items_alpha")


def resize_bgra(items, antialias=True, stream=None, premultiplied=False):
    """ffhip_bgra_resize_items: `items` a list of capi.ResizeItem (device pointers, pitches in bytes), BGRA rectangles of any sizes to BGRA
    pictures of any sizes by the library's integer rule (antialias: the triangle widens with the shrink factor; otherwise two taps), one
    resize launch for the whole batch.  premultiplied=True: ffhip_bgra_resize_items_premultiplied -- straight BGRA in, every pixel
    premultiplied before it is filtered, premultiplied BGRA out: the colour under transparent pixels does not bleed into the edges.
    Only enqueues on `stream` (a hipStream_t handle; None: the default stream)."""
    L = capi.lib()
    n = len(items)
    arr = (capi.ResizeItem * max(n, 1))(*items)
    what = "ffhip_bgra_resize_items_premultiplied" if premultiplied else "ffhip_bgra_resize_items"
    capi.check(getattr(L, what)(arr, n, _filter(antialias), stream), what)


def orient_bgra(items, stream=None):
    """ffhip_bgra_orient_items: `items` a list of capi.OrientItem (device pointers, pitches in bytes, the STORED rectangle and its EXIF
    orientation 1..8), BGRA rectangles of any sizes turned upright, one launch for the whole batch.  Only enqueues on `stream` (a
    hipStream_t handle; None: the default stream)."""
    L = capi.lib()
    n = len(items)
    arr = (capi.OrientItem * max(n, 1))(*items)
    capi.check(L.ffhip_bgra_orient_items(arr, n, stream), "ffhip_bgra_orient_items")


def _filter(antialias):
    return capi.FFHIP_RESIZE_ANTIALIAS if antialias else capi.FFHIP_RESIZE_BILINEAR


def axis_taps(n_in, n_out, antialias=True):
    """ffhip_resize_axis_taps for every output index of an axis: (first[n_out] as an int array, a list of n_out uint16 weight arrays).
    Each array sums to 4096.  Needs no device."""
    L = capi.lib()
    first, taps = np.zeros(n_out, np.int64), []
    f = C.c_int()
    for o in range(n_out):
        count = L.ffhip_resize_axis_taps(n_in, n_out, _filter(antialias), o, C.byref(f), None, 0)
        capi.check(min(count, 0), "ffhip_resize_axis_taps")
        q = np.zeros(count, np.uint16)
        L.ffhip_resize_axis_taps(n_in, n_out, _filter(antialias), o, C.byref(f), q.ctypes.data_as(C.POINTER(C.c_uint16)), count)
        first[o] = f.value
        taps.append(q)
    return first, taps


def tensor_out(t, layout, channels=3):
    """capi.TensorOut of a torch tensor [3][H][W] (layout 'CHW') or [H][W][3] ('HWC') whose innermost dimension(s) are dense: a slice of a
    batch tensor, a view with padded rows.  channels=4: the tensors of the four-channel alpha modes"""
    if layout == "CHW":
        ok, rs, ps = t.dim() == 3 and t.shape[0] == channels and t.stride(2) == 1, t.stride(1), t.stride(0)
    else:
        ok, rs, ps = t.dim() == 3 and t.shape[2] == channels and t.stride(2) == 1 and t.stride(1) == channels, t.stride(0), 0
    if not ok:
        raise ValueError(f"a {layout} tensor with dense pixels is needed, got shape {tuple(t.shape)} strides {t.stride()}")
    return capi.TensorOut(t.data_ptr(), rs, ps)


def _rois(roi, n):
    if roi is None:
        return None
    if len(roi) == 4 and not hasattr(roi[0], "__len__"):
        roi = [roi] * n
    if len(roi) != n:
        raise ValueError("roi: one (x0, y0, width, height), or one per file")
    return [tuple(int(v) for v in r) for r in roi]


def _sizes(size, n):
    """size=(H, W) for all files or a list of one per file -> [(H, W)] * n"""
    if size is None:
        return None
    if len(size) == 2 and not hasattr(size[0], "__len__"):
        size = [size] * n
    if len(size) != n:
        raise ValueError("size: one (height, width), or one per file")
    size = [tuple(int(v) for v in s) for s in size]
    for s in size:
        if len(s) != 2 or min(s) < 1 or max(s) > capi.FFHIP_RESIZE_MAX_SIDE:
            raise ValueError(f"size {s}: (height, width), each in 1..{capi.FFHIP_RESIZE_MAX_SIDE}")
    return size


def _reduce(reduce, size):
    """reduce=1 | 2 | 4 | 8 | 'auto' -> the denominator for every file, 0 for 'auto' (the library chooses per file; needs size)"""
    if reduce == "auto":
        if size is None:
            raise ValueError("reduce='auto' needs size=: the denominator is chosen so that the picture still covers it")
        return 0
    if isinstance(reduce, bool) or reduce not in (1, 2, 4, 8):
        raise ValueError(f"reduce {reduce!r}: 1, 2, 4, 8 or 'auto'")
    return int(reduce)


def _orientations(orientation, n):
    """orientation=None | 1..8 | one per file -> [1..8] * n, None for None"""
    if orientation is None:
        return None
    imposed = [orientation] * n if not hasattr(orientation, "__len__") else list(orientation)
    if len(imposed) != n:
        raise ValueError("orientation: one value 1..8, or one per file")
    for o in imposed:
        if isinstance(o, bool) or o not in (1, 2, 3, 4, 5, 6, 7, 8):
            raise ValueError(f"orientation {o!r}: an EXIF orientation, 1..8")
    return [int(o) for o in imposed]


def entry_point(codec, oriented=False, den=1, targets=False, progressive=False, flags=0):
    """The C entry a files-to-tensors call goes through: codec 'jpeg' or 'webp' and what was asked for -- pictures turned upright, the
    denominator (0: chosen per file), target sizes, progressive files accepted, FFHIP_JPEG_* flags -> the symbol's name.  Needs neither
    torch nor the library."""
    if codec not in ("jpeg", "webp") or (codec == "webp" and (den != 1 or progressive or flags)):
        raise ValueError(f"{codec!r}: 'jpeg', or 'webp' without denominator, progressive files and flags")
    if progressive or flags:                                      # one entry point for every combination
        return "ffhip_jpeg_decode_files_tensor_ex"
    if oriented:
        return f"ffhip_{codec}_decode_files_tensor_oriented"
    if den != 1:
        return "ffhip_jpeg_decode_files_tensor_scaled"
    return f"ffhip_{codec}_decode_files_tensor" + ("_resized" if targets else "")


def webp_entry_point(pixels="reference", oriented=False, targets=False):
    """The C entry a WebP files-to-tensors call goes through under a pixel rule: 'reference' is entry_point('webp', ...); 'libwebp' has ONE
    entry for every combination, ffhip_webp_decode_files_tensor_ex (its tail: _WEBP_EX_TAIL).  Anything else is a ValueError."""
    return "ffhip_webp_decode_files_tensor_ex" if ops.webp_pixel_flags(pixels) else entry_point("webp", oriented, 1, targets)


_WEBP_EX_TAIL = ("resize", "orient", "flags")                    # of ffhip_webp_decode_files_tensor_ex: beside the table, not in it


# what each entry takes between the rectangles and its last three arguments (geom_out / info_out, status, stream)
_ENTRY_TAILS = {
    "ffhip_jpeg_decode_files_tensor": (), "ffhip_webp_decode_files_tensor": (),
    "ffhip_jpeg_decode_files_tensor_resized": ("resize",), "ffhip_webp_decode_files_tensor_resized": ("resize",),
    "ffhip_jpeg_decode_files_tensor_scaled": ("resize", "denom"),
    "ffhip_jpeg_decode_files_tensor_oriented": ("resize", "denom", "orient"), "ffhip_webp_decode_files_tensor_oriented": ("resize", "orient"),
    "ffhip_jpeg_decode_files_tensor_ex": ("resize", "denom", "orient", "flags"),
}


def _decode_to_tensors(codec, files, *, dtype, layout, order, mean, std, roi, stack, n_threads, strict, size, antialias, apply_exif_orientation,
                       orientation, return_orientation, reduce=1, return_reduce=False, progressive=False, flags=0, pixels="reference", alpha="drop", inflate="host"):
    fmt = tensor_format(dtype, layout, order, mean, std)
    png_flags = ops.png_inflate_flags(inflate)                    # 'device': the _ex entry, which takes the alpha record or NULL
    with_alpha = _alpha_arg(alpha)[0] != "drop"                   # 'drop' goes through the entries the call took before there was the argument
    alpha_what = alpha_entry_point(codec.name, alpha, pixels) if with_alpha else None
    record = tensor_alpha(alpha, normalised=mean is not None or std is not None) if with_alpha else None
    channels = alpha_channels(alpha)
    targets = _sizes(size, len(files))                            # argument errors come before any device use
    den = _reduce(reduce, size)
    imposed = _orientations(orientation, len(files))
    oriented = bool(apply_exif_orientation) or imposed is not None
    webp_ex = codec.name == "webp" and pixels == "libwebp"        # the ninth entry: flags = FFHIP_WEBP_PIXELS_LIBWEBP
    one_entry = webp_ex or codec.name in ("png", "vp8l")          # PNG and lossless WebP have ONE entry each, with the ninth's tail and flags = 0
    what = (f"ffhip_{codec.name}_decode_files_tensor" if codec.name in ("png", "vp8l") else webp_entry_point(pixels, oriented, bool(targets)) if webp_ex
            else entry_point(codec.name, oriented, den, bool(targets), progressive, flags))
    what = "ffhip_png_decode_files_tensor_ex" if png_flags else alpha_what or what
    probe = codec.probe_progressive if progressive else codec.probe
    import torch
    tdtype = getattr(torch, _dtype_name(dtype))
    dev = torch.cuda.current_device()
    L = capi.require_device(dev)
    n = len(files)
    rois = _rois(roi, n)
    sizes = []                                                    # (height, width) of each file's tensor; None: the probe refused it
    turns = [1] * n                                               # the orientation of each file's tensor; 0: the probe refused it
    for i, f in enumerate(files):
        try:
            w, h = probe(f)
        except capi.FfhipError:
            if strict or stack:
                raise
            sizes.append(None)
            turns[i] = 0
            continue
        if oriented:                                              # sizes and rectangles are the upright picture's
            turns[i] = imposed[i] if imposed else codec.tag(f)
        swap = turns[i] >= 5
        if targets or den == 1:
            sizes.append(targets[i] if targets else (rois[i][3], rois[i][2]) if rois else (w, h) if swap else (h, w))
            continue
        try:                                                      # without a target the tensor has the mapped rectangle's size
            stored = (0, 0, w, h) if not rois else ops.orient_rect(w, h, turns[i], rois[i]) if oriented else rois[i]
            _, _, mw, mh = ops.jpeg_scaled_rect(w, h, den, stored)
        except capi.FfhipError:
            if strict or stack:
                raise
            mw, mh, swap = rois[i][2], rois[i][3], False          # a rectangle the library refuses: its code comes from the call
        sizes.append((mw, mh) if swap else (mh, mw))
    shape = (lambda h, w: (channels, h, w)) if layout == "CHW" else (lambda h, w: (h, w, channels))
    device = torch.device("cuda", dev)
    if stack:
        if len(set(sizes)) > 1:
            raise ValueError(f"stack=True needs pictures of one size, got {sorted(set(sizes))}")
        batch = torch.empty((n,) + (shape(*sizes[0]) if n else shape(0, 0)), dtype=tdtype, device=device)
        tensors = [batch[i] for i in range(n)]
    else:
        tensors = [None if s is None or min(s) < 1 else torch.empty(shape(*s), dtype=tdtype, device=device) for s in sizes]
    ints = C.c_int * max(n, 1)
    outs = (capi.TensorOut * max(n, 1))(*[capi.TensorOut() if t is None else tensor_out(t, layout, channels) for t in tensors])
    rects = (capi.Rect * max(n, 1))(*[capi.Rect(*r) for r in rois]) if rois else None
    bufs, ptrs, lens = ops.file_args(files)
    status, used, used_turn = ints(), ints(*([1] * max(n, 1))), ints()
    tails = {                                                     # orientation 1 where none is asked for
        "resize": ((capi.Size * max(n, 1))(*[capi.Size(w, h) for h, w in targets]) if targets else None, _filter(antialias)),
        "denom": (ints(*([den] * max(n, 1))), used),
        "orient": (ints(*[(max(t, 1) if imposed else 0) if oriented else 1 for t in turns]), used_turn),
        "flags": (capi.FFHIP_WEBP_PIXELS_LIBWEBP if webp_ex else flags | (capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE if progressive else 0),),
    }
    tail = sum((tails[part] for part in (_WEBP_EX_TAIL if one_entry or with_alpha or png_flags else _ENTRY_TAILS[what])), ())
    if with_alpha or png_flags:                                   # the _alpha entries: the ninth's tail, then the record
        tail += (C.byref(record) if with_alpha else None,)
    if png_flags:
        tail += (png_flags,)
    rc = getattr(L, what)(ptrs, lens, n, n_threads, C.byref(fmt), outs, rects, *tail, None, status, torch.cuda.current_stream().cuda_stream)
    if oriented:
        turns = list(used_turn)[:n]
    status = list(status)[:n]
    if strict or stack or (rc != 0 and rc not in status):         # a file's code, or the call's own failure
        capi.check(rc, what)
    if stack:
        result = batch
    else:
        tensors = [None if status[i] else tensors[i] for i in range(n)]
        result = tensors if strict else (tensors, status)
    extras = ([list(used)[:n]] if return_reduce else []) + ([turns] if return_orientation else [])
    return (result, *extras) if extras else result


def _jpeg_size(f):
    _, w, h = ops.jpeg_probe(f)
    return w, h


def _jpeg_size_any(f):
    _, w, h, _ = ops.jpeg_probe_any(f)
    return w, h


def _webp_size(f):
    w, h, c, r = ops.webp_probe(f)
    return min(w, 16 * c), min(h, 16 * r)


# a codec as _decode_to_tensors sees it: its name in the entry points, file -> (width, height) of the display picture, the same for a
# call that accepts progressive files (None: the codec has none), file -> its EXIF orientation
_Codec = namedtuple("_Codec", "name probe probe_progressive tag")
_JPEG = _Codec("jpeg", _jpeg_size, _jpeg_size_any, ops.jpeg_exif_orientation)
_WEBP = _Codec("webp", _webp_size, None, ops.webp_exif_orientation)
_WEBP_LIBWEBP = _Codec("webp", lambda f: ops.webp_probe(f, "libwebp")[:2], None, ops.webp_exif_orientation)


def _png_size(f):
    info = ops.png_probe(f)
    return info.width, info.height


_PNG = _Codec("png", _png_size, None, ops.png_exif_orientation)


_VP8L = _Codec("vp8l", lambda f: ops.vp8l_probe(f)[:2], None, ops.webp_exif_orientation)


def decode_jpeg_to_tensors(files, dtype=None, layout="CHW", order="RGB", mean=None, std=None, roi=None, stack=False, n_threads=8,
                           strict=True, size=None, antialias=True, reduce=1, return_reduce=False, apply_exif_orientation=False, orientation=None,
                           return_orientation=False, progressive=False, pixels="reference"):
    """ffhip_jpeg_decode_files_tensor: baseline JPEG files (list of bytes) of any geometry in one call -> torch tensors on the current
    device, written on torch's current stream (the call synchronises it).
      dtype    torch.uint8 (None), torch.float16 or torch.float32;  layout 'CHW' / 'HWC';  order 'RGB' / 'BGR'
      mean/std per channel on a 0..1 scale: out = byte * float32(1 / (255 std)) + float32(-mean / std); with neither, the byte value
      roi      None: each file's display size; (x0, y0, width, height) for all files, or a list of one per file
      stack    one [N,3,H,W] / [N,H,W,3] tensor, the files' outputs slices of it; ValueError when the sizes differ, and every file
               has to decode
      size     None: every tensor has its file's (or roi's) size.  (H, W) for all files, or a list of one per file: each picture (its
               roi) is resized on the device to that size (ffhip_jpeg_decode_files_tensor_resized; the library's integer rule), so
               that stack=True takes files of different sizes
      antialias  with size: True widens the filter with the shrink factor (as PIL, torch antialias=True); False: two taps per axis
      reduce   1: the pictures are reconstructed at full size.  2, 4, 8: at 1/2, 1/4, 1/8 size straight from the coefficients
               (ffhip_jpeg_decode_files_tensor_scaled; as libjpeg's scale_num / 8, PIL's draft()): roi stays in full-size coordinates and
               is mapped (ops.jpeg_scaled_rect: its edges may move out by up to reduce - 1 source pixels); without size the tensor has
               the mapped rectangle's size.  'auto' (needs size): per file the largest of 8, 4, 2, 1 at which its rectangle still
               covers size (ops.jpeg_scale_choose), the resize doing the rest
      return_reduce  also return the denominator each file was decoded at
      apply_exif_orientation  True: every picture is delivered UPRIGHT, as its EXIF orientation tag says (ops.jpeg_exif_orientation; what
               torchvision's argument of this name and PIL's ImageOps.exif_transpose do), by ffhip_jpeg_decode_files_tensor_oriented: the
               tensors have the upright shape (a stored 4000 x 3000 of orientation 6 or 8 is 3000 wide and 4000 high), roi and size are
               in upright coordinates, and stack=True with size takes landscape and portrait files together.  False: the stored picture
      orientation  None, or an EXIF orientation 1..8 for all files or a list of one per file: applied whatever the files say (and
               whatever apply_exif_orientation says)
      return_orientation  also return the orientation each file was delivered at (0: the probe refused the file)
      progressive  False: a progressive file is refused, as ever.  True: progressive files are decoded too
               (ffhip_jpeg_decode_files_tensor_ex with FFHIP_JPEG_ACCEPT_PROGRESSIVE; sizes from ops.jpeg_probe_any) and give what their
               baseline twins give; with reduce, the scans behind the coefficients the reduced picture reads are never decoded
      pixels   'reference': the reference decoder's pixels, as ever.  'libjpeg': what libjpeg -- PIL, torchvision, DALI -- makes of the
               same file, bit for bit (ffhip_jpeg_decode_files_tensor_ex with FFHIP_JPEG_PIXELS_LIBJPEG: islow inverse DCT, fancy
               upsampling, the JFIF matrix); reduce must be 1.  Anything else: ValueError
    Returns the list of tensors; with strict=False a failing file does not raise: its entry is None, and the per-file status codes
    follow as a second element.  With return_reduce and / or return_orientation: (that, [denominators], [orientations])."""
    if pixels not in ("reference", "libjpeg"):
        raise ValueError(f"pixels {pixels!r}: 'reference' or 'libjpeg'")
    if pixels == "libjpeg" and reduce != 1:
        raise ValueError("pixels='libjpeg' needs reduce=1: libjpeg's reduced-size transforms are another rule")
    return _decode_to_tensors(_JPEG, files, dtype=dtype, layout=layout, order=order, mean=mean, std=std, roi=roi, stack=stack, n_threads=n_threads,
                              strict=strict, size=size, antialias=antialias, apply_exif_orientation=apply_exif_orientation, orientation=orientation,
                              return_orientation=return_orientation, reduce=reduce, return_reduce=return_reduce, progressive=bool(progressive),
                              flags=capi.FFHIP_JPEG_PIXELS_LIBJPEG if pixels == "libjpeg" else 0)


def decode_webp_to_tensors(files, dtype=None, layout="CHW", order="RGB", mean=None, std=None, roi=None, stack=False, n_threads=8,
                           strict=True, size=None, antialias=True, apply_exif_orientation=False, orientation=None, return_orientation=False,
                           pixels="reference", alpha="drop"):
    """ffhip_webp_decode_files_tensor (with size: ffhip_webp_decode_files_tensor_resized; with apply_exif_orientation or orientation:
    ffhip_webp_decode_files_tensor_oriented, the tag read from the file's EXIF chunk): lossy WebP files; arguments and result as
    decode_jpeg_to_tensors.  A file's display size is the
    probe's width x height as far as the decoded picture holds it.
      pixels   'reference': the reference decoder's pixels, as ever.  'libwebp': what libwebp -- PIL, torchvision, a browser -- makes of the
               same file, sample for sample (ffhip_webp_decode_files_tensor_ex with FFHIP_WEBP_PIXELS_LIBWEBP): the picture is the frame
               tag's width x height, and roi, size and orientation act on it.  Anything else: ValueError
      alpha    as decode_png_to_tensors: the ALPH plane of a file that has one (ffhip_webp_decode_files_tensor_alpha, FFHIP_WEBP_ALPHA
               underneath), 255 for every other file.  Only with pixels='libwebp': the reference rule decodes no alpha (ValueError)"""
    ops.webp_pixel_flags(pixels)
    alpha_entry_point("webp", alpha, pixels)
    return _decode_to_tensors(_WEBP_LIBWEBP if pixels == "libwebp" else _WEBP, files, pixels=pixels, dtype=dtype, layout=layout, order=order, mean=mean, std=std, roi=roi, stack=stack, n_threads=n_threads,
                              strict=strict, size=size, antialias=antialias, apply_exif_orientation=apply_exif_orientation, orientation=orientation,
                              return_orientation=return_orientation, alpha=alpha)


def decode_png_to_tensors(files, dtype=None, layout="CHW", order="RGB", mean=None, std=None, roi=None, stack=False, n_threads=8,
                          strict=True, size=None, antialias=True, apply_exif_orientation=False, orientation=None, return_orientation=False,
                          alpha="drop", inflate="host"):
    """ffhip_png_decode_files_tensor: PNG files of every colour type and bit depth, interlaced or not; arguments and result as
    decode_webp_to_tensors (the orientation tag is read from the file's eXIf chunk).  A file's display size is its width x height.
      alpha    'drop': three channels, alpha is dropped as PIL's convert("RGB") drops it -- the colour stored under transparent pixels
               shows.  'straight': four channels R,G,B,A ([N,4,H,W] with stack=True), the colour as stored.  'premultiplied': four
               channels, the colour times alpha / 255 (PIL's convert("RGBa")).  ('over', (r, g, b)): three channels, the picture
               composited over that background colour (Image.alpha_composite).  With size the resize filters premultiplied samples, so
               the colour under transparent pixels never bleeds into the edges; 'straight' un-premultiplies behind it.  Integers only
               (include/ffpic_hip.h, "alpha into the tensors").  The alpha channel of a float tensor is alpha * float32(1 / 255) when
               mean or std is given, the byte value otherwise (ffhip_png_decode_files_tensor_alpha).  Anything else: ValueError
      inflate  'host' (the default): the host threads inflate.  'device': k_inflate does, a wave per file
               (ffhip_png_decode_files_tensor_ex with FFHIP_PNG_INFLATE_DEVICE); the tensors are the same bit for bit"""
    return _decode_to_tensors(_PNG, files, alpha=alpha, inflate=inflate, dtype=dtype, layout=layout, order=order, mean=mean, std=std, roi=roi, stack=stack, n_threads=n_threads,
                              strict=strict, size=size, antialias=antialias, apply_exif_orientation=apply_exif_orientation, orientation=orientation,
                              return_orientation=return_orientation)


def decode_webp_lossless_to_tensors(files, dtype=None, layout="CHW", order="RGB", mean=None, std=None, roi=None, stack=False, n_threads=8,
                                    strict=True, size=None, antialias=True, apply_exif_orientation=False, orientation=None, return_orientation=False,
                                    alpha="drop"):
    """ffhip_vp8l_decode_files_tensor: lossless WebP (VP8L) files, the pixels libwebp gives; arguments and result as decode_png_to_tensors
    (the orientation tag is read from the file's EXIF chunk; alpha= through ffhip_vp8l_decode_files_tensor_alpha, a file whose
    alpha_is_used bit is clear delivering alpha 255).  A file's display size is its header's width x height."""
    return _decode_to_tensors(_VP8L, files, alpha=alpha, dtype=dtype, layout=layout, order=order, mean=mean, std=std, roi=roi, stack=stack, n_threads=n_threads,
                              strict=strict, size=size, antialias=antialias, apply_exif_orientation=apply_exif_orientation, orientation=orientation,
                              return_orientation=return_orientation)


def _per_picture(value, n, name, error=None):
    """one value or one per picture -> the list of n"""
    values = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(values) != n:
        raise ValueError(error or f"{name}: {len(values)} values for {n} pictures")
    return values


def _picture_list(pictures):
    """one tensor or several -> (single, the list)"""
    import torch
    single = isinstance(pictures, torch.Tensor)
    return single, [pictures] if single else list(pictures)


def _encode_files(single, caps, item_of, call, nospace, entry, to_host):
    """What the encoders share behind their argument checks: picture i's file goes into caps[i] bytes of ONE buffer on the current device,
    item_of(i, d_out, cap) is its item, call(items, stream, strict=False) -> (lens, status) the ops entry named `entry`.  The files whose
    status is `nospace` go through a second call at the length the first one reported; any other status raises.  -> the files as views of
    the buffers, or as bytes with to_host; with `single` the one file."""
    import torch
    n = len(caps)
    if n == 0:
        return []
    dev = torch.cuda.current_device()
    capi.require_device(dev)
    device = torch.device("cuda", dev)
    stream = torch.cuda.current_stream().cuda_stream
    files, todo, caps = [None] * n, list(range(n)), list(caps)
    for _ in range(2):
        offs = np.concatenate([[0], np.cumsum([caps[i] for i in todo])]).astype(np.int64)
        buf = torch.empty(int(offs[-1]), dtype=torch.uint8, device=device)
        lens, status = call([item_of(i, buf.data_ptr() + int(offs[k]), caps[i]) for k, i in enumerate(todo)], stream, strict=False)
        again = []
        for k, i in enumerate(todo):
            if status[k] == 0:
                files[i] = buf[int(offs[k]):int(offs[k]) + lens[k]]
            elif status[k] == nospace:
                caps[i] = (lens[k] + 255) & ~255
                again.append(i)
            else:
                capi.check(status[k], entry)
        todo = again
        if not todo:
            break
    if to_host:
        files = [bytes(f.cpu().numpy()) for f in files]
    return files[0] if single else files


def jpeg_source_of(t):
    """capi.JpegSource of a uint8 device tensor [3,H,W], [1,H,W] or [H,W,3], whatever its strides -> (source, grey).  A first dimension of 3
    or 1 is ALWAYS read as channels first, as torchvision's encode_jpeg reads it: an [H,W,3] picture that is 1 or 3 rows high has to be passed
    as t.permute(2, 0, 1)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 3:
        raise ValueError("encode_jpeg takes uint8 device tensors [3,H,W], [1,H,W] or [H,W,3]")
    if t.shape[0] in (1, 3):
        c, (height, width), (plane, row, pixel) = t.shape[0], t.shape[1:], t.stride()
    elif t.shape[2] == 3:
        c, (height, width), (row, pixel, plane) = 3, t.shape[:2], t.stride()
    else:
        raise ValueError(f"encode_jpeg takes [3,H,W], [1,H,W] or [H,W,3], got {tuple(t.shape)}")
    if width < 1 or height < 1:
        raise ValueError(f"encode_jpeg: an empty picture {tuple(t.shape)}")
    return capi.jpeg_source(t.data_ptr(), width, height, row, pixel, tuple(k * plane for k in range(c)), c), c == 1


def encode_jpeg(pictures, quality=75, subsampling="4:2:0", restart_blocks=0, to_host=False):
    """Device pictures to baseline JPEG files, byte for byte what libjpeg (PIL, torchvision) writes at this quality: a list of uint8 device
    tensors [3,H,W] (R, G, B), [1,H,W] (grey) or [H,W,3] (a first dimension of 3 or 1 is always channels: pass an [H,W,3] picture 1 or 3 rows high as t.permute(2, 0, 1)), of any sizes and strides, in ONE ffhip_jpeg_encode_items call on the current stream
    -> a list of 1-D uint8 device tensors (views of one allocation), or of bytes with to_host=True.  quality, subsampling ('4:4:4', '4:2:2',
    '4:2:0'; a grey picture is written as one component) and restart_blocks (MCUs per restart interval, 0: none) are one value or one per
    picture.  The outputs start at half the pixels' size; the files that need more (the call says how much) go through a second call."""
    single, pictures = _picture_list(pictures)
    n = len(pictures)
    qualities, layouts = _per_picture(quality, n, "quality"), _per_picture(subsampling, n, "subsampling")
    restarts = [int(r) for r in _per_picture(restart_blocks, n, "restart_blocks")]
    sources = [jpeg_source_of(t) for t in pictures]                       # argument errors come before any device use
    layouts = [capi.FFHIP_JPEG_ENC_GREY if grey else ops.jpeg_encode_layout(l) for (_, grey), l in zip(sources, layouts)]
    for (_, grey), l in zip(sources, layouts):
        if not grey and l == capi.FFHIP_JPEG_ENC_GREY:
            raise ValueError("subsampling 'grey' needs a [1,H,W] picture")
    caps = [((1024 + s.width * s.height * s.channels // 2) + 255) & ~255 for s, _ in sources]

    def item_of(i, d_out, cap):
        it = capi.JpegEncodeItem()
        it.src, it.layout, it.quality, it.restart = sources[i][0], layouts[i], int(qualities[i]), restarts[i]
        it.d_out, it.cap = d_out, cap
        return it
    return _encode_files(single, caps, item_of, ops.jpeg_encode_items, capi.FFHIP_EJPEG_NOSPACE, "ffhip_jpeg_encode_items", to_host)


def png_source_of(t):
    """capi.PngSource of a uint8 device tensor [C,H,W] or [H,W,C] with C in 1..4 (grey, grey + alpha, RGB, RGBA), whatever its strides.  A
    first dimension of 1..4 is ALWAYS read as channels first, jpeg_source_of's convention: an [H,W,C] picture up to 4 rows high has to be
    passed as t.permute(2, 0, 1)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 3:
        raise ValueError("encode_png takes uint8 device tensors [C,H,W] or [H,W,C] with C in 1..4")
    if 1 <= t.shape[0] <= 4:
        c, (height, width), (plane, row, pixel) = t.shape[0], t.shape[1:], t.stride()
    elif 1 <= t.shape[2] <= 4:
        c, (height, width), (row, pixel, plane) = t.shape[2], t.shape[:2], t.stride()
    else:
        raise ValueError(f"encode_png takes [C,H,W] or [H,W,C] with C in 1..4, got {tuple(t.shape)}")
    if width < 1 or height < 1 or width > 65535 or height > 65535:
        raise ValueError(f"encode_png: sides of 1..65535, got {tuple(t.shape)}")
    return capi.png_source(t.data_ptr(), width, height, row, pixel, tuple(k * plane for k in range(c)))


def encode_png(pictures, filter="adaptive", to_host=False):
    """Device pictures to PNG files, lossless: a list of uint8 device tensors [C,H,W] or [H,W,C] with C in 1..4 (colour type grey, grey +
    alpha, RGB, RGBA; a first dimension of 1..4 is always channels), of any sizes and strides, in ONE ffhip_png_encode_items call on the
    current stream -> a list of 1-D uint8 device tensors (views of one allocation), or of bytes with to_host=True.  filter: 'adaptive' (per
    row the type with the smallest sum of absolute values), 'none', 'sub', 'up', 'average', 'paeth' or 0..5, one value or one per picture.
    The outputs start at half the bound; the files that need more (the call says how much) go through a second call."""
    single, pictures = _picture_list(pictures)
    filters = [ops.png_filter_id(f) for f in _per_picture(filter, len(pictures), "filter")]   # argument errors come before any device use
    sources = [png_source_of(t) for t in pictures]
    caps = [(ops.png_encode_bound(s.width, s.height, s.channels) // 2 + 255) & ~255 for s in sources]

    def item_of(i, d_out, cap):
        it = capi.PngEncodeItem()
        it.src, it.filter, it.d_out, it.cap = sources[i], filters[i], d_out, cap
        return it
    return _encode_files(single, caps, item_of, ops.png_encode_items, capi.FFHIP_EPNG_NOSPACE, "ffhip_png_encode_items", to_host)


def encode_webp_lossless(pictures, predict=True, subtract_green=True, to_host=False):
    """Device pictures to lossless WebP files: a list of uint8 device tensors as encode_png takes them ([C,H,W] or [H,W,C] with C in 1..4:
    grey, grey + alpha, RGB, RGBA; sides up to 16384), of any sizes and strides, in ONE ffhip_vp8l_encode_items call on the current stream
    -> a list of 1-D uint8 device tensors (views of one allocation), or of bytes with to_host=True.  predict, subtract_green: the two
    transforms, one value or one per picture.  The outputs start at half the bound; the files that need more (the call says how much) go
    through a second call."""
    single, pictures = _picture_list(pictures)
    flags = []
    for name, value in (("predict", predict), ("subtract_green", subtract_green)):
        error = f"{name}: True or False, one value or one per picture"
        values = _per_picture(value, len(pictures), name, error)
        if not all(isinstance(v, (bool, np.bool_)) for v in values):
            raise ValueError(error)
        flags.append(values)
    flags = [ops.vp8l_encode_flags(p, g) for p, g in zip(*flags)]            # argument errors come before any device use
    sources = [png_source_of(t) for t in pictures]
    for s in sources:
        if s.width > 16384 or s.height > 16384:
            raise ValueError(f"encode_webp_lossless: sides of 1..16384, got {s.width} x {s.height}")
    caps = [(ops.vp8l_encode_bound(s.width, s.height) // 2 + 255) & ~255 for s in sources]

    def item_of(i, d_out, cap):
        it = capi.Vp8lEncodeItem()
        it.src, it.flags, it.d_out, it.cap = sources[i], flags[i], d_out, cap
        return it
    return _encode_files(single, caps, item_of, ops.vp8l_encode_items, capi.FFHIP_EVP8L_NOSPACE, "ffhip_vp8l_encode_items", to_host)


def encode_webp(pictures, quality=75, filter=None, to_host=False):
    """Device pictures to lossy WebP files (one VP8 key frame each, the rule of include/ffpic_hip.h "Lossy WebP encoding"): a list of uint8
    device tensors as encode_jpeg takes them ([3,H,W], [1,H,W] or [H,W,3]; sides up to 16383), of any sizes and strides, in ONE
    ffhip_vp8_encode_items call on the current stream -> a list of 1-D uint8 device tensors (views of one allocation), or of bytes with
    to_host=True.  quality 0..100 and filter (the loop filter level 0..63, None for the rule's own) are one value or one per picture.  The
    outputs start at half the pixels' bytes; the files that need more (the call says how much) go through a second call."""
    single, pictures = _picture_list(pictures)
    n = len(pictures)
    qualities = _per_picture(quality, n, "quality")
    filters = [-1 if f is None else f for f in _per_picture(filter, n, "filter")]
    for q, f in zip(qualities, filters):                                   # argument errors come before any device use
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= q <= 100:
            raise ValueError(f"quality: integers 0..100, got {q!r}")
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not -1 <= f <= 63:
            raise ValueError(f"filter: None or integers 0..63, got {f!r}")
    sources = [jpeg_source_of(t)[0] for t in pictures]
    for s in sources:
        if s.width > 16383 or s.height > 16383:
            raise ValueError(f"encode_webp: sides of 1..16383, got {s.width} x {s.height}")
    caps = [(s.width * s.height * s.channels // 2 + 255) & ~255 for s in sources]

    def item_of(i, d_out, cap):
        it = capi.Vp8EncodeItem()
        it.src, it.quality, it.filter, it.d_out, it.cap = sources[i], int(qualities[i]), int(filters[i]), d_out, cap
        return it
    return _encode_files(single, caps, item_of, ops.vp8_encode_items, capi.FFHIP_EVP8_NOSPACE, "ffhip_vp8_encode_items", to_host)
