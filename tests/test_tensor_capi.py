"""CPU: the tensor sink's C interface (ffhip_bgra_to_tensor_items, ffhip_jpeg_decode_files_tensor, ffhip_webp_decode_files_tensor) --
struct layouts against the header, every refusal before the device is asked for, the part-budget switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ffpic_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def fmt(dtype=capi.FFHIP_TENSOR_U8, bgr=0, planar=1, scale=(1, 1, 1), bias=(0, 0, 0)):
    f = capi.TensorFormat()
    f.dtype, f.bgr, f.planar = dtype, bgr, planar
    for c in range(3):
        f.scale[c], f.bias[c] = scale[c], bias[c]
    return f


def item(**kw):
    """a good item for every format: a 20 x 10 rectangle at (2, 3) of a picture with pitch 128, planar strides that fit HWC too"""
    it = capi.TensorItem()
    it.d_bgra, it.pitch, it.x0, it.y0, it.width, it.height = 0x10000, 128, 2, 3, 20, 10
    it.d_out, it.row_stride, it.plane_stride = 0x20004, 64, 64 * 9 + 20
    for k, v in kw.items():
        setattr(it, k, v)
    return it


def call(L, items, f, n=None):
    arr = (capi.TensorItem * max(len(items), 1))(*items)
    return L.ffhip_bgra_to_tensor_items(arr, len(items) if n is None else n, C.byref(f) if f is not None else None, None)


def test_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    for name in ("FFHIP_TENSOR_U8 0", "FFHIP_TENSOR_F16 1", "FFHIP_TENSOR_F32 2"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name
    assert (capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16, capi.FFHIP_TENSOR_F32) == (0, 1, 2)
    F, I, O, R = capi.TensorFormat, capi.TensorItem, capi.TensorOut, capi.Rect
    assert C.sizeof(F) == 36 and (F.dtype.offset, F.bgr.offset, F.planar.offset, F.scale.offset, F.bias.offset) == (0, 4, 8, 12, 24)
    assert C.sizeof(I) == 56
    assert (I.d_bgra.offset, I.pitch.offset, I.x0.offset, I.y0.offset, I.width.offset, I.height.offset) == (0, 8, 16, 20, 24, 28)
    assert (I.d_out.offset, I.row_stride.offset, I.plane_stride.offset) == (32, 40, 48)
    assert C.sizeof(O) == 24 and (O.d_out.offset, O.row_stride.offset, O.plane_stride.offset) == (0, 8, 16)
    assert C.sizeof(R) == 16 and (R.x0.offset, R.y0.offset, R.width.offset, R.height.offset) == (0, 4, 8, 12)
    # the header's field order is the binding's
    for struct, fields in (("ffhip_tensor_format", ["dtype", "bgr", "planar", "scale", "bias"]),
                           ("ffhip_tensor_item", ["d_bgra", "pitch", "x0", "height", "d_out", "row_stride", "plane_stride"]),
                           ("ffhip_tensor_out", ["d_out", "row_stride", "plane_stride"]), ("ffhip_rect", ["x0", "y0", "width", "height"])):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        at = [body.index(f) for f in fields]
        assert at == sorted(at), struct


def test_no_items_is_ok_and_bad_counts_are_refused(L):
    assert call(L, [], fmt()) == 0
    assert L.ffhip_bgra_to_tensor_items(None, 0, C.byref(fmt()), None) == 0
    assert call(L, [], fmt(), n=-1) == EINVAL
    assert L.ffhip_bgra_to_tensor_items(None, 1, C.byref(fmt()), None) == EINVAL
    assert call(L, [item()], None) == EINVAL


BAD_FORMATS = {
    "dtype 3": dict(dtype=3), "dtype -1": dict(dtype=-1),
    "u8 scale": dict(scale=(1, 0.5, 1)), "u8 bias": dict(bias=(0, 0, 1)),
    "nan scale": dict(dtype=capi.FFHIP_TENSOR_F32, scale=(1, float("nan"), 1)), "inf scale": dict(dtype=capi.FFHIP_TENSOR_F16, scale=(float("inf"), 1, 1)),
    "nan bias": dict(dtype=capi.FFHIP_TENSOR_F16, bias=(0, 0, float("nan"))), "inf bias": dict(dtype=capi.FFHIP_TENSOR_F32, bias=(float("-inf"), 0, 0)),
}


@pytest.mark.parametrize("name", list(BAD_FORMATS))
def test_bad_formats_are_refused(L, name):
    assert call(L, [item()], fmt(**BAD_FORMATS[name])) == EINVAL
    assert call(L, [], fmt(**BAD_FORMATS[name])) == EINVAL       # with nothing to do as well


U8, F16, F32 = capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16, capi.FFHIP_TENSOR_F32
BAD_ITEMS = {
    "width 0": (dict(width=0), U8, 1), "height 0": (dict(height=0), U8, 1), "width -1": (dict(width=-1), F32, 0),
    "x0 -1": (dict(x0=-1), U8, 1), "y0 -1": (dict(y0=-1), U8, 0),
    "no picture": (dict(d_bgra=None), U8, 1), "picture at 2": (dict(d_bgra=0x10002), U8, 1), "pitch % 4": (dict(pitch=130), U8, 1),
    "pitch 0": (dict(pitch=0), U8, 1), "rectangle wider than the pitch": (dict(pitch=84), U8, 1),
    "no output": (dict(d_out=None), U8, 1), "f16 output at 1": (dict(d_out=0x20001), F16, 1), "f32 output at 2": (dict(d_out=0x20002), F32, 0),
    "chw row stride": (dict(row_stride=19), U8, 1), "hwc row stride": (dict(row_stride=59), F16, 0), "negative row stride": (dict(row_stride=-64), U8, 1),
    "plane stride": (dict(plane_stride=64 * 9 + 19), F32, 1), "negative plane stride": (dict(plane_stride=-1000), U8, 1),
    "rows past 31 bits": (dict(pitch=1 << 20, y0=2040, height=9), U8, 1), "y0 past 31 bits": (dict(pitch=1 << 20, y0=0x7fffffff), U8, 1),
    "x0 past 31 bits": (dict(pitch=1 << 40, x0=0x7ffffff0), U8, 1),
}


@pytest.mark.parametrize("name", list(BAD_ITEMS))
def test_bad_items_are_refused_before_the_device_is_asked_for(L, name):
    kw, dtype, planar = BAD_ITEMS[name]
    for items in ([item(**kw)], [item(), item(), item(**kw)]):
        assert call(L, items, fmt(dtype=dtype, planar=planar)) == EINVAL, name


def test_limits_are_inclusive(L):
    """what the refusals above leave: the smallest strides, a one-element alignment, the last source offset of 31 bits"""
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present: these addresses are not memory; the -m gpu tests run the call")
    good = [
        (item(row_stride=20, plane_stride=20 * 9 + 20), U8, 1), (item(row_stride=60), U8, 0), (item(d_out=0x20001), U8, 0),
        (item(d_out=0x20002), F16, 1), (item(d_out=0x20004), F32, 0), (item(pitch=88), U8, 1),
        (item(pitch=1 << 20, y0=2037, height=10), F32, 1),                     # (y0 + height) pitch = 2^31 - 2^20
    ]
    for it, dtype, planar in good:
        for bgr in (0, 1):
            assert call(L, [it], fmt(dtype=dtype, planar=planar, bgr=bgr)) == ENODEV
    f = fmt(dtype=F32, scale=(1 / 255, 0.5, 2), bias=(-1, 0, 1))
    assert call(L, [item(), item(width=1, height=1)], f) == ENODEV


def test_part_budget_switch_is_read_through_the_switch_table(L):
    buf = C.create_string_buffer(64)
    capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    assert L.ffhip_env_value_test(b"FFHIP_TENSOR_PART_BYTES", buf, 64) == -1
    capi.setenv("FFHIP_TENSOR_PART_BYTES", 65536)
    try:
        assert L.ffhip_env_value_test(b"FFHIP_TENSOR_PART_BYTES", buf, 64) == 5 and buf.value == b"65536"
    finally:
        capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    assert L.ffhip_env_value_test(b"FFHIP_TENSOR_PART_BYTES", buf, 64) == -1


@pytest.mark.parametrize("entry", ["ffhip_jpeg_decode_files_tensor", "ffhip_webp_decode_files_tensor"])
def test_file_calls_refuse_missing_arguments(L, entry):
    call_ = getattr(L, entry)
    data = np.frombuffer(b"\xff\xd8 not a picture", dtype=np.uint8)
    files, lens = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(data.size)
    outs, status, f = (capi.TensorOut * 1)(), (C.c_int * 1)(), fmt()
    assert call_(files, lens, 0, 2, C.byref(f), outs, None, None, status, None) == 0
    assert call_(None, None, 0, 2, C.byref(f), None, None, None, None, None) == 0
    assert call_(files, lens, -1, 2, C.byref(f), outs, None, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, None, outs, None, None, status, None) == EINVAL            # no format
    assert call_(files, lens, 1, 2, C.byref(f), None, None, None, status, None) == EINVAL      # no outputs
    assert call_(None, lens, 1, 2, C.byref(f), outs, None, None, status, None) == EINVAL
    assert call_(files, None, 1, 2, C.byref(f), outs, None, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(f), outs, None, None, None, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(fmt(dtype=7)), outs, None, None, status, None) == EINVAL
    assert call_(files, lens, 0, 2, C.byref(fmt(scale=(2, 1, 1))), outs, None, None, status, None) == EINVAL
    if L.ffhip_device_count() == 0:   # good arguments: the file is looked at (and found wanting), then the device is missed
        assert call_(files, lens, 1, 2, C.byref(f), outs, None, None, status, None) == ENODEV
        assert status[0] != 0


def test_the_body_on_the_cpu_at_every_alignment(tmp_path):
    """tests/tools/check_tensor_body.cpp: the kernel's body, lane by lane on the host, against a plain loop with guard bytes around"""
    import subprocess
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))), "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "clang++"
    exe = str(tmp_path / "check_tensor_body")
    subprocess.check_call([clang, "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + capi.CSRC,
                           os.path.join(ROOT, "tests", "tools", "check_tensor_body.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "43200 cases, 0 bad" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


def test_python_format_rounds_once():
    from ffpic_amd import tensors
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    f = tensors.tensor_format("float32", "HWC", "BGR", mean, std)
    assert (f.dtype, f.bgr, f.planar) == (F32, 1, 0)
    for c in range(3):
        assert np.float32(f.scale[c]) == np.float32(1.0 / (255.0 * std[c])) and np.float32(f.bias[c]) == np.float32(-mean[c] / std[c])
    f = tensors.tensor_format(np.float16)
    assert (f.dtype, f.bgr, f.planar, list(f.scale), list(f.bias)) == (F16, 0, 1, [1.0] * 3, [0.0] * 3)
    with pytest.raises(ValueError):
        tensors.tensor_format("uint8", mean=mean, std=std)
    with pytest.raises(ValueError):
        tensors.tensor_format("int32")


def _entry_cases():
    """every call the two public functions can make: WebP has neither a denominator nor progressive files nor flags"""
    import itertools
    for codec, oriented, den, targets, progressive, flags in itertools.product(("jpeg", "webp"), (False, True), (1, 2, 0), (False, True), (False, True),
                                                                               (0, capi.FFHIP_JPEG_PIXELS_LIBJPEG)):
        if codec == "jpeg" or (den == 1 and not progressive and not flags):
            yield codec, oriented, den, targets, progressive, flags


@pytest.mark.parametrize("codec,oriented,den,targets,progressive,flags", list(_entry_cases()))
def test_entry_point_table(codec, oriented, den, targets, progressive, flags):
    from ffpic_amd import tensors
    if progressive or flags:
        want = "ffhip_jpeg_decode_files_tensor_ex"
    elif oriented:
        want = {"jpeg": "ffhip_jpeg_decode_files_tensor_oriented", "webp": "ffhip_webp_decode_files_tensor_oriented"}[codec]
    elif den != 1:
        want = "ffhip_jpeg_decode_files_tensor_scaled"
    elif targets:
        want = {"jpeg": "ffhip_jpeg_decode_files_tensor_resized", "webp": "ffhip_webp_decode_files_tensor_resized"}[codec]
    else:
        want = {"jpeg": "ffhip_jpeg_decode_files_tensor", "webp": "ffhip_webp_decode_files_tensor"}[codec]
    assert tensors.entry_point(codec, oriented, den, targets, progressive, flags) == want
    assert want in capi.EXPORTS


def test_entry_point_reaches_all_eight_entries_and_refuses_what_webp_lacks():
    from ffpic_amd import tensors
    reached = {tensors.entry_point(*case) for case in _entry_cases()}
    assert reached == set(tensors._ENTRY_TAILS) and len(reached) == 8
    for kw in (dict(den=2), dict(den=0), dict(progressive=True), dict(flags=capi.FFHIP_JPEG_PIXELS_LIBJPEG)):
        with pytest.raises(ValueError):
            tensors.entry_point("webp", **kw)
    with pytest.raises(ValueError):
        tensors.entry_point("heic")
