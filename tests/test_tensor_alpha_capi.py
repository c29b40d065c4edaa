"""CPU: alpha into the tensors (include/ffpic_hip.h).  The rule's steps, as tests/alpha_spec.py writes them, against PIL over
every pair of bytes; the struct against the header; every refusal of the new entries in front of the device check; the body of the new
kernel instances and the premultiplying resize's staging on the CPU (tests/tools/check_tensor_alpha_body.cpp, a program of its own built with
-fsanitize=address,undefined); the Python layer's argument errors and the entry each combination goes through."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_spec as S
from ffpic_amd import capi, ops, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV
U8, F16, F32 = capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16, capi.FFHIP_TENSOR_F32
DROP, STRAIGHT, PREMULTIPLIED, OVER = capi.FFHIP_ALPHA_DROP, capi.FFHIP_ALPHA_STRAIGHT, capi.FFHIP_ALPHA_PREMULTIPLIED, capi.FFHIP_ALPHA_OVER


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


# ---------------------------------------------------------------------------------------------------- the rule against PIL
C_A = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(-1, 2)     # every (c, a)


def pixels_of(c, a):
    """[n][4] B,G,R,A with the colour byte in all three channels"""
    return np.stack([c, c, c, a], -1).astype(np.uint8)


def test_div255_is_the_rounded_quotient():
    t = np.arange(65026)
    assert np.array_equal(S.div255(t), (2 * t + 255) // 510)                    # floor(t / 255 + 1/2), in integers
    assert np.array_equal(S.div255(t), np.floor(t / 255 + 0.5).astype(np.int64))


def test_premultiply_is_pils_rgba_to_premultiplied():
    Image = pytest.importorskip("PIL.Image")
    px = pixels_of(C_A[:, 0], C_A[:, 1])
    pil = np.frombuffer(Image.frombytes("RGBA", (256, 256), px.tobytes()).convert("RGBa").tobytes(), np.uint8).reshape(-1, 4)
    assert np.array_equal(S.premultiply(px), pil)


def test_unpremultiply_is_pils_premultiplied_to_rgba():
    Image = pytest.importorskip("PIL.Image")
    p, a = C_A[:, 0], C_A[:, 1]
    p = np.minimum(p, a)                                                         # every (p, a) with p <= a (some of them twice)
    px = pixels_of(p, a)
    pil = np.frombuffer(Image.frombytes("RGBa", (256, 256), px.tobytes()).convert("RGBA").tobytes(), np.uint8).reshape(-1, 4)
    got = S.unpremultiply(px)
    assert np.array_equal(got, pil)
    assert np.array_equal(got[a == 255], px[a == 255]) and not got[a == 0][:, :3].any()


@pytest.mark.parametrize("g", [0, 1, 37, 128, 200, 254, 255])
def test_over_is_pils_alpha_composite_onto_an_opaque_background(g):
    Image = pytest.importorskip("PIL.Image")
    px = pixels_of(C_A[:, 0], C_A[:, 1])
    fg = Image.frombytes("RGBA", (256, 256), px.tobytes())
    bg = Image.new("RGBA", (256, 256), (g, g, g, 255))
    pil = np.frombuffer(Image.alpha_composite(bg, fg).tobytes(), np.uint8).reshape(-1, 4)
    assert (pil[:, 3] == 255).all()
    assert np.array_equal(S.over(px, (g, g, g)), pil[:, :3])


def test_the_premultiplied_composite_needs_no_clamp():
    p, a = C_A[:, 0], C_A[:, 1]
    keep = p <= a
    for g in range(256):
        v = p[keep] + S.div255(g * (255 - a[keep]))
        assert v.max() <= 255
        assert np.array_equal(S.over(pixels_of(p[keep], a[keep]), (g, g, g), True)[:, 0], v)
    # and it is the straight composite up to the one rounding the premultiplication adds
    px = pixels_of(C_A[:, 0], C_A[:, 1])
    d = S.over(S.premultiply(px), (200, 200, 200), True).astype(int) - S.over(px, (200, 200, 200)).astype(int)
    assert np.abs(d).max() <= 1


def test_an_opaque_picture_keeps_its_colour_through_every_mode():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (7, 9, 4), dtype=np.uint8)
    px[..., 3] = 255
    rgb = px[..., 2::-1]
    for mode in S.MODES:
        for pre in (False, True):
            assert np.array_equal(S.channels(px, mode, pre, (3, 4, 5))[..., :3], rgb), (mode, pre)


# ---------------------------------------------------------------------------------------------------- the ABI
def test_struct_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    for name in ("FFHIP_ALPHA_DROP 0", "FFHIP_ALPHA_STRAIGHT 1", "FFHIP_ALPHA_PREMULTIPLIED 2", "FFHIP_ALPHA_OVER 3"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name
    assert (DROP, STRAIGHT, PREMULTIPLIED, OVER) == (0, 1, 2, 3)
    A = capi.TensorAlpha
    assert C.sizeof(A) == 20
    assert (A.mode.offset, A.source_premultiplied.offset, A.background.offset, A.alpha_scale.offset, A.alpha_bias.offset) == (0, 4, 8, 12, 16)
    body = re.search(r"typedef struct ffhip_tensor_alpha \{(.*?)\} ffhip_tensor_alpha;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    at = [body.index(f) for f in ("mode", "source_premultiplied", "background[4]", "alpha_scale", "alpha_bias")]
    assert at == sorted(at)
    for entry in ("ffhip_bgra_to_tensor_items_alpha", "ffhip_bgra_resize_items_premultiplied", "ffhip_png_decode_files_tensor_alpha",
                  "ffhip_vp8l_decode_files_tensor_alpha", "ffhip_webp_decode_files_tensor_alpha"):
        assert entry in capi.EXPORTS and re.search(r"\b" + entry + r"\(", text), entry


def fmt(dtype=U8, bgr=0, planar=1):
    f = capi.TensorFormat()
    f.dtype, f.bgr, f.planar = dtype, bgr, planar
    for c in range(3):
        f.scale[c], f.bias[c] = 1, 0
    return f


def alpha(mode=STRAIGHT, pre=0, scale=1.0, bias=0.0):
    a = capi.TensorAlpha()
    a.mode, a.source_premultiplied, a.alpha_scale, a.alpha_bias = mode, pre, scale, bias
    return a


def item(**kw):
    """a good item for every format and channel count: a 20 x 10 rectangle at (2, 3) of a picture with pitch 128"""
    it = capi.TensorItem()
    it.d_bgra, it.pitch, it.x0, it.y0, it.width, it.height = 0x10000, 128, 2, 3, 20, 10
    it.d_out, it.row_stride, it.plane_stride = 0x20004, 96, 96 * 9 + 20
    for k, v in kw.items():
        setattr(it, k, v)
    return it


def items_call(L, it, f, a):
    arr = (capi.TensorItem * 1)(it)
    return L.ffhip_bgra_to_tensor_items_alpha(arr, 1, C.byref(f), C.byref(a) if a is not None else None, None)


BAD_RECORDS = {
    "mode 4": (U8, dict(mode=4)), "mode -1": (U8, dict(mode=-1)), "source 2": (U8, dict(pre=2)),
    "u8 alpha scale": (U8, dict(scale=0.5)), "u8 alpha bias": (U8, dict(bias=1.0)),
    "nan scale": (F32, dict(scale=float("nan"))), "inf scale": (F16, dict(scale=float("inf"))),
    "nan bias": (F16, dict(bias=float("nan"))), "inf bias": (F32, dict(bias=float("-inf"))),
}


@pytest.mark.parametrize("name", list(BAD_RECORDS))
def test_bad_records_are_refused_in_front_of_the_device(L, name):
    dtype, kw = BAD_RECORDS[name]
    assert items_call(L, item(), fmt(dtype), alpha(**kw)) == EINVAL


def test_four_channel_outputs_are_checked_for_four_channels(L):
    w, h = 20, 10
    hwc, chw = fmt(planar=0), fmt(planar=1)
    assert items_call(L, item(row_stride=4 * w - 1), hwc, alpha(STRAIGHT)) == EINVAL          # a row of four channels does not fit
    assert items_call(L, item(row_stride=3 * w), hwc, alpha(PREMULTIPLIED)) == EINVAL
    assert items_call(L, item(row_stride=w, plane_stride=w * (h - 1) + w - 1), chw, alpha(STRAIGHT)) == EINVAL    # planes overlap
    assert items_call(L, item(row_stride=3 * w - 1), hwc, alpha(OVER)) == EINVAL              # three channels under OVER
    assert items_call(L, item(d_out=0x20001), fmt(F16), alpha(STRAIGHT, scale=0.5)) == EINVAL  # an element's alignment, as ever
    if L.ffhip_device_count() == 0:                                                           # good arguments: only the device is missed
        assert items_call(L, item(row_stride=4 * w), hwc, alpha(STRAIGHT)) == ENODEV
        assert items_call(L, item(row_stride=3 * w), hwc, alpha(OVER, pre=1)) == ENODEV
        assert items_call(L, item(row_stride=w, plane_stride=w * h), chw, alpha(PREMULTIPLIED, pre=1)) == ENODEV
        assert items_call(L, item(), fmt(F32), alpha(STRAIGHT, scale=1 / 255, bias=0.5)) == ENODEV


def test_no_record_and_drop_are_the_old_entry(L):
    w = 20
    hwc = fmt(planar=0)
    arr = (capi.TensorItem * 1)(item(row_stride=3 * w - 1))
    assert L.ffhip_bgra_to_tensor_items(arr, 1, C.byref(hwc), None) == EINVAL
    junk = alpha(DROP, pre=7, scale=float("nan"))                                             # nothing but the mode of a DROP record is read
    for a in (None, junk):
        assert items_call(L, item(row_stride=3 * w - 1), hwc, a) == EINVAL
        assert items_call(L, item(), fmt(dtype=3), a) == EINVAL
        assert L.ffhip_bgra_to_tensor_items_alpha(None, 0, C.byref(hwc), C.byref(a) if a else None, None) == 0
        assert L.ffhip_bgra_to_tensor_items_alpha(None, 1, C.byref(hwc), C.byref(a) if a else None, None) == EINVAL
        if L.ffhip_device_count() == 0:
            assert items_call(L, item(row_stride=3 * w), hwc, a) == ENODEV                    # three channels fit
    assert items_call(L, item(row_stride=3 * w), hwc, alpha(STRAIGHT)) == EINVAL


def test_the_premultiplying_resize_checks_as_the_plain_one(L):
    good = capi.ResizeItem(0x10000, 128, 1, 1, 20, 10, 0x20000, 64, 16, 8)
    for change in (dict(width=0), dict(out_width=16385), dict(dst_pitch=60), dict(d_src=0x10002), dict(src_pitch=80)):
        it = capi.ResizeItem(0x10000, 128, 1, 1, 20, 10, 0x20000, 64, 16, 8)
        for k, v in change.items():
            setattr(it, k, v)
        for entry in (L.ffhip_bgra_resize_items, L.ffhip_bgra_resize_items_premultiplied):
            assert entry((capi.ResizeItem * 1)(it), 1, 0, None) == EINVAL, change
    entry = L.ffhip_bgra_resize_items_premultiplied
    assert entry((capi.ResizeItem * 1)(good), 1, 2, None) == EINVAL and entry(None, 1, 0, None) == EINVAL and entry(None, 0, 0, None) == 0
    if L.ffhip_device_count() == 0:
        assert entry((capi.ResizeItem * 1)(good), 1, 1, None) == ENODEV


FILE_ENTRIES = ("png", "vp8l", "webp")


def file_call(L, codec, a, flags=0, f=None, outs=True, n=1):
    bufs, ptrs, lens = ops.file_args([b"not a picture at all"])
    out = (capi.TensorOut * 1)(capi.TensorOut(0x20000, 4096, 1 << 20))
    status = (C.c_int * 1)()
    rc = getattr(L, f"ffhip_{codec}_decode_files_tensor_alpha")(ptrs, lens, n, 2, C.byref(f or fmt()), out if outs else None, None, None, 0, None, None, flags,
                                                               C.byref(a) if a is not None else None, None, status, None)
    return rc, status[0]


@pytest.mark.parametrize("codec", FILE_ENTRIES)
def test_file_calls_refuse_in_front_of_the_device(L, codec):
    flags = capi.FFHIP_WEBP_PIXELS_LIBWEBP if codec == "webp" else 0
    assert file_call(L, codec, alpha(STRAIGHT, pre=1), flags)[0] == EINVAL                    # the chain sets it
    assert file_call(L, codec, alpha(mode=9), flags)[0] == EINVAL
    assert file_call(L, codec, alpha(STRAIGHT, scale=2.0), flags)[0] == EINVAL                 # U8
    assert file_call(L, codec, alpha(OVER, bias=float("nan")), flags, fmt(F32))[0] == EINVAL
    assert file_call(L, codec, alpha(STRAIGHT), flags, outs=False)[0] == EINVAL
    assert file_call(L, codec, alpha(STRAIGHT), flags | 0x40)[0] == EINVAL
    assert file_call(L, codec, alpha(STRAIGHT), flags, n=0)[0] == 0
    if L.ffhip_device_count() == 0:       # good arguments: the file is looked at (and found wanting), then the device is missed
        for a in (alpha(STRAIGHT), alpha(OVER), alpha(DROP, pre=5), None):
            rc, st = file_call(L, codec, a, flags)
            assert rc == ENODEV and st != 0


def test_the_webp_call_needs_the_libwebp_rule(L):
    assert file_call(L, "webp", alpha(STRAIGHT), 0)[0] == EINVAL                              # the reference rule has no alpha
    assert file_call(L, "webp", alpha(OVER), 0)[0] == EINVAL
    assert file_call(L, "webp", alpha(STRAIGHT), capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA)[0] == EINVAL    # the call sets it
    if L.ffhip_device_count() == 0:
        assert file_call(L, "webp", None, 0)[0] == ENODEV and file_call(L, "webp", alpha(DROP), 0)[0] == ENODEV          # the old entry


# ---------------------------------------------------------------------------------------------------- the body on the CPU
def test_the_new_instances_on_the_cpu_at_every_alignment(tmp_path):
    """tests/tools/check_tensor_alpha_body.cpp, built with the address and undefined-behaviour sanitizers and run as a program"""
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))), "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "clang++"
    exe = str(tmp_path / "check_tensor_alpha_body")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + capi.CSRC,
                           os.path.join(ROOT, "tests", "tools", "check_tensor_alpha_body.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "steps: 0 bad" in res.stdout and "sink: checked 138240 cases, 0 bad" in res.stdout and "resize: checked 226 pixels, 0 bad" in res.stdout, res.stdout


# ---------------------------------------------------------------------------------------------------- Python
@pytest.mark.parametrize("bad", ["keep", "over", ("over",), ("over", (1, 2)), ("over", (1, 2, 256)), ("over", (1, 2, -1)), ("over", (0.5, 0, 0)),
                                 ("under", (1, 2, 3)), None, 1, ("over", 7)])
def test_bad_alpha_arguments_are_value_errors_before_any_device_use(bad):
    for call in (tensors.decode_png_to_tensors, tensors.decode_webp_lossless_to_tensors):
        with pytest.raises(ValueError):
            call([b"x"], alpha=bad)
    with pytest.raises(ValueError):
        tensors.decode_webp_to_tensors([b"x"], pixels="libwebp", alpha=bad)
    with pytest.raises(ValueError):
        tensors.tensor_alpha(bad)


def test_alpha_under_the_reference_webp_rule_is_a_value_error():
    for a in ("straight", "premultiplied", ("over", (255, 255, 255))):
        with pytest.raises(ValueError):
            tensors.decode_webp_to_tensors([b"x"], alpha=a)
        with pytest.raises(ValueError):
            tensors.alpha_entry_point("webp", a, "reference")
    with pytest.raises(ValueError):
        tensors.alpha_entry_point("jpeg", "straight")


def test_the_entry_each_combination_goes_through():
    E = tensors.alpha_entry_point
    for a in ("straight", "premultiplied", ("over", (1, 2, 3))):
        assert E("png", a) == "ffhip_png_decode_files_tensor_alpha"
        assert E("vp8l", a) == "ffhip_vp8l_decode_files_tensor_alpha"
        assert E("webp", a, "libwebp") == "ffhip_webp_decode_files_tensor_alpha"
    assert E("png") == E("png", "drop") == "ffhip_png_decode_files_tensor"
    assert E("vp8l", "drop") == "ffhip_vp8l_decode_files_tensor"
    assert E("webp", "drop", "libwebp") == "ffhip_webp_decode_files_tensor_ex"
    assert E("webp", "drop", "reference", oriented=True) == "ffhip_webp_decode_files_tensor_oriented"
    assert E("webp", "drop", "reference", targets=True) == "ffhip_webp_decode_files_tensor_resized"
    assert [tensors.alpha_channels(a) for a in ("drop", "straight", "premultiplied", ("over", (0, 0, 0)))] == [3, 4, 4, 3]


def test_the_record_the_python_layer_builds():
    a = tensors.tensor_alpha(("over", (10, 20, 30)))
    assert (a.mode, a.source_premultiplied, list(a.background)[:3], a.alpha_scale, a.alpha_bias) == (OVER, 0, [30, 20, 10], 1.0, 0.0)
    a = tensors.tensor_alpha("straight", normalised=True, source_premultiplied=True)
    assert (a.mode, a.source_premultiplied) == (STRAIGHT, 1) and np.float32(a.alpha_scale) == np.float32(1 / 255) and a.alpha_bias == 0.0
    assert tensors.tensor_alpha("premultiplied").mode == PREMULTIPLIED and tensors.tensor_alpha().mode == DROP
