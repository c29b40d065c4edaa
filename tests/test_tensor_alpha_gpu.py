"""GPU: alpha into the tensors (include/ffpic_hip.h).  ffhip_bgra_to_tensor_items_alpha in every format, mode and source
kind over one mixed batch; ffhip_bgra_resize_items_premultiplied against premultiply-then-filter, with the two properties it is for; the
three files-to-tensors calls with alpha= against the witness chain over the picture the BGRA file call of the same codec delivers.  The
witness is tests/alpha_spec.py; every comparison is exact."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import alpha_spec as S
import exif_cases as X
import png_writer
import vp8l_writer
import webp_alpha_cases as K
import webp_alpha_writer as A
from ffpic_amd import capi, ops, tensors

pytestmark = pytest.mark.gpu

U8, F16, F32 = capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16, capi.FFHIP_TENSOR_F32
NP_DTYPE = {U8: np.uint8, F16: np.float16, F32: np.float32}
DTYPE_NAME = {U8: "uint8", F16: "float16", F32: "float32"}
FORMATS = list(itertools.product((U8, F16, F32), (1, 0), (0, 1)))          # dtype, planar, bgr
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BACKGROUND = (254, 200, 37)                                                # r, g, b
ALPHAS = (0, 1, 127, 128, 254, 255)
FILL = 0xA5
MODES = [("straight", False), ("straight", True), ("premultiplied", False), ("premultiplied", True), ("over", False), ("over", True)]


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    capi.setenv("FFHIP_TENSOR_PART_BYTES", None)


@functools.lru_cache(maxsize=None)
def axis_taps(n_in, n_out, antialias):
    return tensors.axis_taps(n_in, n_out, antialias)


def picture(rng, h, w, premultiplied=False):
    """random colour under the alphas that matter and random ones; a premultiplied picture keeps every colour byte at or below its alpha"""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = px.reshape(-1, 4)
    flat[::2, 3] = np.resize(np.array(ALPHAS, np.uint8), len(flat[::2]))
    if premultiplied:
        px[..., :3] = np.minimum(px[..., :3], px[..., 3:4])
    return px


def the_format(dtype, planar, bgr, normalise=True):
    chans = slice(None, None, -1) if bgr else slice(None)
    norm = dtype != U8 and normalise
    return tensors.tensor_format(DTYPE_NAME[dtype], "CHW" if planar else "HWC", "BGR" if bgr else "RGB", MEAN[chans] if norm else None, STD[chans] if norm else None)


def spec_args(f, record):
    return dict(np_dtype=NP_DTYPE[f.dtype], planar=bool(f.planar), bgr=bool(f.bgr), scale=list(f.scale), bias=list(f.bias),
                alpha_scale=record.alpha_scale, alpha_bias=record.alpha_bias, background_rgb=BACKGROUND)


# ---------------------------------------------------------------------------------------------------- the sink
#        width, height, offset in elements from a 16-byte boundary, extra elements per row and per plane
ITEMS = [(1, 1, 0, 0), (3, 2, 0, 0), (13, 5, 1, 0), (17, 3, 7, 0), (64, 2, 0, 0), (67, 4, 0, 5)]


def run_sink(f, mode, pre, rng):
    """the batch of ITEMS through ffhip_bgra_to_tensor_items_alpha, every output in ONE 0xA5-filled allocation -> (device bytes, expected)"""
    record = tensors.tensor_alpha(("over", BACKGROUND) if mode == "over" else mode, normalised=f.dtype != U8, source_premultiplied=pre)
    if f.dtype != U8:
        record.alpha_bias = 0.25
    nc, es, dt = tensors.alpha_channels(("over", BACKGROUND) if mode == "over" else mode), np.dtype(NP_DTYPE[f.dtype]).itemsize, NP_DTYPE[f.dtype]
    pics = [picture(rng, h + 1, w + 2, pre) for w, h, _, _ in ITEMS]
    places, at = [], 0
    for w, h, off, extra in ITEMS:
        rs = (w if f.planar else nc * w) + extra
        ps = rs * (h - 1) + w + extra if f.planar else 0
        span = (nc - 1) * ps + rs * (h - 1) + w if f.planar else rs * (h - 1) + nc * w
        places.append((at + off, rs, ps))
        at += (off + span + 3 + 15) // 16 * 16
    exp = np.full(at * es, FILL, np.uint8)
    dev = ops.DeviceBuffer(host=exp)
    srcs, items = [], []
    for (w, h, _, _), (start, rs, ps), pic in zip(ITEMS, places, pics):
        srcs.append(ops.DeviceBuffer(host=np.ascontiguousarray(pic)))
        items.append(capi.TensorItem(srcs[-1].ptr, 4 * pic.shape[1], 2, 1, w, h, dev.ptr + start * es, rs, ps))
        view = np.lib.stride_tricks.as_strided(exp.view(dt)[start:], (nc, h, w) if f.planar else (h, w, nc), (ps * es, rs * es, es) if f.planar else (rs * es, nc * es, es))
        view[...] = S.sink(pic[1:1 + h, 2:2 + w], mode, source_premultiplied=pre, **spec_args(f, record))
    tensors.bgra_to_tensors(items, f, alpha=record)
    capi.sync(None)
    return dev.to_host((exp.size,), np.uint8), exp


@pytest.mark.parametrize("dtype,planar,bgr", FORMATS)
def test_the_sink_in_every_mode_and_source_kind(dtype, planar, bgr):
    """inside: the witness, to the bit (floats with a normalising scale and bias, and a bias on alpha); outside: still 0xA5"""
    rng = np.random.default_rng(4000 + 100 * dtype + 10 * planar + bgr)
    f = the_format(dtype, planar, bgr)
    for mode, pre in MODES:
        got, exp = run_sink(f, mode, pre, rng)
        assert np.array_equal(got, exp), (mode, pre, np.flatnonzero(got != exp)[:8].tolist())


@pytest.mark.parametrize("planar", [1, 0])
def test_every_premultiplied_pair_on_the_device(planar):
    """every (p, a) with p <= a in one 256 x 256 picture: un-premultiplied and composited on the device as the integer rule says"""
    a, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    p = np.minimum(p, a)
    pic = np.stack([p, a - p, np.minimum(255 - p, a), a], -1).astype(np.uint8)
    src = ops.DeviceBuffer(host=pic)
    f = the_format(U8, planar, 0)
    for mode, nc in (("straight", 4), ("over", 3)):
        record = tensors.tensor_alpha(("over", BACKGROUND) if mode == "over" else mode, source_premultiplied=True)
        dev = ops.DeviceBuffer(host=np.full(nc * 65536, FILL, np.uint8))
        tensors.bgra_to_tensors([capi.TensorItem(src.ptr, 1024, 0, 0, 256, 256, dev.ptr, 256 if planar else nc * 256, 65536)], f, alpha=record)
        capi.sync(None)
        want = S.sink(pic, mode, source_premultiplied=True, **spec_args(f, record))
        assert np.array_equal(dev.to_host((nc * 65536,), np.uint8), want.reshape(-1)), mode


def test_no_record_and_drop_give_the_bytes_of_the_old_call():
    rng = np.random.default_rng(4100)
    pic = picture(rng, 9, 70)
    src = ops.DeviceBuffer(host=pic)
    f = the_format(F16, 0, 0)
    outs = []
    for record in ("old", None, tensors.tensor_alpha("drop")):
        dev = ops.DeviceBuffer(host=np.full(2 * (9 * 3 * 70 + 32), FILL, np.uint8))
        item = capi.TensorItem(src.ptr, 4 * 70, 0, 0, 70, 9, dev.ptr + 2, 3 * 70, 0)
        if record == "old":
            tensors.bgra_to_tensors([item], f)
        else:
            arr = (capi.TensorItem * 1)(item)
            capi.check(capi.lib().ffhip_bgra_to_tensor_items_alpha(arr, 1, C.byref(f), C.byref(record) if record else None, None), "items_alpha")
        capi.sync(None)
        outs.append(dev.to_host((2 * (9 * 3 * 70 + 32),), np.uint8))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and (outs[0] != FILL).any()


# ---------------------------------------------------------------------------------------------------- the resize
SHAPES = [(5, 3, 2, 2), (37, 53, 8, 8), (3, 3, 7, 5), (300, 2, 7, 1), (4100, 1, 3, 1)]      # width, height -> out width, out height


def run_resize(pics, antialias, premultiplied):
    """the SHAPES in one call, outputs in one 0xA5-filled allocation with padded rows -> [out pictures], and the padding checked untouched"""
    places, at = [], 0
    for _, _, ow, oh in SHAPES:
        pitch = 4 * (ow + 2)
        places.append((at, pitch))
        at += pitch * oh + 16
    host = np.full(at, FILL, np.uint8)
    dev = ops.DeviceBuffer(host=host)
    srcs = [ops.DeviceBuffer(host=np.ascontiguousarray(p)) for p in pics]
    items = [capi.ResizeItem(s.ptr, 4 * w, 0, 0, w, h, dev.ptr + off, pitch, ow, oh) for s, (w, h, ow, oh), (off, pitch) in zip(srcs, SHAPES, places)]
    tensors.resize_bgra(items, antialias=antialias, premultiplied=premultiplied)
    capi.sync(None)
    got = dev.to_host((at,), np.uint8)
    outs, mask = [], np.ones(at, bool)
    for (_, _, ow, oh), (off, pitch) in zip(SHAPES, places):
        rows = np.lib.stride_tricks.as_strided(got[off:], (oh, 4 * ow), (pitch, 1))
        outs.append(rows.reshape(oh, ow, 4).copy())
        for y in range(oh):
            mask[off + y * pitch:off + y * pitch + 4 * ow] = False
    assert (got[mask] == FILL).all()
    return outs


@pytest.fixture(scope="module")
def resize_sources():
    rng = np.random.default_rng(4200)
    return [picture(rng, h, w) for w, h, _, _ in SHAPES]


@pytest.mark.parametrize("antialias", [False, True])
def test_the_premultiplying_resize_is_premultiply_then_the_rule(resize_sources, antialias):
    got = run_resize(resize_sources, antialias, True)
    for pic, out, (w, h, ow, oh) in zip(resize_sources, got, SHAPES):
        assert np.array_equal(out, S.resize_premultiplied(pic, oh, ow, antialias, axis_taps)), (w, h, ow, oh)
        assert (out[..., :3] <= out[..., 3:4]).all()                       # a premultiplied picture


@pytest.mark.parametrize("antialias", [False, True])
def test_the_colour_under_transparent_pixels_does_not_bleed(resize_sources, antialias):
    """two sources that differ only where a == 0: identical through the premultiplying call -- and not through the plain one"""
    rng = np.random.default_rng(4300)
    twins = []
    for pic in resize_sources:
        t = pic.copy()
        hidden = t[..., 3] == 0
        assert hidden.any()
        t[hidden, :3] = 255 - t[hidden, :3] // 2
        twins.append(t)
    for a, b in zip(run_resize(resize_sources, antialias, True), run_resize(twins, antialias, True)):
        assert np.array_equal(a, b)
    plain = zip(run_resize(resize_sources, antialias, False), run_resize(twins, antialias, False))
    assert any(not np.array_equal(a, b) for a, b in plain)


@pytest.mark.parametrize("antialias", [False, True])
def test_opaque_pictures_resize_as_through_the_plain_call(resize_sources, antialias):
    opaque = [p.copy() for p in resize_sources]
    for p in opaque:
        p[..., 3] = 255
    for a, b in zip(run_resize(opaque, antialias, True), run_resize(opaque, antialias, False)):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- files to tensors
def png_files():
    rng = np.random.default_rng(4400)
    palette = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    trns = bytes(int(v) for v in rng.integers(0, 256, 11))
    return [png_writer.write(rng.integers(0, 16, (13, 21, 1)), 3, 4, palette=palette, trns=trns),                # palette + tRNS
            png_writer.write(picture(rng, 9, 16)[..., 2:4].astype(np.int64), 4, 8, filters=4, interlace=True),   # grey + alpha, Adam7
            png_writer.write(picture(rng, 20, 33)[..., [2, 1, 0, 3]].astype(np.int64), 6, 8, filters=2)]         # RGBA


def vp8l_files():
    rng = np.random.default_rng(4500)
    words = lambda h, w: picture(rng, h, w).view(np.uint32).reshape(h, w)   # noqa: E731
    return [vp8l_writer.write(words(11, 19), alpha=True), vp8l_writer.write(words(14, 9), alpha=False), vp8l_writer.write(words(7, 40), alpha=True)]


def webp_files():
    rng = np.random.default_rng(4600)
    plane = lambda h, w: picture(rng, h, w)[..., 3]                         # noqa: E731
    return [A.wrap(K.carrier(23, 11), plane(11, 23), A.RAW, A.HORIZONTAL), A.wrap(K.carrier(17, 20), plane(20, 17), A.LOSSLESS, A.NONE),
            K.carrier(16, 16)]                                              # the last: no VP8X, no plane


CODECS = {
    "png": (png_files, lambda files, **kw: tensors.decode_png_to_tensors(files, **kw), lambda files, **kw: ops.png_decode_files_device(files, **kw)),
    "vp8l": (vp8l_files, lambda files, **kw: tensors.decode_webp_lossless_to_tensors(files, **kw), lambda files, **kw: ops.vp8l_decode_files_device(files, **kw)),
    "webp": (webp_files, lambda files, **kw: tensors.decode_webp_to_tensors(files, pixels="libwebp", **kw),
             lambda files, **kw: ops.webp_decode_files_device(files, pixels="libwebp", alpha=True, **kw)),
}


@pytest.fixture(scope="module", params=list(CODECS))
def codec(request):
    """(name, files, the tensor call, the pictures the BGRA file call of the same codec delivers)"""
    capi.require_device(0)
    make, to_tensors, to_bgra = CODECS[request.param]
    files = make()
    pictures = to_bgra(files)[1]
    assert any((p[..., 3] != 255).any() for p in pictures) and max(max(p.shape[:2]) for p in pictures) <= 48
    return request.param, files, to_tensors, pictures


OPTIONS = {"plain": dict(), "sized": dict(size=(8, 8)), "turned and sized": dict(size=(8, 8), orientation=6)}
LOOKS = [dict(dtype="uint8", layout="CHW", order="RGB"), dict(dtype="float32", layout="HWC", order="BGR", mean=MEAN[::-1], std=STD[::-1]),
         dict(dtype="float16", layout="CHW", order="RGB", std=STD)]


def witness(pic, alpha, look, size=None, orientation=1):
    f = tensors.tensor_format(look["dtype"], look["layout"], look["order"], look.get("mean"), look.get("std"))
    record = tensors.tensor_alpha(alpha, normalised="mean" in look or "std" in look)
    args = spec_args(f, record)
    mode = alpha[0] if isinstance(alpha, tuple) else alpha
    return S.chain(pic, mode, axis_taps, X.orient, size, orientation, True, **args)


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("alpha", ["straight", "premultiplied", ("over", BACKGROUND)], ids=["straight", "premultiplied", "over"])
def test_files_to_tensors_equal_the_witness_chain(codec, alpha, option):
    name, files, to_tensors, pictures = codec
    for look in LOOKS:
        got = to_tensors(files, alpha=alpha, **look, **OPTIONS[option])
        for k, (t, pic) in enumerate(zip(got, pictures)):
            want = witness(pic, alpha, look, **OPTIONS[option])
            assert tuple(t.shape) == want.shape, (name, k, look)
            assert np.array_equal(t.cpu().numpy().view(np.uint8), want.view(np.uint8)), (name, k, look["dtype"])


def test_stacked_straight_tensors_have_four_channels(codec):
    name, files, to_tensors, pictures = codec
    got = to_tensors(files, alpha="straight", size=(8, 8), stack=True)
    assert tuple(got.shape) == (len(files), 4, 8, 8)
    for k, pic in enumerate(pictures):
        assert np.array_equal(got[k].cpu().numpy(), witness(pic, "straight", LOOKS[0], size=(8, 8))), (name, k)


def test_a_lossless_file_with_the_alpha_bit_unset_is_opaque():
    files = vp8l_files()
    assert [ops.vp8l_probe(f)[2] for f in files] == [1, 0, 1]
    with_alpha = tensors.decode_webp_lossless_to_tensors(files, alpha="straight")[1].cpu().numpy()
    dropped = tensors.decode_webp_lossless_to_tensors(files, alpha="drop")[1].cpu().numpy()
    assert (with_alpha[3] == 255).all() and np.array_equal(with_alpha[:3], dropped)
    over = tensors.decode_webp_lossless_to_tensors(files, alpha=("over", BACKGROUND))[1].cpu().numpy()
    assert np.array_equal(over, dropped)


def test_drop_is_the_call_without_the_argument(codec):
    name, files, to_tensors, _ = codec
    for kw in (dict(), dict(size=(8, 8), orientation=6, dtype="float32", std=STD)):
        for a, b in zip(to_tensors(files, alpha="drop", **kw), to_tensors(files, **kw)):
            assert tuple(a.shape)[0] == 3 and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), name


def test_many_parts_give_the_same_tensors(codec):
    name, files, to_tensors, pictures = codec
    kw = dict(alpha="premultiplied", size=(8, 8), orientation=6)
    whole = [t.cpu().numpy() for t in to_tensors(files, **kw)]
    capi.setenv("FFHIP_TENSOR_PART_BYTES", "1000")
    parts = [t.cpu().numpy() for t in to_tensors(files, **kw)]
    assert capi.lib().ffhip_debug_tensor_last_parts() == len(files)
    for k, (a, b, pic) in enumerate(zip(whole, parts, pictures)):
        assert np.array_equal(a, b) and np.array_equal(a, witness(pic, "premultiplied", LOOKS[0], size=(8, 8), orientation=6)), (name, k)


def test_a_damaged_file_gets_its_decoders_code_and_the_others_are_delivered(codec):
    name, files, to_tensors, pictures = codec
    damaged = {"png": lambda f: f[:len(f) // 2], "vp8l": lambda f: f[:len(f) // 2],
               "webp": lambda f: A.with_alph(f, lambda p: p[:len(p) // 2])}[name](files[0])
    batch = [files[1], damaged, files[2]]
    code = CODECS[name][2](batch, strict=False)[3]
    assert code[1] != 0 and code[0] == code[2] == 0
    got, status = to_tensors(batch, alpha="straight", strict=False)
    assert list(status) == list(code) and got[1] is None
    for t, pic in zip((got[0], got[2]), (pictures[1], pictures[2])):
        assert np.array_equal(t.cpu().numpy(), witness(pic, "straight", LOOKS[0]))
    with pytest.raises(capi.FfhipError):
        to_tensors(batch, alpha="straight")
