"""CPU: the resize stage's C interface (ffhip_resize_axis_taps, ffhip_bgra_resize_items, ffhip_*_decode_files_tensor_resized) -- struct
layouts against the header, the taps against the rule written a second time here, a picture from the library's taps against torch's CPU
interpolate, every refusal before the device is asked for."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from ffpic_amd import capi, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV
BIL, AA = capi.FFHIP_RESIZE_BILINEAR, capi.FFHIP_RESIZE_ANTIALIAS


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


# ---------------------------------------------------------------------------------------------------- the rule, a second time
def rule_taps(n_in, n_out, filt, o):
    """(first, q as int64) of output o: the header's rule, over all source samples at once"""
    S = 2 * max(n_in, n_out) if filt == AA else 2 * n_out
    c = (2 * o + 1) * n_in
    k = np.arange(n_in, dtype=np.int64)
    d = np.abs((2 * k + 1) * n_out - c)
    ks = k[d < S]
    assert len(ks) and np.all(np.diff(ks) == 1)                 # a contiguous run
    r = S - d[d < S]
    R = int(r.sum())
    q = (r * 4096 + R // 2) // R
    m = int(np.argmax(r))                                       # argmax: the lowest k on a tie
    q[m] += 4096 - int(q.sum())
    if q[m] < 0:                                                # step 5: the largest tap cannot pay: the next ones in the same order do
        owed, q[m] = -int(q[m]), 0
        order = np.lexsort((np.arange(len(r)), -r))             # falling r, the lowest k on a tie
        assert order[0] == m
        rest = order[1:]
        before = np.cumsum(q[rest]) - q[rest]                   # what the taps ahead of each have paid at most
        q[rest] -= np.clip(owed - before, 0, q[rest])
    return int(ks[0]), q


def lib_taps(L, n_in, n_out, filt, o):
    first = C.c_int(-1)
    count = L.ffhip_resize_axis_taps(n_in, n_out, filt, o, C.byref(first), None, 0)
    assert count >= 1
    q = np.zeros(count, np.uint16)
    assert L.ffhip_resize_axis_taps(n_in, n_out, filt, o, C.byref(first), q.ctypes.data_as(C.POINTER(C.c_uint16)), count) == count
    return first.value, q


SIDES = (1, 2, 3, 5, 7, 16, 17, 64, 65, 224, 1080, 16384)
SMALL = 224                                                      # every o where both sides are at most this


def outputs_checked(n_in, n_out):
    if n_in <= SMALL and n_out <= SMALL:
        return list(range(n_out))
    rng = np.random.default_rng(n_in * 20000 + n_out)
    return sorted({0, n_out - 1, n_out // 2, *[int(v) for v in rng.integers(0, n_out, 50)]})


@pytest.fixture(scope="module")
def checked(L):
    """{(n_in, n_out, filter): [(o, first, q of the library as uint16, first and q of the rule)]}, computed once"""
    out = {}
    for n_in, n_out, filt in itertools.product(SIDES, SIDES, (BIL, AA)):
        out[n_in, n_out, filt] = [(o,) + lib_taps(L, n_in, n_out, filt, o) + rule_taps(n_in, n_out, filt, o) for o in outputs_checked(n_in, n_out)]
    return out


def test_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    for name in ("FFHIP_RESIZE_BILINEAR 0", "FFHIP_RESIZE_ANTIALIAS 1", "FFHIP_RESIZE_MAX_SIDE 16384"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name
    assert (capi.FFHIP_RESIZE_BILINEAR, capi.FFHIP_RESIZE_ANTIALIAS, capi.FFHIP_RESIZE_MAX_SIDE) == (0, 1, 16384)
    I, S = capi.ResizeItem, capi.Size
    assert C.sizeof(I) == 56
    assert (I.d_src.offset, I.src_pitch.offset, I.x0.offset, I.y0.offset, I.width.offset, I.height.offset) == (0, 8, 16, 20, 24, 28)
    assert (I.d_dst.offset, I.dst_pitch.offset, I.out_width.offset, I.out_height.offset) == (32, 40, 48, 52)
    assert C.sizeof(S) == 8 and (S.width.offset, S.height.offset) == (0, 4)
    for struct, fields in (("ffhip_resize_item", ["d_src", "src_pitch", "x0", "height", "d_dst", "dst_pitch", "out_width", "out_height"]),
                           ("ffhip_size", ["width", "height"])):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        at = [body.index(f) for f in fields]
        assert at == sorted(at), struct
    for entry in ("ffhip_resize_axis_taps", "ffhip_bgra_resize_items", "ffhip_jpeg_decode_files_tensor_resized", "ffhip_webp_decode_files_tensor_resized"):
        assert entry in capi.EXPORTS and re.search(r"\b" + entry + r"\(", text), entry


def test_taps_equal_the_rule(checked):
    """first, count and every weight, both filters, every pair of sides; the taps stay inside the source and sum to 4096"""
    for (n_in, n_out, filt), rows in checked.items():
        for o, first, q, rfirst, rq in rows:
            where = (n_in, n_out, filt, o)
            assert first == rfirst and len(q) == len(rq), where
            assert np.array_equal(q.astype(np.int64), rq), where
            assert 0 <= first and first + len(q) <= n_in, where
            assert int(q.astype(np.int64).sum()) == 4096 and int(rq.sum()) == 4096, where


@pytest.mark.parametrize("filt", [BIL, AA])
@pytest.mark.parametrize("n_in", SIDES)
def test_weights_are_never_negative(checked, n_in, filt):
    """Step 5 of the rule: every q_k >= 0.  The library's 16-bit weights read as signed are never negative and never above 4096 -- also
    where the residual of step 4 alone would be (ANTIALIAS 1080 -> 1: -41 at the largest tap; 16384 -> 3: -454; 16384 -> 17: -9), which
    the rule settles by taking what is owed from the next taps in the same order."""
    for n_out in SIDES:
        for o, first, q, rfirst, rq in checked[n_in, n_out, filt]:
            assert int(q.view(np.int16).min()) >= 0 and int(q.max()) <= 4096, (n_in, n_out, filt, o)
            assert int(rq.min()) >= 0, (n_in, n_out, filt, o, int(rq.min()))


def test_long_runs_pay_their_residual_in_order(L):
    """where step 4 alone would go negative: the largest tap is 0, the taps around it are 0 as far as the debt reaches, sum 4096"""
    for n_in, n_out, owed_alone in ((1080, 1, 41), (16384, 3, 454), (16384, 17, 9)):
        first, q = lib_taps(L, n_in, n_out, AA, 0)
        rfirst, rq = rule_taps(n_in, n_out, AA, 0)
        assert first == rfirst and np.array_equal(q.astype(np.int64), rq) and int(q.astype(np.int64).sum()) == 4096
        r = 2 * n_in - np.abs((2 * (first + np.arange(len(q), dtype=np.int64)) + 1) * n_out - n_in)
        assert q[int(np.argmax(r))] == 0
    for n_in, n_out in ((224, 1), (224, 3), (65, 1), (1080, 17)):       # and short runs never need it: step 4 alone
        for o in range(n_out):
            S, c = 2 * n_in, (2 * o + 1) * n_in
            k = np.arange(n_in, dtype=np.int64)
            d = np.abs((2 * k + 1) * n_out - c)
            r = S - d[d < S]
            q0 = (r * 4096 + int(r.sum()) // 2) // int(r.sum())
            q0[int(np.argmax(r))] += 4096 - int(q0.sum())
            assert q0.min() >= 0 and np.array_equal(lib_taps(L, n_in, n_out, AA, o)[1].astype(np.int64), q0)


def test_identity_and_single_sample(L):
    for n in (1, 2, 17, 224, 16384):
        for filt in (BIL, AA):
            for o in {0, n // 2, n - 1}:
                first, q = lib_taps(L, n, n, filt, o)
                assert (first, list(q)) == (o, [4096])
    for n_out in (1, 2, 5, 224, 16384):
        for filt in (BIL, AA):
            for o in {0, n_out // 2, n_out - 1}:
                assert lib_taps(L, 1, n_out, filt, o)[0] == 0 and list(lib_taps(L, 1, n_out, filt, o)[1]) == [4096]


def test_taps_refusals_and_cap(L):
    first, q = C.c_int(), (C.c_uint16 * 8)()
    for args in ((0, 4, AA, 0), (16385, 4, AA, 0), (4, 0, BIL, 0), (4, 16385, BIL, 0), (4, 4, 2, 0), (4, 4, -1, 0), (4, 4, AA, -1), (4, 4, AA, 4)):
        assert L.ffhip_resize_axis_taps(*args, C.byref(first), q, 8) == EINVAL, args
    assert L.ffhip_resize_axis_taps(4, 4, AA, 0, None, q, 8) == EINVAL
    assert L.ffhip_resize_axis_taps(4, 4, AA, 0, C.byref(first), None, 8) == EINVAL
    assert L.ffhip_resize_axis_taps(4, 4, AA, 0, C.byref(first), q, -1) == EINVAL
    # a short array takes the first `cap` weights; the count is the run's
    full = lib_taps(L, 37, 8, AA, 3)[1]
    for k in range(8):
        q[k] = 0xBEEF
    assert L.ffhip_resize_axis_taps(37, 8, AA, 3, C.byref(first), q, 3) == len(full) > 3
    assert list(q)[:3] == list(full[:3]) and list(q)[3:] == [0xBEEF] * 5
    assert L.ffhip_resize_axis_taps(16384, 16384, BIL, 16383, C.byref(first), q, 8) == 1 and first.value == 16383


def test_python_axis_taps(L):
    first, taps = tensors.axis_taps(53, 8, antialias=True)
    assert len(first) == len(taps) == 8
    for o in range(8):
        f, q = rule_taps(53, 8, AA, o)
        assert first[o] == f and np.array_equal(taps[o], q) and taps[o].dtype == np.uint16
    first, taps = tensors.axis_taps(53, 8, antialias=False)
    assert max(len(t) for t in taps) <= 2


# ---------------------------------------------------------------------------------------------------- against torch's interpolate
@pytest.mark.parametrize("shape", [(37, 53, 8, 8), (240, 135, 14, 14), (100, 7, 9, 20), (33, 65, 64, 80)])
@pytest.mark.parametrize("antialias", [False, True])
def test_library_taps_against_torch_interpolate(L, shape, antialias):
    """a picture resized in numpy with the LIBRARY's taps against float64 bilinear interpolation: each weight is off by at most 0.5 / 4096,
    the residual moved by step 4 by at most n 0.5 / 4096, so sum |dq| <= n / 4096 per axis; plus the final rounding"""
    import torch
    h, w, oh, ow = shape
    img = np.random.default_rng(h * w + oh).integers(0, 256, (h, w, 3), dtype=np.uint8)
    W, most = [], []
    for n_in, n_out in ((h, oh), (w, ow)):
        first, taps = tensors.axis_taps(n_in, n_out, antialias)
        m = np.zeros((n_out, n_in), np.int64)
        for o in range(n_out):
            m[o, first[o]:first[o] + len(taps[o])] = taps[o]
        W.append(m)
        most.append(max(len(t) for t in taps))
    ny, nx = most
    out = (np.einsum("oy,yxc,px->opc", W[0], img.astype(np.int64), W[1]) + (1 << 23)) >> 24
    ref = torch.nn.functional.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None].double(), size=(oh, ow), mode="bilinear",
                                          align_corners=False, antialias=antialias)[0].permute(1, 2, 0).numpy()
    bound = 0.5 + 255 * (nx + ny) / 4096
    worst = float(np.abs(out - ref).max())
    print(f"{shape} antialias={antialias}: taps {nx} x {ny}, worst {worst:.3f}, bound {bound:.3f}")
    assert out.min() >= 0 and out.max() <= 255
    assert worst <= bound


# ---------------------------------------------------------------------------------------------------- refusals without a device
def item(**kw):
    """a good item: a 20 x 10 rectangle at (2, 3) of a picture with pitch 128 onto 7 x 5 with pitch 32"""
    it = capi.ResizeItem()
    it.d_src, it.src_pitch, it.x0, it.y0, it.width, it.height = 0x10000, 128, 2, 3, 20, 10
    it.d_dst, it.dst_pitch, it.out_width, it.out_height = 0x20000, 32, 7, 5
    for k, v in kw.items():
        setattr(it, k, v)
    return it


def call(L, items, filt=AA, n=None):
    arr = (capi.ResizeItem * max(len(items), 1))(*items)
    return L.ffhip_bgra_resize_items(arr, len(items) if n is None else n, filt, None)


def test_no_items_is_ok_and_bad_counts_and_filters_are_refused(L):
    assert call(L, []) == 0 and call(L, [], BIL) == 0
    assert L.ffhip_bgra_resize_items(None, 0, AA, None) == 0
    assert call(L, [], n=-1) == EINVAL
    assert L.ffhip_bgra_resize_items(None, 1, AA, None) == EINVAL
    for filt in (2, -1, 7):
        assert call(L, [item()], filt) == EINVAL and call(L, [], filt) == EINVAL


BAD_ITEMS = {
    "width 0": dict(width=0), "height 0": dict(height=0), "out_width 0": dict(out_width=0), "out_height 0": dict(out_height=0),
    "width 16385": dict(width=16385, src_pitch=4 * 16400), "height 16385": dict(height=16385, src_pitch=80, x0=0),
    "out_width 16385": dict(out_width=16385, dst_pitch=4 * 16385), "out_height 16385": dict(out_height=16385),
    "width -1": dict(width=-1), "x0 -1": dict(x0=-1), "y0 -1": dict(y0=-1),
    "no source": dict(d_src=None), "source at 2": dict(d_src=0x10002), "source pitch % 4": dict(src_pitch=130), "source pitch 0": dict(src_pitch=0),
    "rectangle wider than the pitch": dict(src_pitch=84),
    "rows past 31 bits": dict(src_pitch=1 << 20, y0=2040, height=9), "y0 past 31 bits": dict(src_pitch=1 << 20, y0=0x7fffffff),
    "no destination": dict(d_dst=None), "destination at 1": dict(d_dst=0x20001), "destination at 2": dict(d_dst=0x20002),
    "destination pitch % 4": dict(dst_pitch=30), "destination pitch below the row": dict(dst_pitch=24), "negative destination pitch": dict(dst_pitch=-32),
}


@pytest.mark.parametrize("name", list(BAD_ITEMS))
def test_bad_items_are_refused_before_the_device_is_asked_for(L, name):
    for filt in (BIL, AA):
        for items in ([item(**BAD_ITEMS[name])], [item(), item(), item(**BAD_ITEMS[name])]):
            assert call(L, items, filt) == EINVAL, name


def test_limits_are_inclusive(L):
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present: these addresses are not memory; the -m gpu tests run the call")
    good = [item(), item(src_pitch=88), item(dst_pitch=28), item(width=16384, x0=0, src_pitch=65536, height=1), item(out_width=16384, dst_pitch=65536),
            item(height=16384, y0=0, src_pitch=80, x0=0), item(out_height=16384), item(src_pitch=1 << 20, y0=2037, height=10),
            item(width=1, height=1, out_width=1, out_height=1, dst_pitch=4)]
    for it in good:
        for filt in (BIL, AA):
            assert call(L, [it], filt) == ENODEV
    assert call(L, good) == ENODEV


@pytest.mark.parametrize("entry", ["ffhip_jpeg_decode_files_tensor_resized", "ffhip_webp_decode_files_tensor_resized"])
def test_file_calls_refuse_missing_arguments(L, entry):
    call_ = getattr(L, entry)
    data = np.frombuffer(b"\xff\xd8 not a picture", dtype=np.uint8)
    files, lens = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(data.size)
    outs, status, size = (capi.TensorOut * 1)(), (C.c_int * 1)(), (capi.Size * 1)(capi.Size(8, 8))
    f = capi.TensorFormat()
    f.dtype, f.bgr, f.planar = capi.FFHIP_TENSOR_U8, 0, 1
    for c in range(3):
        f.scale[c], f.bias[c] = 1, 0
    bad = capi.TensorFormat()
    bad.dtype = 7
    assert call_(files, lens, 0, 2, C.byref(f), outs, None, size, AA, None, status, None) == 0
    assert call_(None, None, 0, 2, C.byref(f), None, None, None, BIL, None, None, None) == 0
    assert call_(files, lens, -1, 2, C.byref(f), outs, None, size, AA, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(f), outs, None, None, AA, None, status, None) == EINVAL        # no out_size
    assert call_(files, lens, 1, 2, C.byref(f), outs, None, size, 2, None, status, None) == EINVAL           # unknown filter
    assert call_(files, lens, 0, 2, C.byref(f), outs, None, size, -1, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, None, outs, None, size, AA, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(bad), outs, None, size, AA, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(f), None, None, size, AA, None, status, None) == EINVAL
    assert call_(None, lens, 1, 2, C.byref(f), outs, None, size, AA, None, status, None) == EINVAL
    assert call_(files, None, 1, 2, C.byref(f), outs, None, size, AA, None, status, None) == EINVAL
    assert call_(files, lens, 1, 2, C.byref(f), outs, None, size, AA, None, None, None) == EINVAL
    if L.ffhip_device_count() == 0:   # good arguments: the file is looked at (and found wanting), then the device is missed
        assert call_(files, lens, 1, 2, C.byref(f), outs, None, size, AA, None, status, None) == ENODEV
        assert status[0] != 0


def test_python_size_argument_errors_come_before_the_device():
    files = [b"\xff\xd8 not a picture"] * 2
    for decode in (tensors.decode_jpeg_to_tensors, tensors.decode_webp_to_tensors):
        for size in ([(8, 8)], [(8, 8)] * 3, (0, 8), (8, -1), [(8, 8), (8, 0)], (8, 16385), [(8, 8, 8), (8, 8)]):
            with pytest.raises(ValueError):
                decode(files, size=size)
