"""GPU: BGRA rectangles resized on the device.  ffhip_bgra_resize_items for every pair of shapes and both filters against the rule written
in numpy as integer matrices -- exactly, with every byte around the outputs checked untouched --; the resized file calls against the BGRA
file calls underneath, the numpy rule and the tensor formatting; the torch layer.  No tolerance anywhere."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ffpic_amd import capi, ops, tensors
from test_jpeg_mixed_gpu import _pil_file, _writer_file
from test_webp_front_capi import NAMES, UNPINNED, file_bytes

pytestmark = pytest.mark.gpu

BIL, AA = capi.FFHIP_RESIZE_BILINEAR, capi.FFHIP_RESIZE_ANTIALIAS
U8, F16, F32 = capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16, capi.FFHIP_TENSOR_F32
NP_DTYPE = {U8: np.uint8, F16: np.float16, F32: np.float32}
FORMATS = list(itertools.product((U8, F16, F32), (1, 0), (0, 1)))          # dtype, planar, bgr
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = 0xA5


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    capi.setenv("FFHIP_TENSOR_PART_BYTES", None)


# ---------------------------------------------------------------------------------------------------- the rule in numpy
_MATRICES = {}


def axis_matrix(n_in, n_out, filt):
    """W [n_out][n_in] int64: the rule (include/ffpic_hip.h), all output indices at once; not taken from the library's taps"""
    key = (n_in, n_out, filt)
    if key not in _MATRICES:
        S = 2 * max(n_in, n_out) if filt == AA else 2 * n_out
        c = (2 * np.arange(n_out, dtype=np.int64)[:, None] + 1) * n_in
        d = np.abs((2 * np.arange(n_in, dtype=np.int64)[None, :] + 1) * n_out - c)
        r = np.where(d < S, S - d, 0)
        R = r.sum(1, keepdims=True)
        q = (r * 4096 + R // 2) // R
        best = np.argmax(r, 1)                                                      # argmax: the lowest k on a tie
        q[np.arange(n_out), best] += 4096 - q.sum(1)
        for o in np.nonzero(q[np.arange(n_out), best] < 0)[0]:                      # step 5: the next taps in the same order pay
            owed, q[o, best[o]] = -int(q[o, best[o]]), 0
            rest = np.lexsort((np.arange(n_in), -r[o]))[1:]                         # falling r, the lowest k on a tie
            before = np.cumsum(q[o, rest]) - q[o, rest]
            q[o, rest] -= np.clip(owed - before, 0, q[o, rest])
        assert np.all(q.sum(1) == 4096) and q.min() >= 0
        _MATRICES[key] = q
    return _MATRICES[key]


def resize_rule(v, oh, ow, filt):
    """[h][w][C] uint8 -> [oh][ow][C] uint8: (Wy v Wx^T + 2^23) >> 24 per channel"""
    Wy, Wx = axis_matrix(v.shape[0], oh, filt), axis_matrix(v.shape[1], ow, filt)
    # the integer products through float64 matrix products: every partial sum is an integer below 2^53, so they are exact
    acc = np.tensordot(Wy.astype(np.float64), v.astype(np.float64), (1, 0))                     # [oh][w][C]
    acc = np.tensordot(acc, Wx.astype(np.float64), (1, 1)).transpose(0, 2, 1).astype(np.int64)  # [oh][C][ow] -> [oh][ow][C]
    out = (acc + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255                                  # no clamp needed
    return out.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- the items call
def run_resize(src, cases, filt, stream=None, one_by_one=False):
    """cases (x0, y0, w, h, ow, oh, extra pitch in pixels) of the host picture `src` [H][W][4] through ffhip_bgra_resize_items, all outputs
    in ONE 0xA5-filled allocation -> (device bytes, expected bytes)"""
    dsrc = ops.DeviceBuffer(host=np.ascontiguousarray(src))
    places, at = [], 0
    for k, (x0, y0, w, h, ow, oh, extra) in enumerate(cases):
        pitch = 4 * (ow + extra)
        at += 4 * (k % 3)                                                   # outputs start at any multiple of 4
        places.append((at, pitch))
        at += pitch * (oh - 1) + 4 * ow + 12
    exp = np.full(at + 16, FILL, np.uint8)
    dev = ops.DeviceBuffer(host=exp)
    items = []
    for (x0, y0, w, h, ow, oh, extra), (off, pitch) in zip(cases, places):
        items.append(capi.ResizeItem(dsrc.ptr, src.shape[1] * 4, x0, y0, w, h, dev.ptr + off, pitch, ow, oh))
        view = np.lib.stride_tricks.as_strided(exp[off:], (oh, ow, 4), (pitch, 4, 1))
        view[...] = resize_rule(src[y0:y0 + h, x0:x0 + w], oh, ow, filt)
    for part in ([[it] for it in items] if one_by_one else [items]):
        tensors.resize_bgra(part, antialias=filt == AA, stream=stream)
    capi.sync(stream)
    return dev.to_host((exp.size,), np.uint8), exp


WIDTHS = (1, 2, 3, 5, 17, 63, 64, 65, 130, 257)
HEIGHTS = (1, 2, 3, 17, 40)
OUTS = (1, 2, 3, 7, 16, 33, 64, 65)
X0S = (0, 1, 3)


@pytest.mark.parametrize("filt", [BIL, AA])
def test_every_shape_pair(filt):
    """every source width x height x output width x height x x0 in ONE call per filter: inside equals the rule, outside is still 0xA5"""
    rng = np.random.default_rng(2000 + filt)
    src = rng.integers(0, 256, (max(HEIGHTS) + 3, max(WIDTHS) + max(X0S), 4), dtype=np.uint8)        # alpha random too
    cases = [(x0, (w + ow) % 4, w, h, ow, oh, (w + h + oh) % 3) for w, h, ow, oh, x0 in itertools.product(WIDTHS, HEIGHTS, OUTS, OUTS, X0S)]
    got, exp = run_resize(src, cases, filt)
    assert np.array_equal(got, exp)


@pytest.fixture(scope="module")
def big_picture():
    return np.random.default_rng(77).integers(0, 256, (2160, 3840, 4), dtype=np.uint8)


@pytest.mark.parametrize("filt", [BIL, AA])
def test_large_shrink(big_picture, filt):
    """2160 x 3840 -> 224 x 224 (35 x 20 taps); 4097 x 31 -> 5 x 64 (1639 taps down an output column); runs so long that the residual
    is paid by more than the largest tap (1080 -> 1, either axis); and what the LDS staging adds: a row longer than one chunk of 4096
    pixels (three refills, taps that straddle them), more than one tile of 256 output columns"""
    got, exp = run_resize(big_picture, [(0, 0, 3840, 2160, 224, 224, 0)], filt)
    assert np.array_equal(got, exp)
    rng = np.random.default_rng(78)
    tall = rng.integers(0, 256, (4097, 31, 4), dtype=np.uint8)
    got, exp = run_resize(tall, [(0, 0, 31, 4097, 64, 5, 1), (1, 2, 30, 1080, 3, 1, 0)], filt)
    assert np.array_equal(got, exp)
    wide = rng.integers(0, 256, (3, 9001, 4), dtype=np.uint8)
    got, exp = run_resize(wide, [(0, 0, 9001, 3, 5, 2, 0), (1, 0, 9000, 3, 300, 3, 2), (3, 1, 8200, 2, 700, 1, 1), (0, 0, 300, 3, 9001 // 8, 4, 0), (5, 0, 1080, 3, 1, 2, 1)], filt)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("filt", [BIL, AA])
def test_upscale_identity_and_constant(filt):
    rng = np.random.default_rng(79)
    src = rng.integers(0, 256, (48, 70, 4), dtype=np.uint8)
    got, exp = run_resize(src, [(2, 1, 5, 7, 48, 64, 3), (0, 0, 70, 48, 70, 48, 2), (3, 2, 17, 9, 17, 9, 0)], filt)
    assert np.array_equal(got, exp)
    # identity: the source bytes themselves (not only the rule's word for it)
    dsrc, ddst = ops.DeviceBuffer(host=src), ops.DeviceBuffer(host=np.zeros((48, 70, 4), np.uint8))
    tensors.resize_bgra([capi.ResizeItem(dsrc.ptr, 280, 0, 0, 70, 48, ddst.ptr, 280, 70, 48)], antialias=filt == AA)
    capi.sync()
    assert np.array_equal(ddst.to_host((48, 70, 4), np.uint8), src)
    # a constant picture stays constant
    const = np.full((1080, 1920, 4), 255, np.uint8)
    dsrc, ddst = ops.DeviceBuffer(host=const), ops.DeviceBuffer(host=np.zeros((224, 224, 4), np.uint8))
    tensors.resize_bgra([capi.ResizeItem(dsrc.ptr, 1920 * 4, 0, 0, 1920, 1080, ddst.ptr, 224 * 4, 224, 224)], antialias=filt == AA)
    capi.sync()
    assert np.all(ddst.to_host((224, 224, 4), np.uint8) == 255)


def mixed_case(seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (48, 340, 4), dtype=np.uint8)
    cases = []
    for k in range(40):
        w, h = int(rng.integers(1, 320)), int(rng.integers(1, 40))
        ow, oh = int(rng.integers(1, 300)), int(rng.integers(1, 50))
        if k % 5 == 0:
            w, ow = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        cases.append((int(rng.integers(0, 340 - w + 1)), int(rng.integers(0, 48 - h + 1)), w, h, ow, oh, int(rng.integers(0, 4))))
    return src, cases


@pytest.mark.parametrize("filt", [BIL, AA])
@pytest.mark.parametrize("own_stream", [False, True])
def test_a_mixed_batch_equals_its_items_alone(filt, own_stream):
    L = capi.lib()
    src, cases = mixed_case(11)
    st = L.ffhip_stream_create() if own_stream else None
    try:
        assert not own_stream or st
        together, exp = run_resize(src, cases, filt, stream=st)
        alone, _ = run_resize(src, cases, filt, stream=st, one_by_one=True)
    finally:
        if st:
            L.ffhip_stream_destroy(st)
    assert np.array_equal(together, alone)
    assert np.array_equal(together, exp)


# ---------------------------------------------------------------------------------------------------- files
def make_format(dtype, planar, bgr, normalise=True):
    name = {U8: "uint8", F16: "float16", F32: "float32"}[dtype]
    chans = slice(None, None, -1) if bgr else slice(None)
    norm = dtype != U8 and normalise
    return tensors.tensor_format(name, "CHW" if planar else "HWC", "BGR" if bgr else "RGB", MEAN[chans] if norm else None, STD[chans] if norm else None)


def expected(bgra, f):
    """numpy's tensor of a [h][w][4] BGRA picture in format f"""
    v = bgra[..., [0, 1, 2] if f.bgr else [2, 1, 0]]
    if f.dtype != U8:
        v = v.astype(np.float32) * np.array(list(f.scale), np.float32) + np.array(list(f.bias), np.float32)
        assert v.dtype == np.float32
        v = v.astype(NP_DTYPE[f.dtype])
    return v.transpose(2, 0, 1) if f.planar else v


class Outputs:
    """One device allocation filled with 0xA5 that holds every tensor at an offset of `off` elements from a 16-byte boundary, with its own
    strides; `exp` is the same memory as numpy expects it after the call."""

    def __init__(self, f, shapes):
        self.f, self.es = f, np.dtype(NP_DTYPE[f.dtype]).itemsize
        self.places, at = [], 0
        for i, (h, w) in enumerate(shapes):
            h, w = max(h, 1), max(w, 1)                                   # (a refused size still gets a place)
            off, extra = (3 * i + 1) % 16, (5 * i) % 4
            rs = (w if f.planar else 3 * w) + extra
            ps = rs * (h - 1) + w + extra if f.planar else 0
            span = 2 * ps + rs * (h - 1) + w if f.planar else rs * (h - 1) + 3 * w
            self.places.append((at + off, rs, ps, h, w))
            at += (off + span + 5 + 15) // 16 * 16
        self.total = max(at, 16)
        self.exp = np.full(self.total * self.es, FILL, np.uint8)
        self.dev = ops.DeviceBuffer(host=self.exp)

    def out(self, k):
        at, rs, ps, _, _ = self.places[k]
        return self.dev.ptr + at * self.es, rs, ps

    def expect(self, k, bgra):
        at, rs, ps, h, w = self.places[k]
        typed, es = self.exp.view(NP_DTYPE[self.f.dtype]), self.es
        view = np.lib.stride_tricks.as_strided(typed[at:], (3, h, w), (ps * es, rs * es, es)) if self.f.planar else \
            np.lib.stride_tricks.as_strided(typed[at:], (h, w, 3), (rs * es, 3 * es, es))
        view[...] = expected(bgra, self.f)

    def read(self):
        return self.dev.to_host((self.total * self.es,), np.uint8)


def check_files(entry, batch, f, filt, sizes, rois=None, expect_bad=(), stream=None, n_threads=4):
    """the resized C file call: sizes[i] = (h, w) of file i's output.  Every delivered tensor equals decode -> numpy rule -> formatting,
    a refused file's output still holds its 0xA5.  stream: the stream of the call (NULL unless given; one that is given is waited for)"""
    files, images, bad = batch
    L, n = capi.lib(), len(files)
    outs = Outputs(f, sizes)
    bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    o = (capi.TensorOut * n)(*[capi.TensorOut(*outs.out(k)) for k in range(n)])
    rects = (capi.Rect * n)(*[capi.Rect(*r) for r in rois]) if rois else None
    out_size = (capi.Size * n)(*[capi.Size(w, h) for h, w in sizes])
    status = (C.c_int * n)()
    rc = getattr(L, entry)(ptrs, lens, n, n_threads, C.byref(f), o, rects, out_size, filt, None, status, stream)
    if stream is not None:
        capi.sync(stream)
    status = list(status)
    for k, img in enumerate(images):
        if k == bad or k in expect_bad:
            assert status[k] != 0, k
            continue
        assert status[k] == 0, k
        x0, y0, w, h = rois[k] if rois else (0, 0, img.shape[1], img.shape[0])
        outs.expect(k, resize_rule(img[y0:y0 + h, x0:x0 + w], sizes[k][0], sizes[k][1], filt))
    assert rc == next(s for s in status if s)                                   # the first failure
    assert np.array_equal(outs.read(), outs.exp)
    return status


@pytest.fixture(scope="module")
def jpeg_batch():
    """files of several layouts and sizes, a truncated one in the middle; their BGRA pictures from the BGRA file call, computed once"""
    capi.require_device(0)
    rng = np.random.default_rng(6)
    spec = [(67, 35, "420", 0), (16, 16, "444", 0), (200, 31, "422", 3), (33, 70, "440", 0), (301, 47, "420", 7), (5, 3, "444", 1)]
    files = [_writer_file(rng, w, h, layout, restart=r)[0] for w, h, layout, r in spec]
    try:
        files += [_pil_file(rng, 333, 211, sub=2), _pil_file(rng, 97, 203, mode="L")]
    except pytest.skip.Exception:
        pass
    bad = len(files) // 2
    files.insert(bad, files[4][:len(files[4]) * 2 // 3])
    _, images, _, status = ops.jpeg_decode_files_mixed_device(files, n_threads=4, strict=False)
    assert status[bad] != 0 and not any(status[:bad] + status[bad + 1:])
    return files, images, bad


@pytest.fixture(scope="module")
def webp_batch():
    capi.require_device(0)
    files = [file_bytes(n) for n in NAMES if n not in UNPINNED]
    bad = len(files) // 2
    files.insert(bad, file_bytes("syn_parts2")[:-5950])                        # truncated inside its last partition
    _, images, _, status = ops.webp_decode_files_device(files, n_threads=4, strict=False)
    assert status[bad] != 0 and not any(status[:bad] + status[bad + 1:])
    return files, images, bad


def display_sizes(images, bad):
    return [(1, 1) if k == bad else img.shape[:2] for k, img in enumerate(images)]


def inner_rois(images, bad):
    return [(0, 0, 1, 1) if k == bad else (1, 2, w - 3, h - 2) if w > 3 and h > 2 else (0, 0, w, h) for k, (h, w) in enumerate(display_sizes(images, bad))]


def per_file_sizes(n):
    return [((7 * k) % 45 + 1, (11 * k) % 70 + 1) for k in range(n)]


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
@pytest.mark.parametrize("dtype,planar,bgr", FORMATS)
def test_files_to_one_size_in_every_format(jpeg_batch, webp_batch, codec, dtype, planar, bgr):
    batch = jpeg_batch if codec == "jpeg" else webp_batch
    check_files(f"ffhip_{codec}_decode_files_tensor_resized", batch, make_format(dtype, planar, bgr), AA, [(32, 32)] * len(batch[0]))


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
@pytest.mark.parametrize("filt", [BIL, AA])
def test_files_with_rectangles_and_sizes_of_their_own(jpeg_batch, webp_batch, codec, filt):
    batch = jpeg_batch if codec == "jpeg" else webp_batch
    entry, f, n = f"ffhip_{codec}_decode_files_tensor_resized", make_format(U8, 1, 0), len(batch[0])
    check_files(entry, batch, f, filt, per_file_sizes(n))
    check_files(entry, batch, f, filt, [(32, 32)] * n, inner_rois(batch[1], batch[2]))
    check_files(entry, batch, f, filt, per_file_sizes(n), inner_rois(batch[1], batch[2]))


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_a_bad_size_and_a_bad_rectangle_are_their_files_alone(jpeg_batch, webp_batch, codec):
    batch = jpeg_batch if codec == "jpeg" else webp_batch
    entry, f, n = f"ffhip_{codec}_decode_files_tensor_resized", make_format(U8, 1, 0), len(batch[0])
    sizes = [(32, 32)] * n
    sizes[0], sizes[1] = (32, 0), (16385, 32)
    rois = inner_rois(batch[1], batch[2])
    h, w = batch[1][n - 1].shape[:2]
    rois[n - 1] = (1, 0, w, h)                                                  # one column too far
    status = check_files(entry, batch, f, AA, sizes, rois, expect_bad=(0, 1, n - 1))
    assert [status[k] for k in (0, 1, n - 1)] == [capi.FFHIP_EINVAL] * 3


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_many_parts_give_the_bytes_of_one_part(jpeg_batch, webp_batch, codec):
    batch = jpeg_batch if codec == "jpeg" else webp_batch
    entry, f, n = f"ffhip_{codec}_decode_files_tensor_resized", make_format(F16, 1, 0), len(batch[0])
    for budget in (200000, 1, None):
        capi.setenv("FFHIP_TENSOR_PART_BYTES", budget)
        check_files(entry, batch, f, AA, per_file_sizes(n))


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_tensors(jpeg_batch, webp_batch):
    import torch
    for decode, (files, images, bad) in ((tensors.decode_jpeg_to_tensors, jpeg_batch), (tensors.decode_webp_to_tensors, webp_batch)):
        good = [k for k in range(len(files)) if k != bad]
        assert len({images[k].shape[:2] for k in good}) > 1
        f = make_format(F16, 1, 0)
        batch = decode([files[k] for k in good], size=(32, 48), stack=True, dtype=torch.float16, mean=MEAN, std=STD)
        assert isinstance(batch, torch.Tensor) and tuple(batch.shape) == (len(good), 3, 32, 48) and batch.is_cuda and batch.dtype == torch.float16
        for i, k in enumerate(good):
            assert np.array_equal(batch[i].cpu().numpy(), expected(resize_rule(images[k], 32, 48, AA), f))
        with pytest.raises(ValueError):
            decode([files[k] for k in good], stack=True)                       # size=None: mixed sizes still do not stack
        with pytest.raises(ValueError):
            decode([files[k] for k in good], size=[(32, 48)] * (len(good) - 1) + [(32, 47)], stack=True)
        with torch.cuda.stream(torch.cuda.Stream()):
            out, status = decode(files, size=(9, 20), antialias=False, layout="HWC", order="BGR", strict=False)
        assert out[bad] is None and status[bad] != 0
        for k in good:
            assert status[k] == 0 and tuple(out[k].shape) == (9, 20, 3) and out[k].dtype == torch.uint8
            assert np.array_equal(out[k].cpu().numpy(), expected(resize_rule(images[k], 9, 20, BIL), make_format(U8, 0, 1)))
        sizes = per_file_sizes(len(good))
        out = decode([files[k] for k in good], size=sizes, roi=[inner_rois(images, bad)[k] for k in good])
        for i, k in enumerate(good):
            x0, y0, w, h = inner_rois(images, bad)[k]
            assert tuple(out[i].shape) == (3,) + sizes[i]
            assert np.array_equal(out[i].cpu().numpy(), expected(resize_rule(images[k][y0:y0 + h, x0:x0 + w], sizes[i][0], sizes[i][1], AA), make_format(U8, 1, 0)))
