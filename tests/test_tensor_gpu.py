"""GPU: decoded pictures into tensors.  ffhip_bgra_to_tensor_items at every alignment of its destination, in all twelve formats, against
numpy -- exactly, with every byte around the outputs checked untouched --; the file calls against the BGRA file calls underneath; the
torch layer.  No tolerance anywhere: the uint8 path is a permutation, the float path is byte * scale + bias with both roundings."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ffpic_amd import capi, ops, tensors
from test_jpeg_mixed_gpu import _pil_file, _writer_file
from test_webp_front_capi import NAMES, UNPINNED, file_bytes

pytestmark = pytest.mark.gpu

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
    """One device allocation filled with 0xA5 that holds every output at an offset of `off` elements from a 16-byte boundary, with its own
    strides; `exp` is the same memory as numpy expects it after the call."""

    def __init__(self, f, shapes, offs, extras):
        self.f, self.es = f, np.dtype(NP_DTYPE[f.dtype]).itemsize
        self.places, at = [], 0
        for (h, w), off, extra in zip(shapes, offs, extras):
            rs = (w if f.planar else 3 * w) + extra
            ps = rs * (h - 1) + w + extra if f.planar else 0
            span = 2 * ps + rs * (h - 1) + w if f.planar else rs * (h - 1) + 3 * w
            self.places.append((at + off, rs, ps, h, w))
            at += (off + span + 5 + 15) // 16 * 16                       # elements; the next output starts on a 16-byte boundary again
        self.total = max(at, 16)
        self.exp = np.full(self.total * self.es, FILL, np.uint8)
        self.dev = ops.DeviceBuffer(host=self.exp)

    def out(self, k):
        at, rs, ps, _, _ = self.places[k]
        return self.dev.ptr + at * self.es, rs, ps

    def expect(self, k, bgra):
        at, rs, ps, h, w = self.places[k]
        typed = self.exp.view(NP_DTYPE[self.f.dtype])
        es = self.es
        view = np.lib.stride_tricks.as_strided(typed[at:], (3, h, w), (ps * es, rs * es, es)) if self.f.planar else \
            np.lib.stride_tricks.as_strided(typed[at:], (h, w, 3), (rs * es, 3 * es, es))
        view[...] = expected(bgra, self.f)

    def read(self):
        return self.dev.to_host((self.total * self.es,), np.uint8)

    def view(self, k, flat):
        """output k inside `flat`, the allocation's bytes (read(), or exp): [3][h][w] or [h][w][3]"""
        at, rs, ps, h, w = self.places[k]
        typed, es = flat.view(NP_DTYPE[self.f.dtype]), self.es
        return np.lib.stride_tricks.as_strided(typed[at:], (3, h, w) if self.f.planar else (h, w, 3), (ps * es, rs * es, es) if self.f.planar else (rs * es, 3 * es, es))


def run_items(f, src, rects, offs, extras, stream=None, one_by_one=False):
    """rectangles (x0, y0, w, h) of the host picture `src` [H][W][4] through ffhip_bgra_to_tensor_items -> (device bytes, expected bytes)"""
    dsrc = ops.DeviceBuffer(host=np.ascontiguousarray(src))
    outs = Outputs(f, [(h, w) for _, _, w, h in rects], offs, extras)
    items = []
    for k, (x0, y0, w, h) in enumerate(rects):
        ptr, rs, ps = outs.out(k)
        items.append(capi.TensorItem(dsrc.ptr, src.shape[1] * 4, x0, y0, w, h, ptr, rs, ps))
        outs.expect(k, src[y0:y0 + h, x0:x0 + w])
    for part in ([[it] for it in items] if one_by_one else [items]):
        tensors.bgra_to_tensors(part, f, stream)
    capi.sync(stream)
    return outs.read(), outs.exp


# ---------------------------------------------------------------------------------------------------- 1. every alignment
WIDTHS = (1, 2, 3, 4, 5, 7, 13, 16, 17, 63, 64, 65, 67, 255, 257)
HEIGHTS = (1, 2, 3, 17)
X0S = (0, 1, 2, 3, 5)


@pytest.mark.parametrize("dtype,planar,bgr", FORMATS)
def test_every_alignment_every_format(dtype, planar, bgr):
    """every width x height x x0 x output offset x row stride in ONE call per format: inside equals numpy, outside is still 0xA5"""
    rng = np.random.default_rng(1000 + 100 * dtype + 10 * planar + bgr)
    src = rng.integers(0, 256, (max(HEIGHTS) + 3, max(WIDTHS) + max(X0S), 4), dtype=np.uint8)       # alpha random too
    cases = list(itertools.product(WIDTHS, HEIGHTS, X0S, (0, 1, 2, 3), (0, 1, 3)))
    rects = [(x0, (w + x0) % 4, w, h) for w, h, x0, _, _ in cases]
    got, exp = run_items(make_format(dtype, planar, bgr), src, rects, [c[3] for c in cases], [c[4] for c in cases])
    assert np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------------- 2. every byte value
@pytest.mark.parametrize("dtype,planar", [(F32, 1), (F32, 0), (F16, 1), (F16, 0)])
@pytest.mark.parametrize("norm", ["imagenet", "1/255", "bytes"])
def test_all_byte_values_in_every_channel(dtype, planar, norm):
    src = np.zeros((2, 256, 4), np.uint8)
    for c in range(3):
        src[0, :, c] = (np.arange(256) + 37 * c) % 256
        src[1, :, c] = (255 - np.arange(256) + 91 * c) % 256
    src[..., 3] = np.arange(256) * 7 % 256
    f = make_format(dtype, planar, 0, normalise=norm == "imagenet")
    if norm == "1/255":
        for c in range(3):
            f.scale[c] = 1.0 / 255.0
    got, exp = run_items(f, src, [(0, 0, 256, 2)], [1], [2])
    assert np.array_equal(got, exp)
    assert len(np.unique(exp.view(NP_DTYPE[dtype]))) >= 256


# ---------------------------------------------------------------------------------------------------- 3. mixed batches
def mixed_case(seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (48, 340, 4), dtype=np.uint8)
    rects = []
    for k in range(40):
        w, h = int(rng.integers(1, 320)), int(rng.integers(1, 40))
        if k % 5 == 0:
            w = int(rng.integers(1, 20))
        rects.append((int(rng.integers(0, 340 - w + 1)), int(rng.integers(0, 48 - h + 1)), w, h))
    return src, rects, [int(v) for v in rng.integers(0, 16, 40)], [int(v) for v in rng.integers(0, 9, 40)]


@pytest.mark.parametrize("dtype,planar,bgr", [(U8, 1, 0), (U8, 0, 1), (F16, 1, 1), (F16, 0, 0), (F32, 1, 0), (F32, 0, 1)])
@pytest.mark.parametrize("own_stream", [False, True])
def test_a_mixed_batch_equals_its_items_alone(dtype, planar, bgr, own_stream):
    L = capi.lib()
    src, rects, offs, extras = mixed_case(7)
    f = make_format(dtype, planar, bgr)
    st = L.ffhip_stream_create() if own_stream else None
    try:
        assert not own_stream or st
        together, exp = run_items(f, src, rects, offs, extras, stream=st)
        alone, _ = run_items(f, src, rects, offs, extras, stream=st, one_by_one=True)
    finally:
        if st:
            L.ffhip_stream_destroy(st)
    assert np.array_equal(together, alone)
    assert np.array_equal(together, exp)


# ---------------------------------------------------------------------------------------------------- 4 - 6. files
def files_to_tensors(entry, files, sizes, f, rois=None, n_threads=4):
    """the C file call into one 0xA5-filled allocation; sizes[i] = (h, w) of file i's output -> (status, Outputs, return code)"""
    L = capi.lib()
    n = len(files)
    outs = Outputs(f, sizes, [(3 * i + 1) % 16 for i in range(n)], [(5 * i) % 4 for i in range(n)])
    bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    o = (capi.TensorOut * n)(*[capi.TensorOut(*outs.out(k)) for k in range(n)])
    rects = (capi.Rect * n)(*[capi.Rect(*r) for r in rois]) if rois else None
    status = (C.c_int * n)()
    rc = getattr(L, entry)(ptrs, lens, n, n_threads, C.byref(f), o, rects, None, status, None)
    return list(status), outs, rc


FILE_FORMATS = [(U8, 1, 0), (U8, 0, 0), (F16, 0, 1), (F32, 1, 1)]


@pytest.fixture(scope="module")
def jpeg_batch():
    """files of several layouts and sizes, with and without restart markers, a truncated one in the middle; their BGRA pictures (display
    size) from the BGRA file call, computed once"""
    capi.require_device(0)
    rng = np.random.default_rng(5)
    spec = [(67, 35, "420", 0), (16, 16, "444", 0), (200, 31, "422", 3), (33, 70, "440", 0), (129, 9, "h4v1", 2), (40, 40, "grey", 0),
            (301, 47, "420", 7), (5, 3, "444", 1), (96, 64, "h1v4", 0)]
    files = [_writer_file(rng, w, h, layout, restart=r)[0] for w, h, layout, r in spec]
    try:
        files += [_pil_file(rng, 333, 211, sub=2), _pil_file(rng, 127, 65, sub=0), _pil_file(rng, 97, 203, mode="L")]
    except pytest.skip.Exception:
        pass
    bad = len(files) // 2
    files.insert(bad, files[6][:len(files[6]) * 2 // 3])
    _, images, _, status = ops.jpeg_decode_files_mixed_device(files, n_threads=4, strict=False)
    assert status[bad] != 0 and not any(status[:bad] + status[bad + 1:])
    sizes = [(h, w) for _, w, h in (ops.jpeg_probe(d) for d in files)]
    return files, images, sizes, bad


def check_files(entry, files, images, sizes, bad, f, rois=None, expect_bad=()):
    if rois:
        sizes = [(r[3], r[2]) for r in rois]
    status, outs, rc = files_to_tensors(entry, files, sizes, f, rois)
    for k, img in enumerate(images):
        if k == bad or k in expect_bad:
            assert status[k] != 0, k
            continue
        assert status[k] == 0, k
        x0, y0, w, h = rois[k] if rois else (0, 0, img.shape[1], img.shape[0])
        outs.expect(k, img[y0:y0 + h, x0:x0 + w])
    assert rc == next(s for s in status if s)                                   # the first failure
    assert np.array_equal(outs.read(), outs.exp)                               # a failed file's output still holds its 0xA5
    return status


@pytest.mark.parametrize("dtype,planar,bgr", FILE_FORMATS)
def test_jpeg_files_equal_the_bgra_call(jpeg_batch, dtype, planar, bgr):
    files, images, sizes, bad = jpeg_batch
    check_files("ffhip_jpeg_decode_files_tensor", files, images, sizes, bad, make_format(dtype, planar, bgr))


def inner_rois(sizes):
    return [(1, 2, w - 3, h - 2) if w > 3 and h > 2 else (0, 0, w, h) for h, w in sizes]


def test_jpeg_rectangles_inside_and_outside(jpeg_batch):
    files, images, sizes, bad = jpeg_batch
    rois = inner_rois(sizes)
    check_files("ffhip_jpeg_decode_files_tensor", files, images, sizes, bad, make_format(U8, 1, 0), rois)
    h0, w0 = sizes[0]
    rois[0] = (1, 0, w0, h0)                                                    # one column too far
    rois[2] = (0, sizes[2][0] - 1, 4, 2)                                        # one row too far
    rois[3] = (-1, 0, 4, 4)
    status = check_files("ffhip_jpeg_decode_files_tensor", files, images, sizes, bad, make_format(F16, 0, 0), rois, expect_bad=(0, 2, 3))
    assert [status[k] for k in (0, 2, 3)] == [capi.FFHIP_EINVAL] * 3


@pytest.fixture(scope="module")
def webp_batch():
    capi.require_device(0)
    names = [n for n in NAMES if n not in UNPINNED]
    files = [file_bytes(n) for n in names]
    bad = len(files) // 2
    files.insert(bad, file_bytes("syn_parts2")[:-5950])                        # truncated inside its last partition
    _, images, _, status = ops.webp_decode_files_device(files, n_threads=4, strict=False)
    assert status[bad] != 0 and not any(status[:bad] + status[bad + 1:])
    sizes = []
    for d in files:
        w, h, c, r = ops.webp_probe(d)
        sizes.append((min(h, 16 * r), min(w, 16 * c)))
    for img, s in zip(images, sizes):
        assert img is None or img.shape[:2] == s
    return files, images, sizes, bad


@pytest.mark.parametrize("dtype,planar,bgr", FILE_FORMATS)
def test_webp_files_equal_the_bgra_call(webp_batch, dtype, planar, bgr):
    files, images, sizes, bad = webp_batch
    check_files("ffhip_webp_decode_files_tensor", files, images, sizes, bad, make_format(dtype, planar, bgr))


def test_webp_rectangles_inside_and_outside(webp_batch):
    files, images, sizes, bad = webp_batch
    rois = inner_rois(sizes)
    check_files("ffhip_webp_decode_files_tensor", files, images, sizes, bad, make_format(F32, 0, 1), rois)
    rois[1] = (0, 0, sizes[1][1] + 1, sizes[1][0])
    status = check_files("ffhip_webp_decode_files_tensor", files, images, sizes, bad, make_format(U8, 0, 0), rois, expect_bad=(1,))
    assert status[1] == capi.FFHIP_EINVAL


def parts_of(coded_bytes, budget):
    """the parts the file calls cut a batch into: files while their pictures fit the budget, at least one"""
    parts, cur = 0, None
    for b in coded_bytes:
        b = (b + 255) // 256 * 256
        if cur is None or cur + b > budget:
            parts, cur = parts + 1, 0
        cur += b
    return parts


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_many_parts_give_the_bytes_of_one_part(jpeg_batch, webp_batch, codec):
    files, images, sizes, bad = jpeg_batch if codec == "jpeg" else webp_batch
    pick = [k for k in range(len(files)) if k != bad][:5]
    pick.insert(2, bad)                                                         # six files, the damaged one among them
    files, images, sizes = [files[k] for k in pick], [images[k] for k in pick], [sizes[k] for k in pick]
    if codec == "jpeg":
        coded = [g.width * g.height * 4 for g, _, _ in (ops.jpeg_probe(d) for d in files)]
    else:
        coded = [64 * c * 16 * r for _, _, c, r in (ops.webp_probe(d) for d in files)]
    entry = f"ffhip_{codec}_decode_files_tensor"
    f = make_format(F16, 1, 0)
    assert parts_of(coded, 1 << 30) == 1
    for budget in (sorted(coded)[3] + sorted(coded)[0], 1):
        assert parts_of(coded, budget) >= 3
        capi.setenv("FFHIP_TENSOR_PART_BYTES", budget)
        check_files(entry, files, images, sizes, 2, f)
    capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    check_files(entry, files, images, sizes, 2, f)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_a_damaged_file_with_a_bad_rectangle_keeps_the_decoders_code(webp_batch, codec):
    """Whose code a file gets: the decoder's comes before this call's own.  File 1 is truncated inside its scan AND has a rectangle that
    leaves its picture; file 2 is intact with such a rectangle; files 0 and 3 are delivered as in a call of their own.  One part, and a
    part per file"""
    if codec == "jpeg":
        rng = np.random.default_rng(11)
        files = [_writer_file(rng, w, h, layout)[0] for w, h, layout in ((37, 23, "420"), (100, 75, "444"), (100, 75, "420"), (37, 23, "444"))]
        files[1] = files[1][:len(files[1]) * 2 // 3]
        sizes = [(h, w) for _, w, h in (ops.jpeg_probe(d) for d in files)]
    else:
        all_files, _, all_sizes, bad = webp_batch
        pick = [k for k in range(len(all_files)) if k != bad][:3]
        pick.insert(1, bad)
        files, sizes = [all_files[k] for k in pick], [all_sizes[k] for k in pick]
    entry, f = f"ffhip_{codec}_decode_files_tensor", make_format(F16, 1, 0)
    good = inner_rois(sizes)
    rois = list(good)
    rois[1] = (1, 0, sizes[1][1], sizes[1][0])                                  # one column too far
    rois[2] = (0, sizes[2][0] - 1, 4, 2)                                        # one row too far
    shapes = [(r[3], r[2]) for r in rois]
    ref_status, _, ref_rc = files_to_tensors(entry, files, [(r[3], r[2]) for r in good], f, good)
    assert ref_status[1] != 0 and ref_rc == ref_status[1] and not any(ref_status[k] for k in (0, 2, 3))
    alone = {}
    for k in (0, 3):
        status, outs, rc = files_to_tensors(entry, [files[k]], [shapes[k]], f, [rois[k]])
        assert rc == 0 and status == [0]
        alone[k] = outs.view(0, outs.read()).copy()
    for budget, parts in ((None, 1), (1, 4)):
        capi.setenv("FFHIP_TENSOR_PART_BYTES", budget)
        status, outs, rc = files_to_tensors(entry, files, shapes, f, rois)
        assert ops.tensor_last_parts() == parts
        assert status == [0, ref_status[1], capi.FFHIP_EINVAL, 0] and rc == status[1]
        for k in (0, 3):
            outs.view(k, outs.exp)[...] = alone[k]
        assert np.array_equal(outs.read(), outs.exp)                           # outputs 1 and 2 and every byte around still hold 0xA5


# ---------------------------------------------------------------------------------------------------- 7. torch
def test_torch_tensors(jpeg_batch, webp_batch):
    import torch
    for decode, (files, images, sizes, bad) in ((tensors.decode_jpeg_to_tensors, jpeg_batch), (tensors.decode_webp_to_tensors, webp_batch)):
        good = [k for k in range(len(files)) if k != bad]
        out = decode([files[k] for k in good])
        for k, t in zip(good, out):
            ref = torch.from_numpy(images[k].copy())[..., [2, 1, 0]].permute(2, 0, 1)
            assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (3,) + sizes[k]
            assert torch.equal(t.cpu(), ref)
        # float forms, a damaged file, an own stream
        f = make_format(F16, 0, 1)
        with torch.cuda.stream(torch.cuda.Stream()):
            out, status = decode(files, dtype=torch.float16, layout="HWC", order="BGR", mean=MEAN[::-1], std=STD[::-1], strict=False)
        assert out[bad] is None and status[bad] != 0
        for k in good:
            assert out[k].dtype == torch.float16 and tuple(out[k].shape) == sizes[k] + (3,) and out[k].device.type == "cuda"
            assert np.array_equal(out[k].cpu().numpy(), expected(images[k], f))
        with pytest.raises(capi.FfhipError):
            decode(files)
        out = decode([files[good[0]]], dtype=torch.float32)
        assert out[0].dtype == torch.float32 and torch.equal(out[0].cpu(), torch.from_numpy(images[good[0]].copy())[..., [2, 1, 0]].permute(2, 0, 1).float())
        # stack: one tensor when the sizes agree
        same = [files[good[1]]] * 3
        for layout, shape in (("CHW", (3, 3) + sizes[good[1]]), ("HWC", (3,) + sizes[good[1]] + (3,))):
            batch = decode(same, dtype=torch.float32, layout=layout, mean=MEAN, std=STD, stack=True)
            assert isinstance(batch, torch.Tensor) and tuple(batch.shape) == shape and batch.is_cuda and batch.is_contiguous()
            f32 = make_format(F32, layout == "CHW", 0)
            for i in range(3):
                assert np.array_equal(batch[i].cpu().numpy(), expected(images[good[1]], f32))
        with pytest.raises(ValueError):
            decode([files[good[0]], files[good[1]]], stack=True)
        roi = (1, 1, 4, 3)
        out = decode([files[good[0]], files[good[2]]], roi=roi, stack=True)
        assert tuple(out.shape) == (2, 3, 3, 4)
        for i, k in enumerate((good[0], good[2])):
            assert np.array_equal(out[i].cpu().numpy(), expected(images[k][1:4, 1:5], make_format(U8, 1, 0)))
