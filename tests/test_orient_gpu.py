"""GPU: decoded pictures turned upright.  ffhip_bgra_orient_items for every shape, orientation and placement against the table in numpy
-- exactly, with every byte around the outputs checked untouched --; the oriented file calls against the table applied to what the
existing file calls deliver for the mapped rectangle and size; the torch layer.  No tolerance anywhere: pixels only move."""
import ctypes as C
import itertools

import numpy as np
import pytest

import exif_cases as X
from ffpic_amd import capi, ops, tensors
from test_resize_gpu import FORMATS, NP_DTYPE, Outputs, make_format
from test_webp_front_capi import NAMES, UNPINNED, file_bytes

pytestmark = pytest.mark.gpu

BIL, AA = capi.FFHIP_RESIZE_BILINEAR, capi.FFHIP_RESIZE_ANTIALIAS
U8 = capi.FFHIP_TENSOR_U8
FILL = 0xA5
SIZES = [(1, 1), (1, 7), (7, 1), (3, 200), (63, 65), (64, 64), (65, 63), (130, 67), (257, 129)]       # w x h
AT = (5, 3)


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    capi.setenv("FFHIP_TENSOR_PART_BYTES", None)


# ---------------------------------------------------------------------------------------------------- the stage
@pytest.fixture(scope="module")
def sources():
    """random pictures, alpha random too: per size one that the rectangle fills (pitch 4 x width), and one large one that holds every
    rectangle at (5, 3) with a pitch beyond 4 x its width -> (host pictures, one device buffer, each picture's offset in it)"""
    capi.require_device(0)
    rng = np.random.default_rng(4100)
    pics = {s: rng.integers(0, 256, (s[1], s[0], 4), dtype=np.uint8) for s in SIZES}
    pics["large"] = rng.integers(0, 256, (max(h for _, h in SIZES) + AT[1] + 2, max(w for w, _ in SIZES) + AT[0] + 3, 4), dtype=np.uint8)
    offs, at = {}, 0
    for k, p in pics.items():
        offs[k] = at
        at += (p.nbytes + 255) // 256 * 256
    flat = np.zeros(at, np.uint8)
    for k, p in pics.items():
        flat[offs[k]:offs[k] + p.nbytes] = p.reshape(-1)
    return pics, ops.DeviceBuffer(host=flat), offs


ALL_CASES = [(s, o, placed) for s, o, placed in itertools.product(SIZES, range(1, 9), (False, True))]


def run_orient(sources, cases, stream=None, one_by_one=False):
    """cases (size, orientation, placed at (5, 3) of the large picture?) through ffhip_bgra_orient_items, all outputs in ONE 0xA5-filled
    allocation at pitch 4 x upright width + 12 with 64 bytes of it on either side of each -> (device bytes, expected bytes)"""
    pics, dsrc, offs = sources
    places, at = [], 64
    for (w, h), o, placed in cases:
        uw, uh = X.upright_size(w, h, o)
        pitch = 4 * uw + 12
        places.append((at, pitch, uw, uh))
        at += pitch * (uh - 1) + 4 * uw + 64
    exp = np.full(at, FILL, np.uint8)
    dev = ops.DeviceBuffer(host=exp)
    items = []
    for ((w, h), o, placed), (off, pitch, uw, uh) in zip(cases, places):
        key, (x0, y0) = ("large", AT) if placed else ((w, h), (0, 0))
        items.append(capi.OrientItem(dsrc.ptr + offs[key], pics[key].shape[1] * 4, x0, y0, w, h, dev.ptr + off, pitch, o))
        view = np.lib.stride_tricks.as_strided(exp[off:], (uh, uw, 4), (pitch, 4, 1))
        view[...] = X.orient(pics[key][y0:y0 + h, x0:x0 + w], o)
    for part in ([[it] for it in items] if one_by_one else [items]):
        tensors.orient_bgra(part, stream=stream)
    capi.sync(stream)
    return dev.to_host((exp.size,), np.uint8), exp


@pytest.mark.parametrize("o", range(1, 9))
def test_stage_against_the_table(sources, o):
    """every size, at the origin of its own picture and at (5, 3) of a larger one: the table's pixels inside, 0xA5 in the row padding and
    around every output"""
    for s, placed in itertools.product(SIZES, (False, True)):
        got, exp = run_orient(sources, [(s, o, placed)])
        assert np.array_equal(got, exp), (s, o, placed)


@pytest.mark.parametrize("own_stream", [False, True])
def test_a_mixed_batch_equals_its_items_alone(sources, own_stream):
    L = capi.lib()
    st = L.ffhip_stream_create() if own_stream else None
    try:
        assert not own_stream or st
        together, exp = run_orient(sources, ALL_CASES, stream=st)
        alone, _ = run_orient(sources, ALL_CASES, stream=st, one_by_one=True)
    finally:
        if st:
            L.ffhip_stream_destroy(st)
    assert np.array_equal(together, alone)
    assert np.array_equal(together, exp)


def test_round_trip(sources):
    """orient(o) then orient(inverse(o)): the picture itself"""
    pics, dsrc, offs = sources
    for (w, h), o in itertools.product(SIZES, range(1, 9)):
        uw, uh = X.upright_size(w, h, o)
        mid = ops.DeviceBuffer(host=np.full(4 * uw * uh, FILL, np.uint8))
        back = ops.DeviceBuffer(host=np.full(4 * w * h, FILL, np.uint8))
        tensors.orient_bgra([capi.OrientItem(dsrc.ptr + offs[(w, h)], 4 * w, 0, 0, w, h, mid.ptr, 4 * uw, o)])
        tensors.orient_bgra([capi.OrientItem(mid.ptr, 4 * uw, 0, 0, uw, uh, back.ptr, 4 * w, ops.orient_inverse(o))])
        capi.sync()
        assert np.array_equal(back.to_host((h, w, 4), np.uint8), pics[(w, h)]), (w, h, o)


# ---------------------------------------------------------------------------------------------------- files
class Batch:
    """files with their stored display sizes (w, h) and the orientation each carries (0: a file no probe takes)"""

    def __init__(self, codec, files, sizes, tags):
        self.codec, self.files, self.sizes, self.tags = codec, files, sizes, tags
        self.bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
        n = len(files)
        self.ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.lens = (C.c_size_t * n)(*[b.size for b in self.bufs])


def ints(values):
    return None if values is None else (C.c_int * len(values))(*values)


def tensor_view(outs, raw, k):
    at, rs, ps, h, w = outs.places[k]
    typed, es = raw.view(NP_DTYPE[outs.f.dtype]), outs.es
    if outs.f.planar:
        return np.lib.stride_tricks.as_strided(typed[at:], (3, h, w), (ps * es, rs * es, es))
    return np.lib.stride_tricks.as_strided(typed[at:], (h, w, 3), (rs * es, 3 * es, es))


def existing_call(b, f, shapes, rois, sizes, filt, denom):
    """the call without orientation that fits the arguments -> (tensors as numpy [h][w][3] (None: refused), status, denominators used)"""
    L, n = capi.lib(), len(b.files)
    outs = Outputs(f, shapes)
    o = (capi.TensorOut * n)(*[capi.TensorOut(*outs.out(k)) for k in range(n)])
    rects = (capi.Rect * n)(*[capi.Rect(*r) for r in rois]) if rois else None
    out_size = (capi.Size * n)(*[capi.Size(w, h) for h, w in sizes]) if sizes else None
    status, used = (C.c_int * n)(), (C.c_int * n)(*([1] * n))
    head = (b.ptrs, b.lens, n, 4, C.byref(f), o, rects)
    if denom is not None:
        L.ffhip_jpeg_decode_files_tensor_scaled(*head, out_size, filt, ints(denom), used, None, status, None)
    elif sizes:
        getattr(L, f"ffhip_{b.codec}_decode_files_tensor_resized")(*head, out_size, filt, None, status, None)
    else:
        getattr(L, f"ffhip_{b.codec}_decode_files_tensor")(*head, None, status, None)
    raw = outs.read()
    got = []
    for k in range(n):
        t = None if status[k] else tensor_view(outs, raw, k).copy()
        got.append(t if t is None or not f.planar else t.transpose(1, 2, 0))
    return got, list(status), list(used), raw


def oriented_call(b, f, shapes, rois, sizes, filt, denom, orient):
    L, n = capi.lib(), len(b.files)
    outs = Outputs(f, shapes)
    o = (capi.TensorOut * n)(*[capi.TensorOut(*outs.out(k)) for k in range(n)])
    rects = (capi.Rect * n)(*[capi.Rect(*r) for r in rois]) if rois else None
    out_size = (capi.Size * n)(*[capi.Size(w, h) for h, w in sizes]) if sizes else None
    status, used, turned = (C.c_int * n)(), (C.c_int * n)(*([-1] * n)), (C.c_int * n)(*([-1] * n))
    head = (b.ptrs, b.lens, n, 4, C.byref(f), o, rects, out_size, filt)
    if b.codec == "jpeg":
        rc = L.ffhip_jpeg_decode_files_tensor_oriented(*head, ints(denom), used, ints(orient), turned, None, status, None)
    else:
        rc = L.ffhip_webp_decode_files_tensor_oriented(*head, ints(orient), turned, None, status, None)
    return outs, rc, list(status), list(used), list(turned)


def check_oriented(b, f=None, roi=None, size=None, filt=AA, denom=None, orient=None, bad=()):
    """The oriented call with UPRIGHT arguments against the table applied to the existing call's output for the mapped ones.
    roi: a function (upright w, h) -> upright rectangle; size: the upright (h, w) for every file; denom: one value for every file.
    bad: files expected to fail (with any code); their outputs keep their 0xA5.  Returns what the oriented call reported."""
    f = f or make_format(U8, 0, 0)
    n = len(b.files)
    eff = [b.tags[k] if orient is None or orient[k] == 0 else orient[k] for k in range(n)]          # the orientation that counts
    eff = [e or 1 for e in eff]
    up = [X.upright_size(w, h, eff[k]) for k, (w, h) in enumerate(b.sizes)]
    up_rois = [roi(*up[k]) for k in range(n)] if roi else None
    st_rois = [X.stored_rect(*b.sizes[k], eff[k], up_rois[k]) if k not in bad else (0, 0, 1, 1) for k in range(n)] if roi else None
    st_sizes = [size[::-1] if eff[k] >= 5 else size for k in range(n)] if size else None
    den = None if denom is None else [denom] * n
    # the shapes of the stored results
    st_shapes = []
    for k, (w, h) in enumerate(b.sizes):
        if st_sizes:
            st_shapes.append(st_sizes[k])
            continue
        r = st_rois[k] if st_rois else (0, 0, w, h)
        if den and den[k] > 1:
            r = ops.jpeg_scaled_rect(w, h, den[k], r)
        st_shapes.append((r[3], r[2]))
    ref, ref_status, ref_used, _ = existing_call(b, f, st_shapes, st_rois, st_sizes, filt, den)
    shapes = [s[::-1] if eff[k] >= 5 else s for k, s in enumerate(st_shapes)]
    outs, rc, status, used, turned = oriented_call(b, f, shapes, up_rois, [size] * n if size else None, filt, den, orient)
    raw = outs.read()
    for k in range(n):
        if k in bad or b.tags[k] == 0:
            assert status[k] != 0, k
            continue
        assert status[k] == 0 and ref_status[k] == 0, (k, status[k], ref_status[k])
        t = X.orient(ref[k], eff[k])
        tensor_view(outs, outs.exp, k)[...] = t.transpose(2, 0, 1) if f.planar else t
        if den:
            assert used[k] == ref_used[k], k
    assert np.array_equal(raw, outs.exp)
    assert rc == next((s for s in status if s), 0)
    assert turned == [0 if b.tags[k] == 0 else eff[k] for k in range(n)]
    assert ops.orient_last_items() == sum(1 for k in range(n) if status[k] == 0 and eff[k] != 1)
    return status, used, turned


@pytest.fixture(scope="module")
def jpeg_base():
    rng = np.random.default_rng(4200)
    spec = [(37, 23, "420"), (37, 23, "444"), (37, 23, "grey"), (100, 75, "420"), (100, 75, "444"), (100, 75, "grey"), (640, 480, "420")]
    return [(X.writer_jpeg(rng, w, h, layout), (w, h)) for w, h, layout in spec]


@pytest.fixture(scope="module")
def jpeg_tagged(jpeg_base):
    """every file under every tag, in alternating byte orders and types"""
    files, sizes, tags = [], [], []
    for (data, size), o in itertools.product(jpeg_base, range(1, 9)):
        files.append(X.tagged_jpeg(data, o, big_endian=bool(o & 1), kind=X.LONG if o & 2 else X.SHORT))
        sizes.append(size)
        tags.append(o)
    return Batch("jpeg", files, sizes, tags)


@pytest.fixture(scope="module")
def webp_tagged():
    names = [n for n in NAMES if n not in UNPINNED]
    files, sizes, tags = [], [], []
    for k, name in enumerate(names + ["pil_50x48_q30"] * 8):
        data = file_bytes(name)
        w, h, c, r = ops.webp_probe(data)
        o = k % 8 + 1
        files.append(X.tagged_webp(data, o, exif_prefix=bool(k & 1), big_endian=bool(k & 2), kind=X.LONG if k & 4 else X.SHORT))
        sizes.append((min(w, 16 * c), min(h, 16 * r)))
        tags.append(o)
    return Batch("webp", files, sizes, tags)


def inner(uw, uh):
    return (1, 2, uw - 3, uh - 2) if uw > 3 and uh > 2 else (0, 0, uw, uh)


def batch_of(request, codec):
    return request.getfixturevalue(f"{codec}_tagged")


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_files_whole_and_inner_rectangle(request, codec):
    b = batch_of(request, codec)
    status, used, turned = check_oriented(b)
    assert turned == b.tags and not any(status)
    check_oriented(b, roi=inner)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
@pytest.mark.parametrize("filt", [BIL, AA])
def test_files_resized_to_an_upright_size(request, codec, filt):
    """48 wide x 80 high in upright axes: 80 x 48 in the stored axes of the files that are turned by a quarter"""
    b = batch_of(request, codec)
    check_oriented(b, size=(80, 48), filt=filt)
    check_oriented(b, size=(80, 48), filt=filt, roi=inner)
    check_oriented(b, size=(32, 32), filt=filt)


def test_jpeg_files_at_reduced_size(jpeg_tagged):
    b = jpeg_tagged
    check_oriented(b, denom=2)
    check_oriented(b, denom=2, roi=inner)
    check_oriented(b, denom=2, size=(80, 48))
    status, used, _ = check_oriented(b, denom=0, size=(80, 48))
    assert set(used) > {1}                                                   # "auto" chose something for the larger files
    check_oriented(b, denom=0, size=(20, 12), roi=inner)
    check_oriented(b, denom=1)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
@pytest.mark.parametrize("dtype,planar,bgr", [fmt for fmt in FORMATS if fmt != (U8, 0, 0)])
def test_files_in_the_other_formats(request, codec, dtype, planar, bgr):
    check_oriented(batch_of(request, codec), f=make_format(dtype, planar, bgr), size=(80, 48), roi=inner)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_an_imposed_orientation_overrides_the_tag(request, codec):
    b = batch_of(request, codec)
    n = len(b.files)
    status, used, turned = check_oriented(b, orient=[(3 * k) % 9 for k in range(n)], size=(80, 48))     # 0: the tag after all
    assert turned == [(3 * k) % 9 or b.tags[k] for k in range(n)]
    check_oriented(b, orient=[8 - (k % 8) for k in range(n)], roi=inner)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_all_1_and_untagged_batches_give_the_bytes_of_the_existing_calls(request, codec, jpeg_base):
    b = batch_of(request, codec)
    n = len(b.files)
    if codec == "jpeg":
        plain = Batch("jpeg", [d for d, _ in jpeg_base], [s for _, s in jpeg_base], [1] * len(jpeg_base))
    else:
        names = [m for m in NAMES if m not in UNPINNED]
        plain = Batch("webp", [file_bytes(m) for m in names], b.sizes[:len(names)], [1] * len(names))
    f = make_format(U8, 0, 0)
    for batch, orient in ((b, [1] * n), (plain, None)):
        m = len(batch.files)
        for rois, sizes, denom in ((None, None, None), ([inner(w, h) for w, h in batch.sizes], [(33, 20)] * m, None), (None, [(33, 20)] * m, 0 if codec == "jpeg" else None)):
            shapes = sizes or [(h, w) for w, h in batch.sizes]
            den = None if denom is None else [denom] * m
            _, ref_status, ref_used, ref_raw = existing_call(batch, f, shapes, rois, sizes, AA, den)
            outs, rc, status, used, turned = oriented_call(batch, f, shapes, rois, sizes, AA, den, orient)
            assert rc == 0 and status == ref_status == [0] * m and turned == [1] * m
            assert np.array_equal(outs.read(), ref_raw)
            assert ops.orient_last_items() == 0
            if den:
                assert used == ref_used


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_a_damaged_file_and_a_bad_upright_rectangle_are_their_files_alone(request, codec):
    b = batch_of(request, codec)
    files, sizes, tags = list(b.files[:12]), list(b.sizes[:12]), list(b.tags[:12])
    files[4], tags[4] = files[4][:len(files[4]) * 2 // 3 if codec == "jpeg" else 30], 0        # truncated: inside the scan / inside the frame header
    damaged = Batch(codec, files, sizes, tags)
    # file 5 (turned by a quarter, not square): the STORED picture's rectangle does not fit the upright picture
    assert tags[5] >= 5 and sizes[5][0] != sizes[5][1]
    n = 12
    f = make_format(U8, 0, 0)
    eff = [t or 1 for t in tags]
    up = [X.upright_size(*sizes[k], eff[k]) for k in range(n)]
    up_rois = [(0, 0, up[k][1], up[k][0]) if k == 5 else inner(*up[k]) for k in range(n)]
    shapes = [(r[3], r[2]) for r in up_rois]
    outs, rc, status, used, turned = oriented_call(damaged, f, shapes, up_rois, None, AA, None, None)
    assert ops.orient_last_items() == sum(1 for k in range(n) if k not in (4, 5) and eff[k] != 1)
    assert status[5] == capi.FFHIP_EINVAL and status[4] != 0 and not any(status[k] for k in range(n) if k not in (4, 5))
    assert rc == status[4]
    # the others: what the intact batch gives them
    st_rois = [X.stored_rect(*sizes[k], eff[k], up_rois[k]) if k != 5 else (0, 0, 1, 1) for k in range(n)]
    intact = Batch(codec, list(b.files[:12]), sizes, list(b.tags[:12]))
    ref, ref_status, _, _ = existing_call(intact, f, [(r[3], r[2]) for r in st_rois], st_rois, None, AA, None)
    for k in range(n):
        if k not in (4, 5):
            tensor_view(outs, outs.exp, k)[...] = X.orient(ref[k], eff[k])
    assert np.array_equal(outs.read(), outs.exp)


@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_many_parts_give_the_bytes_of_one_part(request, codec):
    b = batch_of(request, codec)
    for budget in (200000, 1, None):
        capi.setenv("FFHIP_TENSOR_PART_BYTES", budget)
        check_oriented(b, roi=inner)
        parts = ops.tensor_last_parts()
        assert parts == (len(b.files) if budget == 1 else parts) and (parts > 1) == (budget is not None)
        check_oriented(b, size=(80, 48))


# ---------------------------------------------------------------------------------------------------- torch
@pytest.mark.parametrize("codec", ["jpeg", "webp"])
def test_torch_tensors(request, codec):
    import torch
    b = batch_of(request, codec)
    decode = tensors.decode_jpeg_to_tensors if codec == "jpeg" else tensors.decode_webp_to_tensors
    plain = decode(b.files)                                                     # the defaults: today's result, the tag ignored
    for k, t in enumerate(plain):
        assert tuple(t.shape) == (3, b.sizes[k][1], b.sizes[k][0])
    up, turned = decode(b.files, apply_exif_orientation=True, return_orientation=True)
    assert turned == b.tags
    for k, t in enumerate(up):
        uw, uh = X.upright_size(*b.sizes[k], b.tags[k])
        assert tuple(t.shape) == (3, uh, uw) and t.is_cuda and t.dtype == torch.uint8
        assert np.array_equal(t.cpu().numpy().transpose(1, 2, 0), X.orient(plain[k].cpu().numpy().transpose(1, 2, 0), b.tags[k]))
    assert len({tuple(t.shape) for t in up}) > 1 and {o >= 5 for o in b.tags} == {False, True}      # landscape and portrait together
    batch = decode(b.files, apply_exif_orientation=True, size=(64, 48), stack=True)
    assert isinstance(batch, torch.Tensor) and tuple(batch.shape) == (len(b.files), 3, 64, 48)
    for k in range(0, len(b.files), 5):
        alone = decode([b.files[k]], apply_exif_orientation=True, size=(64, 48))[0]
        assert torch.equal(batch[k], alone)
        stored = decode([b.files[k]], size=(48, 64) if b.tags[k] >= 5 else (64, 48))[0]
        assert np.array_equal(alone.cpu().numpy().transpose(1, 2, 0), X.orient(stored.cpu().numpy().transpose(1, 2, 0), b.tags[k]))
    # an imposed orientation, a rectangle in upright axes, HWC
    out, turned = decode(b.files[:8], orientation=6, roi=(1, 2, 5, 7), layout="HWC", return_orientation=True)
    assert turned == [6] * 8
    for k, t in enumerate(out):
        assert tuple(t.shape) == (7, 5, 3)
        assert np.array_equal(t.cpu().numpy(), X.orient(plain[k].cpu().numpy().transpose(1, 2, 0), 6)[2:9, 1:6])
    if codec == "jpeg":
        out, used, turned = decode(b.files[-8:], apply_exif_orientation=True, reduce=2, return_reduce=True, return_orientation=True)
        assert used == [2] * 8 and turned == b.tags[-8:]
        for k, t in enumerate(out):
            uw, uh = X.upright_size(320, 240, b.tags[len(b.files) - 8 + k])
            assert tuple(t.shape) == (3, uh, uw)
