"""GPU: libjpeg's pixel rule on the device (ffhip_jpeg_recon_items_libjpeg, FFHIP_JPEG_PIXELS_LIBJPEG on the file calls, pixels="libjpeg" in
Python).  The items call is held to the host function ffhip_jpeg_libjpeg_picture bit for bit -- on small coefficients and over
the full int16 x uint16 range --, the file calls to PIL (libjpeg-turbo) on PIL-written files, and the enqueue-only entry to the stream-order
contract of DESIGN.md 4.15."""
import ctypes as C

import numpy as np
import pytest

import exif_cases as X
import jpeg_libjpeg_cases as LC
import stream_order as SO
from ffpic_amd import capi, ops, tensors
from stream_order import Operand, Output

pytestmark = pytest.mark.gpu
FILL = 0xA5
LJ, PROG = capi.FFHIP_JPEG_PIXELS_LIBJPEG, capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE
BATCH = LC.WRITER_SIZES + LC.EXTRA_SIZES


# ---------------------------------------------------------------------------------------------------- the items call
def layout_of(pictures):
    """every picture at a 16-byte offset of ONE allocation, pitches of exactly 4 x the coded width and that plus 16 in turn, guard bytes between"""
    places, total = [], 48
    for k, p in enumerate(pictures):
        pitch = 4 * p.geom.width + 16 * (k % 2)
        places.append((total, pitch))
        total += pitch * p.geom.height + 16 * (1 + k % 3)
    return places, total


def items_of(pictures, places, out_ptr, planes, quants):
    items = []
    for p, (off, pitch), devs, dq in zip(pictures, places, planes, quants):
        it = capi.JpegItem()
        it.geom = p.geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [d.ptr if d is not None else None for d in devs]
        it.d_quant, it.d_bgra, it.pitch = dq.ptr, out_ptr + off, pitch
        items.append(it)
    return items


def expected_buffer(pictures, places, total, got=None):
    """0xA5 everywhere but the display rectangles, which hold the host function's pixels; with `got`, the coded picture outside the display
    rectangle (written, unspecified) is taken from there"""
    want = np.full(total, FILL, np.uint8)
    for p, (off, pitch) in zip(pictures, places):
        H, W = p.geom.height, p.geom.width
        rows = np.lib.stride_tricks.as_strided(want[off:], (H, W, 4), (pitch, 4, 1))
        if got is not None:
            rows[...] = np.lib.stride_tricks.as_strided(got[off:], (H, W, 4), (pitch, 4, 1))
        rows[:p.height, :p.width] = ops.jpeg_libjpeg_picture(p.geom, p.width, p.height, *p.coef, p.quant)
    return want


@pytest.mark.parametrize("full_range", [False, True], ids=["small", "full_range"])
def test_one_mixed_batch_equals_the_host_function(full_range):
    """all layouts, chroma grids of 1..3 samples across, single rows and columns, an interior MCU with all eight neighbours: ONE call.  Inside
    the display rectangle the host function's bytes; outside pitch x coded height, and behind each row's 4 x coded width, nothing is touched"""
    L = capi.require_device()
    pictures = [LC.writer_picture(*s, full_range=full_range) for s in BATCH]
    places, total = layout_of(pictures)
    dout = ops.DeviceBuffer(host=np.full(total, FILL, np.uint8))
    planes = [[ops.DeviceBuffer(host=c) if c is not None else None for c in p.coef] for p in pictures]
    quants = [ops.DeviceBuffer(host=p.quant) for p in pictures]
    items = items_of(pictures, places, dout.ptr, planes, quants)
    ops.jpeg_recon_items_libjpeg(items, [(p.width, p.height) for p in pictures])
    capi.check(L.ffhip_stream_sync(None))
    got = dout.to_host((total,), np.uint8)
    want = expected_buffer(pictures, places, total, got)
    for p, (off, pitch) in zip(pictures, places):                              # picture by picture first, for a readable failure
        H, W = p.geom.height, p.geom.width
        g = np.lib.stride_tricks.as_strided(got[off:], (H, W, 4), (pitch, 4, 1))[:p.height, :p.width]
        w = np.lib.stride_tricks.as_strided(want[off:], (H, W, 4), (pitch, 4, 1))[:p.height, :p.width]
        assert np.array_equal(g, w), (p.name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]          # the guards
    if not full_range:                                                         # ... and the host function is PIL on these (test_jpeg_libjpeg.py)
        p, (off, pitch) = pictures[0], places[0]
        g = np.lib.stride_tricks.as_strided(got[off:], (p.height, p.width, 4), (pitch, 4, 1))
        assert np.array_equal(g[..., 2::-1], LC.pil_rgb(p.data))


# ---------------------------------------------------------------------------------------------------- the file calls
@pytest.fixture(scope="module")
def files():
    """PIL-written: baseline and progressive, with and without restart markers, 4:2:0 / 4:2:2 / 4:4:4 / grey -> [(name, bytes, PIL's RGB)]"""
    f = dict(LC.pil_files())
    a, b = LC.synthetic_rgb(61, 45, 1), LC.synthetic_rgb(50, 33, 2)
    f["420_rst_rows"] = LC.pil_write(a, quality=90, subsampling=2, restart_marker_rows=1)
    f["444_rst_blocks"] = LC.pil_write(b, quality=90, subsampling=0, restart_marker_blocks=3)
    f["422_progressive"] = LC.pil_write(a, quality=90, subsampling=1, progressive=True)
    assert b"\xff\xdd" in f["420_rst_rows"] and b"\xff\xdd" not in f["420"]
    return [(k, v, LC.pil_rgb(v)) for k, v in f.items()]


@pytest.fixture(params=["host", "device"])
def front_end(request):
    """both entropy front ends, baseline and progressive, by the library's switches"""
    v = "1" if request.param == "device" else "0"
    capi.setenv("FFHIP_JPEG_GPU_ENTROPY", v)
    capi.setenv("FFHIP_JPEG_PROGRESSIVE_GPU", v)
    yield request.param
    capi.setenv("FFHIP_JPEG_GPU_ENTROPY", None)
    capi.setenv("FFHIP_JPEG_PROGRESSIVE_GPU", None)


def test_file_call_equals_pil(files, front_end):
    data = [d for _, d, _ in files]
    _, images, _ = ops.jpeg_decode_files_mixed_device(data, n_threads=4, progressive=True, pixels="libjpeg")
    assert ops.progressive_last()[0] == 2 and ops.progressive_last()[4] == (front_end == "device")
    for (name, _, want), img in zip(files, images):
        assert np.array_equal(img[..., 2::-1], want) and (img[..., 3] == 255).all(), (name, front_end)


def test_tensors_equal_pil(files, front_end):
    import torch
    data = [d for _, d, _ in files]
    for layout in ("CHW", "HWC"):
        got = tensors.decode_jpeg_to_tensors(data, layout=layout, progressive=True, pixels="libjpeg")
        for (name, _, want), t in zip(files, got):
            assert t.dtype == torch.uint8
            t = t.cpu().numpy()
            assert np.array_equal(t.transpose(1, 2, 0) if layout == "CHW" else t, want), (name, layout, front_end)
    # without the progressive flag the baseline files take the same path
    base = [(n, d, w) for n, d, w in files if "progressive" not in n]
    for (name, _, want), t in zip(base, tensors.decode_jpeg_to_tensors([d for _, d, _ in base], layout="HWC", pixels="libjpeg")):
        assert np.array_equal(t.cpu().numpy(), want), name


def test_oriented_and_resized_tensor_is_the_existing_stages_on_pil_pixels(files):
    """a file tagged 6 with size=(H, W): everything behind the reconstruction is unchanged, so the tensor is what ffhip_bgra_resize_items and
    ffhip_bgra_orient_items make of PIL's pixels"""
    L = capi.require_device()
    name, data, rgb = files[0]
    h, w = rgb.shape[:2]
    OH, OW = 24, 20                                                                 # upright target; stored: 24 wide, 20 high
    got = tensors.decode_jpeg_to_tensors([X.tagged_jpeg(data, 6)], layout="HWC", size=(OH, OW), apply_exif_orientation=True, pixels="libjpeg")[0]
    bgra = np.concatenate([rgb[..., ::-1], np.full((h, w, 1), 255, np.uint8)], -1)
    src, mid, dst = ops.DeviceBuffer(host=bgra), ops.DeviceBuffer(nbytes=OH * OW * 4), ops.DeviceBuffer(nbytes=OH * OW * 4)
    tensors.resize_bgra([capi.ResizeItem(src.ptr, 4 * w, 0, 0, w, h, mid.ptr, 4 * OH, OH, OW)], antialias=True)
    tensors.orient_bgra([capi.OrientItem(mid.ptr, 4 * OH, 0, 0, OH, OW, dst.ptr, 4 * OW, 6)])
    capi.check(L.ffhip_stream_sync(None))
    want = dst.to_host((OH, OW, 4), np.uint8)[..., 2::-1]
    assert np.array_equal(got.cpu().numpy(), want)


def test_flag_with_a_denominator_is_refused_and_no_flag_is_the_old_call(files):
    L = capi.require_device()
    base = [d for n, d, _ in files if "progressive" not in n]
    n = len(base)
    g0, old, _ = ops.jpeg_decode_files_mixed_device(base, crop=False)
    pitches = [g.width * 4 for g in g0]
    offs = np.concatenate([[0], np.cumsum([(p * g.height + 15) & ~15 for p, g in zip(pitches, g0)])])
    dout = ops.DeviceBuffer(host=np.full(int(offs[-1]) + 16, FILL, np.uint8))
    bufs = [np.frombuffer(d, dtype=np.uint8) for d in base]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    outs = (C.c_void_p * n)(*[dout.ptr + int(o) for o in offs[:-1]])
    pitch = (C.c_int64 * n)(*pitches)
    geoms, status = (capi.JpegGeom * n)(), (C.c_int * n)()
    f = L.ffhip_jpeg_decode_files_mixed_device_ex
    assert f(ptrs, lens, n, 4, outs, pitch, (C.c_int * n)(*([2] * n)), LJ, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 4, outs, pitch, (C.c_int * n)(*([1] * (n - 1) + [2])), LJ | PROG, geoms, status, None) == capi.FFHIP_EINVAL
    capi.check(L.ffhip_stream_sync(None))
    assert (dout.to_host((int(offs[-1]) + 16,), np.uint8) == FILL).all()           # nothing was enqueued
    capi.check(f(ptrs, lens, n, 4, outs, pitch, None, 0, geoms, status, None))
    flat = dout.to_host((int(offs[-1]) + 16,), np.uint8)
    for k in range(n):
        assert np.array_equal(flat[int(offs[k]):int(offs[k]) + old[k].size], old[k].reshape(-1)), k
    with pytest.raises(ValueError):
        tensors.decode_jpeg_to_tensors(base, pixels="libjpeg", reduce=2)


def test_a_tensor_call_without_the_progressive_flag_leaves_the_progressive_record(files):
    """ffhip_debug_progressive_last is the record of the thread's last call that took progressive files.  A tensor call with
    FFHIP_JPEG_PIXELS_LIBJPEG alone writes nothing into it, however many parts it takes: here each of two baseline files is a part of its
    own, and the record a progressive call left before is returned exactly as it was"""
    prog = [d for n, d, _ in files if "progressive" in n]
    base = [d for n, d, _ in files if "progressive" not in n][:2]
    ops.jpeg_decode_files_mixed_device(prog, n_threads=2, progressive=True)
    before = ops.progressive_last()
    assert before[0] == len(prog) and before[1] > 0, before
    capi.setenv("FFHIP_TENSOR_PART_BYTES", 1)
    try:
        got = tensors.decode_jpeg_to_tensors(base, layout="HWC", pixels="libjpeg")
        assert ops.tensor_last_parts() == 2
    finally:
        capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    assert ops.progressive_last() == before
    for t, d in zip(got, base):
        assert np.array_equal(t.cpu().numpy(), LC.pil_rgb(d))


# ---------------------------------------------------------------------------------------------------- stream order
K = 128         # copies of one stall, as test_stream_order_gpu.py holds them to its rule


@pytest.fixture(scope="module")
def stall():
    capi.require_device(0)
    return SO.Stall()


@pytest.fixture(params=["created", "null"])
def stream(request):
    L = capi.require_device(0)
    if request.param == "null":
        yield None
        return
    s = L.ffhip_stream_create()
    assert s
    yield s
    L.ffhip_stream_destroy(s)


def test_recon_items_libjpeg_is_stream_ordered(stall, stream):
    """The scenario of stream_order.py: the planes and the quantiser tables arrive on the stalled stream behind the call's enqueue (the buffers
    hold a decoy then) and are overwritten behind it; the consumer's copy must hold the host function's pixels for the REAL input"""
    L = capi.lib()
    sizes = [(56, 40, 2, 2), (33, 17, 1, 1), (21, 13, 0, 0), (30, 24, 2, 1)]
    true = [LC.writer_picture(*s) for s in sizes]
    decoy = [LC.writer_picture(*s, full_range=True) for s in sizes]
    places, total = layout_of(true)
    out = Output(total)
    dq = [Operand(t.quant, d.quant) for t, d in zip(true, decoy)]
    planes = [[Operand(a, b) if a is not None else None for a, b in zip(t.coef, d.coef)] for t, d in zip(true, decoy)]
    items = items_of(true, places, out.ptr, planes, dq)
    arr = (capi.JpegItem * len(items))(*items)
    shown = (capi.Size * len(items))(*[capi.Size(p.width, p.height) for p in true])
    operands = dq + [o for devs in planes for o in devs if o is not None]

    def call(s):
        capi.check(L.ffhip_jpeg_recon_items_libjpeg(arr, shown, len(items), s), "ffhip_jpeg_recon_items_libjpeg")

    rc = SO.run("jpeg_recon_items_libjpeg", stall, stream, K, call, operands, [out])
    assert rc == 0, rc
    got = out.copied()
    want = expected_buffer(true, places, total, got)
    wrong = expected_buffer(decoy, places, total, got)
    assert not np.array_equal(want, wrong)
    assert np.array_equal(got, want), ("the decoy's pixels" if np.array_equal(got, wrong) else "neither", int((got != want).sum()))
