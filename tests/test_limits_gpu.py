"""GPU: every device stage at the limits its argument check admits -- the largest sides, the last 31-bit source offset, destination
offsets past 32 bits, the widest row, the floats' edges -- against answer keys that are no run of the library (limits.py, the numpy
rules of the stages' own tests, the oracle, the spec witnesses).  No tolerance anywhere.  Every case is the smallest picture that still
reaches its limit; the allocations around them, up to 8 GiB, are 0xA5 on the device and are counted there, never mirrored on the host
(DESIGN.md 4.15a has the table of cases and sizes)."""
import ctypes as C

import numpy as np
import pytest

import exif_cases as X
import limits as M
import oracle_lib as O
import png_cases
import png_spec
import png_writer
import vp8l_cases
import vp8l_writer
from ffpic_amd import capi, ops, synth, tensors
from limits import AA, BIL, F16, F32, FILL, U8, Layout, pixel_rows
from test_resize_gpu import resize_rule
from test_tensor_gpu import FORMATS, NP_DTYPE, expected, make_format
from test_vp8_frames_gpu import oracle_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device():
    import torch
    capi.require_device(0)
    yield
    try:                                                        # a failed assertion is this test's alone; a device error ends the module
        capi.sync()
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit(f"the device reports an error behind this test ({e}): nothing more is started on it", returncode=3)
    torch.cuda.empty_cache()


def es_of(dtype):
    return np.dtype(NP_DTYPE[dtype]).itemsize


def finish():
    import torch
    capi.sync()
    torch.cuda.synchronize()


def on_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


# ---------------------------------------------------------------------------------------------------- 1. resize, side limits
@pytest.fixture(scope="module")
def side_keys():
    """the two source pictures and, per filter, every SIDE_CASES item's place in them and its expected output, computed once on the host"""
    rng = np.random.default_rng(1601)
    wide, tall = rng.integers(0, 256, (2, 16384, 4), dtype=np.uint8), rng.integers(0, 256, (16384, 2, 4), dtype=np.uint8)
    places = [("wide", 0, 0), ("wide", 0, 0), ("tall", 0, 0), ("wide", 5, 1), ("wide", 7, 0), ("wide", 1, 1), ("wide", 0, 1)]
    keys = {}
    for filt in (BIL, AA):
        keys[filt] = []
        for (w, h, ow, oh), (pic, x0, y0) in zip(M.SIDE_CASES, places):
            v = (wide if pic == "wide" else tall)[y0:y0 + h, x0:x0 + w]
            assert v.shape[:2] == (h, w)
            keys[filt].append(v if (w, h) == (ow, oh) else M.resize_sparse(v, oh, ow, filt))       # equal sizes: "a copy"
    return wide, tall, places, keys


@pytest.mark.parametrize("one_by_one", [False, True])
@pytest.mark.parametrize("filt", [BIL, AA])
def test_resize_side_limits(side_keys, filt, one_by_one):
    """sides of 16384 in and out, on either axis: a 16384-tap run through four LDS chunks of exactly 4096, 16384 rows in y, 64 column tiles,
    `first` = 16383 in its 16-bit field; one mixed call, and one call per item"""
    wide, tall, places, keys = side_keys
    lay = Layout()
    at = {"wide": lay.add(wide.nbytes), "tall": lay.add(tall.nbytes)}
    src = lay.allocate()
    src.put(at["wide"], 65536, pixel_rows(wide))
    src.put(at["tall"], 8, pixel_rows(tall))
    lay, outs = Layout(), []
    for w, h, ow, oh in M.SIDE_CASES:
        pitch = 4 * ow + 12
        outs.append((lay.add(pitch * (oh - 1) + 4 * ow), pitch))
    dst = lay.allocate()
    items = []
    for (w, h, ow, oh), (pic, x0, y0), (off, pitch) in zip(M.SIDE_CASES, places, outs):
        items.append(capi.ResizeItem(src.ptr + at[pic], 65536 if pic == "wide" else 8, x0, y0, w, h, dst.ptr + off, pitch, ow, oh))
    for part in ([[it] for it in items] if one_by_one else [items]):
        tensors.resize_bgra(part, antialias=filt == AA)
    finish()
    dst.check([(off, pitch, pixel_rows(key)) for (off, pitch), key in zip(outs, keys[filt])])
    src.check([(at["wide"], 65536, pixel_rows(wide)), (at["tall"], 8, pixel_rows(tall))])
    src.free(), dst.free()


# ---------------------------------------------------------------------------------------------------- 2. the last 31-bit source offset
PITCH, Y0, HEIGHT, WIDTH = 1 << 20, 2037, 10, 70
X0 = PITCH // 4 - WIDTH                                         # 4 (x0 + width) == pitch
assert (Y0 + HEIGHT) * PITCH == 0x7ff00000                      # the last multiple of the pitch below 2^31


class LastOffsetSource:
    """A 2 GiB picture of pitch 2^20 with two rectangles uploaded: its last ten rows' last 70 pixels, and 33 x 5 pixels at (3, 0)"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        lay = Layout()
        self.base = lay.add((Y0 + HEIGHT) * PITCH)
        self.arena = lay.allocate()
        self.rects = [(X0, Y0, rng.integers(0, 256, (HEIGHT, WIDTH, 4), dtype=np.uint8)), (3, 0, rng.integers(0, 256, (5, 33, 4), dtype=np.uint8))]
        for x0, y0, pic in self.rects:
            self.arena.put(self.base + y0 * PITCH + 4 * x0, PITCH, pixel_rows(pic))
        self.ptr = self.arena.ptr + self.base

    def check_untouched_and_free(self):
        self.arena.check([(self.base + y0 * PITCH + 4 * x0, PITCH, pixel_rows(pic)) for x0, y0, pic in self.rects])
        self.arena.free()


@pytest.mark.parametrize("filt", [BIL, AA])
def test_resize_at_the_last_source_offset(filt):
    src = LastOffsetSource(2100 + filt)
    lay, items, rects = Layout(), [], []
    for (x0, y0, pic), (ow, oh) in zip(src.rects, ((33, 7), (40, 9))):
        pitch = 4 * ow + 8
        rects.append((lay.add(pitch * oh), pitch, pixel_rows(resize_rule(pic, oh, ow, filt))))
        items.append([src.ptr, PITCH, x0, y0, pic.shape[1], pic.shape[0], rects[-1][0], pitch, ow, oh])
    dst = lay.allocate()
    tensors.resize_bgra([capi.ResizeItem(*it[:6], dst.ptr + it[6], *it[7:]) for it in items], antialias=filt == AA)
    finish()
    dst.check(rects)
    dst.free()
    src.check_untouched_and_free()


@pytest.mark.parametrize("o", range(1, 9))
def test_orient_at_the_last_source_offset(o):
    src = LastOffsetSource(2200 + o)
    lay, items, rects = Layout(), [], []
    for x0, y0, pic in src.rects:
        uw, uh = X.upright_size(pic.shape[1], pic.shape[0], o)
        pitch = 4 * uw + 12
        rects.append((lay.add(pitch * uh), pitch, pixel_rows(X.orient(pic, o))))
        items.append([src.ptr, PITCH, x0, y0, pic.shape[1], pic.shape[0], rects[-1][0], pitch, o])
    dst = lay.allocate()
    tensors.orient_bgra([capi.OrientItem(*it[:6], dst.ptr + it[6], *it[7:]) for it in items])
    finish()
    dst.check(rects)
    dst.free()
    src.check_untouched_and_free()


@pytest.mark.parametrize("dtype,planar,bgr", FORMATS)
def test_tensor_at_the_last_source_offset(dtype, planar, bgr):
    src = LastOffsetSource(2300 + 100 * dtype + 10 * planar + bgr)
    f, es = make_format(dtype, planar, bgr), es_of(dtype)
    lay, items, rects = Layout(), [], []
    for k, (x0, y0, pic) in enumerate(src.rects):
        h, w = pic.shape[:2]
        rs = (w if planar else 3 * w) + 3
        ps = rs * h + 5 if planar else 0
        off = lay.add(M.tensor_span(es, planar, rs, ps, h, w) + 16) + (k + 1) * es           # aligned to one element only
        rects += M.tensor_rects(off, es, planar, rs, ps, expected(pic, f))
        items.append([src.ptr, PITCH, x0, y0, w, h, off, rs, ps])
    dst = lay.allocate()
    tensors.bgra_to_tensors([capi.TensorItem(*it[:6], dst.ptr + it[6], *it[7:]) for it in items], f)
    finish()
    dst.check(rects)
    dst.free()
    src.check_untouched_and_free()


# ---------------------------------------------------------------------------------------------------- 3. destination offsets past 32 bits
def small_source(pic):
    lay = Layout()
    off = lay.add(pic.nbytes)
    src = lay.allocate()
    src.put(off, 4 * pic.shape[1], pixel_rows(pic))
    return src, src.ptr + off


@pytest.mark.parametrize("o", [1, 6])
def test_orient_destination_pitch_of_2_to_32(o):
    """the documented largest dst_pitch, upright height 2: the second row starts 4 GiB behind the first"""
    ws, hs = (70, 2) if o == 1 else (2, 70)
    pic = np.random.default_rng(3100 + o).integers(0, 256, (hs, ws, 4), dtype=np.uint8)
    src, sptr = small_source(pic)
    up = X.orient(pic, o)
    assert up.shape[:2] == (2, 70)
    lay, pitch = Layout(), 1 << 32
    off = lay.add(pitch + 4 * 70)
    dst = lay.allocate()
    tensors.orient_bgra([capi.OrientItem(sptr, 4 * ws, 0, 0, ws, hs, dst.ptr + off, pitch, o)])
    finish()
    dst.check([(off, pitch, pixel_rows(up))])
    dst.free(), src.free()


@pytest.mark.parametrize("filt", [BIL, AA])
def test_resize_destination_pitch_past_2_to_32(filt):
    pic = np.random.default_rng(3200 + filt).integers(0, 256, (9, 13, 4), dtype=np.uint8)
    src, sptr = small_source(pic)
    lay, pitch = Layout(), (1 << 32) + 16
    off = lay.add(pitch + 4 * 5)
    dst = lay.allocate()
    tensors.resize_bgra([capi.ResizeItem(sptr, 4 * 13, 0, 0, 13, 9, dst.ptr + off, pitch, 5, 2)], antialias=filt == AA)
    finish()
    dst.check([(off, pitch, pixel_rows(resize_rule(pic, 2, 5, filt)))])
    dst.free(), src.free()


@pytest.mark.parametrize("dtype,planar", [(U8, 1), (U8, 0), (F16, 1), (F16, 0)])
def test_tensor_strides_past_32_bits(dtype, planar):
    """U8: plane_stride 2^31 + 5, row_stride 2^31 + 3; F16: 2^30 + 3 elements either.  The third plane, the third row, start past 4 GiB"""
    h, w = (2, 9) if planar else (3, 9)
    pic = np.random.default_rng(3300 + 10 * dtype + planar).integers(0, 256, (h, w, 4), dtype=np.uint8)
    src, sptr = small_source(pic)
    f, es = make_format(dtype, planar, 0), es_of(dtype)
    far = (1 << 31) + (5 if planar else 3) if dtype == U8 else (1 << 30) + 3
    rs, ps = (w + 2, far) if planar else (far, 0)
    lay = Layout()
    off = lay.add(M.tensor_span(es, planar, rs, ps, h, w))
    assert M.tensor_span(es, planar, rs, ps, h, w) > 1 << 32
    dst = lay.allocate()
    tensors.bgra_to_tensors([capi.TensorItem(sptr, 4 * w, 0, 0, w, h, dst.ptr + off, rs, ps)], f)
    finish()
    dst.check(M.tensor_rects(off, es, planar, rs, ps, expected(pic, f)))
    dst.free(), src.free()


# ---------------------------------------------------------------------------------------------------- 4. the widest row
WIDEST_PITCH = 0x7ffffffc
WIDEST = WIDEST_PITCH // 4
EDGE = 4096                                                     # pixels the host reads back at either end


def widest_source(seed):
    """one row of 2^29 - 1 random pixels, made on the device"""
    import torch
    torch.manual_seed(seed)
    lay = Layout()
    off = lay.add(WIDEST_PITCH)
    src = lay.allocate()
    src.t[off:off + WIDEST_PITCH].random_(0, 256)
    return src, off


def margins_untouched(arena, off, nbytes):
    return not bool((arena.t[:off] != FILL).any()) and not bool((arena.t[off + nbytes:] != FILL).any())


def ends(arena, off, nbytes, n):
    return arena.get(off, n, 1, n)[0], arena.get(off + nbytes - n, n, 1, n)[0]


@pytest.mark.parametrize("o", [2, 5])
def test_orient_the_widest_row(o):
    """pitch 0x7ffffffc, one row: mirrored (2), and transposed to a picture one pixel wide with dst_pitch 4 (5: the row's bytes again)"""
    import torch
    src, soff = widest_source(4000 + o)
    lay = Layout()
    doff = lay.add(WIDEST_PITCH)
    dst = lay.allocate()
    tensors.orient_bgra([capi.OrientItem(src.ptr + soff, WIDEST_PITCH, 0, 0, WIDEST, 1, dst.ptr + doff, WIDEST_PITCH if o == 2 else 4, o)])
    finish()
    s = src.t[soff:soff + WIDEST_PITCH].view(torch.int32)
    d = dst.t[doff:doff + WIDEST_PITCH].view(torch.int32)
    assert torch.equal(d, s.flip(0) if o == 2 else s)
    assert margins_untouched(dst, doff, WIDEST_PITCH) and margins_untouched(src, soff, WIDEST_PITCH)
    (s_first, s_last), (d_first, d_last) = ends(src, soff, WIDEST_PITCH, 4 * EDGE), ends(dst, doff, WIDEST_PITCH, 4 * EDGE)
    up_first, up_last = (X.orient(p.reshape(1, EDGE, 4), o).reshape(-1) for p in ((s_last, s_first) if o == 2 else (s_first, s_last)))
    assert np.array_equal(d_first, up_first) and np.array_equal(d_last, up_last)
    del s, d
    src.free(), dst.free()


def test_tensor_the_widest_row():
    """U8 planar RGB of the 2^29 - 1 pixel row: three planes of 2^29 - 1 bytes, 5 bytes of padding between them"""
    import torch
    src, soff = widest_source(4100)
    f = make_format(U8, 1, 0)
    ps = WIDEST + 5
    lay = Layout()
    doff = lay.add(2 * ps + WIDEST + 16) + 1                                       # aligned to one byte only
    dst = lay.allocate()
    tensors.bgra_to_tensors([capi.TensorItem(src.ptr + soff, WIDEST_PITCH, 0, 0, WIDEST, 1, dst.ptr + doff, WIDEST, ps)], f)
    finish()
    s = src.t[soff:soff + WIDEST_PITCH].view(WIDEST, 4)
    for c in range(3):
        plane = dst.t[doff + c * ps:doff + c * ps + WIDEST]
        assert torch.equal(plane, s[:, 2 - c]), c
        assert c == 2 or not bool((dst.t[doff + c * ps + WIDEST:doff + (c + 1) * ps] != FILL).any())
    assert margins_untouched(dst, doff, 2 * ps + WIDEST) and margins_untouched(src, soff, WIDEST_PITCH)
    s_first, s_last = ends(src, soff, WIDEST_PITCH, 4 * EDGE)
    for c in range(3):
        p_first, p_last = ends(dst, doff + c * ps, WIDEST, EDGE)
        assert np.array_equal(p_first, expected(s_first.reshape(1, EDGE, 4), f)[c, 0])
        assert np.array_equal(p_last, expected(s_last.reshape(1, EDGE, 4), f)[c, 0])
    del s, plane
    src.free(), dst.free()


# ---------------------------------------------------------------------------------------------------- 5. JPEG recon items
def jpeg_planes(rng, geom, q):
    """random planes in the range of the other item tests (synth._blocks), MCU order"""
    cy = synth._blocks(rng, geom.y_blocks, q[0]).reshape(-1)
    if geom.ncomp == 1:
        return cy, None, None
    return cy, synth._blocks(rng, geom.c_blocks, q[1]).reshape(-1), synth._blocks(rng, geom.c_blocks, q[1]).reshape(-1)


def jpeg_item(geom, planes, quant, d_bgra, pitch):
    it = capi.JpegItem()
    it.geom = geom
    it.d_coef_y, it.d_coef_u, it.d_coef_v = [p.data_ptr() if p is not None else None for p in planes]
    it.d_quant, it.d_bgra, it.pitch = quant.data_ptr(), d_bgra, pitch
    return it


def run_jpeg_picture(layout, mcu_cols, mcu_rows, pitch, seed):
    """one item of random planes against the oracle; pitch None: 4 x width + 16"""
    ncomp, h, v, _ = M.JPEG_CLASSES[layout]
    geom, q = capi.jpeg_geom(mcu_cols, mcu_rows, ncomp, h, v), synth.quant_tables()
    host = jpeg_planes(np.random.default_rng(seed), geom, q)
    exp = O.oracle_jpeg_recon(O.make_geom(mcu_cols, mcu_rows, ncomp, h, v), *host, q)[0]
    pitch = 4 * geom.width + 16 if pitch is None else pitch
    planes, dq = [on_device(p) if p is not None else None for p in host], on_device(q)
    lay = Layout()
    off = lay.add(pitch * (geom.height - 1) + 4 * geom.width)
    dst = lay.allocate()
    ops.jpeg_recon_items([jpeg_item(geom, planes, dq, dst.ptr + off, pitch)])
    finish()
    dst.check([(off, pitch, pixel_rows(exp))])
    dst.free()


@pytest.mark.parametrize("layout", ["420", "h1v4"])
def test_jpeg_items_at_the_largest_pitch(layout):
    """2 x 2 MCUs at pitch 0x7fffff0: a macroblock row of 4:2:0 spans 2^31 bytes, an MCU row of h1v4 (32 picture rows) almost 2^32;
    allocations of 3.9 and 7.9 GiB"""
    assert M.JPEG_MAX_PITCH * 16 <= 0x7fffffff < (M.JPEG_MAX_PITCH + 16) * 16
    run_jpeg_picture(layout, 2, 2, M.JPEG_MAX_PITCH, 5100)


@pytest.mark.parametrize("layout", list(M.JPEG_CLASSES))
def test_jpeg_items_4096_units_per_row(layout):
    """the widest picture of every fused layout class, two MCU rows: 16 to 32 MiB of pixels"""
    run_jpeg_picture(layout, M.jpeg_max_cols(layout), 2, None, 5200)


def test_jpeg_items_2_to_20_units_per_picture():
    """The reciprocal division's worst case, n x < 2^32 with n = 2^20 - 1 and x = 4096, in the class where it is the fewest pixels: grey,
    32768 x 256 MCUs of one block, 2^29 pixels.  Buffers: the coefficient plane 1 GiB (DC-only, nine DC values, made on the device), the
    picture 2 GiB at pitch 4 x width + 16; the expected picture (2 GiB) is the oracle's nine MCUs expanded by torch indexing"""
    import torch
    ncomp, h, v, mcus = M.JPEG_CLASSES["grey"]
    mc, mr = M.jpeg_max_cols("grey"), M.JPEG_UNITS_PER_PICTURE // M.JPEG_UNITS_PER_ROW
    assert mc // mcus * mr == 1 << 20 and all(m * 64 * hh * vv >= mcus * 64 for _, hh, vv, m in M.JPEG_CLASSES.values())   # pixels of a unit
    geom, q = capi.jpeg_geom(mc, mr, ncomp, h, v), synth.quant_tables()
    dcs = np.array([-204, -150, -64, -1, 0, 1, 77, 150, 203], np.int16)          # q[0][0] x dc / 8 + 128 stays inside 0..255: nine different MCUs
    assert int(q[0][0]) == 5
    table = np.zeros((len(dcs), 8, 32), np.uint8)
    for k, dc in enumerate(dcs):
        block = np.zeros(64, np.int16)
        block[0] = dc
        table[k] = O.oracle_jpeg_recon(O.make_geom(1, 1, ncomp, h, v), block, None, None, q)[0].reshape(8, 32)
    assert len({t.tobytes() for t in table}) == len(dcs)
    torch.manual_seed(5300)
    idx = torch.randint(0, len(dcs), (mr, mc), device="cuda")
    plane = torch.zeros((mr * mc, 64), dtype=torch.int16, device="cuda")
    plane[:, 0] = on_device(dcs)[idx.reshape(-1)]
    W, H = geom.width, geom.height
    pitch = 4 * W + 16
    lay = Layout()
    off = lay.add(pitch * H)
    dst = lay.allocate()
    ops.jpeg_recon_items([jpeg_item(geom, (plane, None, None), on_device(q), dst.ptr + off, pitch)])
    finish()
    exp = on_device(table)[idx].permute(0, 2, 1, 3).reshape(H, 4 * W)                 # [mr][mc][8][32] -> [mr][8][mc][32]
    assert torch.equal(dst.rows(off, pitch, H, 4 * W), exp)
    del exp
    assert not bool((dst.rows(off + 4 * W, pitch, H, 16) != FILL).any())
    assert margins_untouched(dst, off, pitch * H)
    host_idx = idx.cpu().numpy()
    rows = sorted({0, mr - 1, *[int(r) for r in np.random.default_rng(5301).integers(0, mr, 64)]})
    for r in rows:
        want = table[host_idx[r]].transpose(1, 0, 2).reshape(8, 4 * W)
        assert np.array_equal(dst.get(off + 8 * r * pitch, pitch, 8, 4 * W), want), r
    del plane, idx
    dst.free()


# ---------------------------------------------------------------------------------------------------- 6. VP8 items
@pytest.mark.parametrize("ft", [0, 2])
def test_vp8_items_at_the_largest_pitch(ft):
    """2 x 2 macroblocks, B_PRED among them, at pitch 2^26 - 16: pitch x 16 x mbrows = 2^31 - 512; a 2 GiB allocation"""
    c = r = 2
    pitch = (1 << 26) - 16
    assert pitch * 16 * r == (1 << 31) - 512
    modes = synth.vp8_modes(c, r, seed=6100 + ft)
    modes[:, 0] = [4, 3, 1, 4]                                                       # B_PRED, H_PRED, TM_PRED, B_PRED
    modes[:, 18] = np.random.default_rng(6100 + ft).integers(0, 4, c * r)
    resid, filt = synth.vp8_residual(c * r, seed=6100 + ft), synth.vp8_filters(seed=6100 + ft)
    exp, _ = oracle_chain(c, r, ft, modes, resid, filt)
    assert exp.shape == (16 * r, 64 * c)
    dm, dr = on_device(modes), on_device(resid)
    lay = Layout()
    off = lay.add(pitch * 16 * r)
    dst = lay.allocate()
    it = capi.Vp8Item()
    it.mbcols, it.mbrows, it.h_modes, it.d_modes, it.d_residual = c, r, modes.ctypes.data, dm.data_ptr(), dr.data_ptr()
    it.filter_type = ft
    for k, val in enumerate(filt.reshape(-1)):
        it.filters[k] = int(val)
    it.d_bgra, it.pitch = dst.ptr + off, pitch
    ops.vp8_decode_items([it])
    finish()
    dst.check([(off, pitch, exp)])
    dst.free()


# ---------------------------------------------------------------------------------------------------- 7. PNG and lossless WebP file calls
def run_files(codec, files, keys, pitches):
    """the file call of `codec` into one allocation, picture k at pitches[k]: each holds its key [h][w][4], nothing else changed"""
    n = len(files)
    lay = Layout()
    offs = [lay.add(p * (k.shape[0] - 1) + 4 * k.shape[1]) for k, p in zip(keys, pitches)]
    dst = lay.allocate()
    bufs, ptrs, lens = ops.file_args(files)
    infos = ((capi.PngInfo if codec == "png" else capi.Vp8lInfo) * n)()
    status = (C.c_int * n)()
    outs, pitch = (C.c_void_p * n)(*[dst.ptr + o for o in offs]), (C.c_int64 * n)(*pitches)
    rc = getattr(capi.lib(), f"ffhip_{codec}_decode_files_device")(ptrs, lens, n, 4, outs, pitch, infos, status, None)
    assert rc == 0 and not any(status)
    finish()
    dst.check([(o, p, pixel_rows(k)) for o, p, k in zip(offs, pitches, keys)])
    dst.free()


def png_file(samples, ctype, depth, filters):
    """-> (the file, its key: the witness's picture, which is also the writer's)"""
    data = png_writer.write(samples, ctype, depth, filters=filters)
    key = png_spec.decode(data)
    assert np.array_equal(key, png_writer.expected_bgra(samples, ctype, depth))
    return data, key


@pytest.mark.parametrize("codec", ["png", "vp8l"])
def test_file_calls_at_the_largest_pitch(codec):
    """a 5 x 3 picture at pitch 0x7ffffff0: row 2 lies past 4 GiB"""
    rng = np.random.default_rng(7100)
    if codec == "png":
        data, key = png_file(rng.integers(0, 256, (3, 5, 4)), 6, 8, [1, 4, 3])
    else:
        argb = vp8l_cases.noise(rng, 3, 5)
        data = vp8l_writer.write(argb, [{"type": vp8l_cases.G}, vp8l_cases.predictor(rng, 3, 5), vp8l_cases.cross(rng, 3, 5)])
        key = vp8l_writer.expected_bgra(argb, True)
    run_files(codec, [data], [key], [0x7ffffff0])


def test_png_the_widest_rows():
    """65535 x 1: grey of 1 bit under every filter type a first row can have, RGBA of 16 bits under Sub and Paeth"""
    rng = np.random.default_rng(7200)
    made = [png_file(rng.integers(0, 2, (1, 65535, 1)), 0, 1, f) for f in range(5)]
    made += [png_file(rng.integers(0, 65536, (1, 65535, 4)), 6, 16, f) for f in (1, 4)]
    run_files("png", [d for d, _ in made], [k for _, k in made], [4 * 65536 + 16 * (i % 2) for i in range(len(made))])


def test_png_the_tallest_picture():
    """1 x 65535 grey of 8 bits, the filter types in the order of png_cases.TOUR: 1024 bands of 64 rows, one launch each"""
    data, key = png_file(np.random.default_rng(7300).integers(0, 256, (65535, 1, 1)), 0, 8, png_cases.TOUR)
    run_files("png", [data], [key], [16])
    assert ops.png_last() == (1, 1024)


@pytest.mark.parametrize("w,h", [(16384, 1), (1, 16384)])
def test_vp8l_the_widest_and_the_tallest_picture(w, h):
    """the format's largest sides under a predictor transform: 16384 rows are 256 levels of k_vp8l_predict"""
    rng = np.random.default_rng(7400 + h)
    argb = vp8l_cases.noise(rng, h, w)
    data = vp8l_writer.write(argb, [vp8l_cases.predictor(rng, h, w)])
    run_files("vp8l", [data], [vp8l_writer.expected_bgra(argb, True)], [4 * w + 16 if h == 1 else 16])
    assert ops.vp8l_last() == (1, (h + 63) // 64, 0)


# ---------------------------------------------------------------------------------------------------- 8. the floats at their edges
@pytest.mark.parametrize("dtype,planar", [(F32, 1), (F32, 0), (F16, 1), (F16, 0)])
@pytest.mark.parametrize("scale,bias,what", M.FLOAT_EDGES)
def test_tensor_floats_at_their_edges(dtype, planar, scale, bias, what):
    """all 256 byte values in every channel under scales and biases that overflow F16, land on F16 and F32 subnormals and on the tie at the
    smallest one, and give signed zeros: bit patterns, not values"""
    pic = M.byte_ramps()
    key = M.float_key(pic, dtype, planar, 0, scale, bias)
    assert M.float_key_holds(key, what)
    f, es = make_format(dtype, planar, 0, normalise=False), es_of(dtype)
    for c in range(3):
        f.scale[c], f.bias[c] = scale, bias
    src, sptr = small_source(pic)
    h, w = pic.shape[:2]
    rs = (w if planar else 3 * w) + 2
    ps = rs * h + 3 if planar else 0
    lay = Layout()
    off = lay.add(M.tensor_span(es, planar, rs, ps, h, w) + 16) + es
    dst = lay.allocate()
    tensors.bgra_to_tensors([capi.TensorItem(sptr, 4 * w, 0, 0, w, h, dst.ptr + off, rs, ps)], f)
    finish()
    dst.check(M.tensor_rects(off, es, planar, rs, ps, key))
    dst.free(), src.free()
