"""GPU: the batch and planar entry points at the strides, offsets and alignments their argument checks admit -- gaps between rows, planes,
tiles and pictures, bases and strides that choose the other kernel, offsets past 2^31 and 2^32 -- with the machinery of limits.py: every
operand, sources included, lies in one allocation of 0xA5 with 1 MiB in front of and behind it; the written rectangles come back and are
compared byte for byte, the sources must come back as they went up, and everything else is held by the count of bytes that are not 0xA5.
The answer keys are the oracle's (planar colour) and the numpy definition of test_heif_gpu.py (the grid), computed tight on the host
(DESIGN.md 4.15a has the table of cases and sizes)."""
import ctypes as C

import numpy as np
import pytest

import limits as M
import oracle_lib as O
from ffpic_amd import capi, synth
from limits import Layout
from test_color_gpu import oracle_420_8, oracle_420_16
from test_heif_gpu import expected_canvas
from test_hevc_gpu import oracle_tus
from test_vp8_frames_gpu import force, oracle_chain
from test_vp8_gpu import oracle_residual
from test_vp8_lf_gpu import oracle_lf

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


def finish():
    import torch
    capi.sync()
    torch.cuda.synchronize()


def as_bytes(a):
    """[h][w] samples -> [h][w x itemsize] uint8"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


# ---------------------------------------------------------------------------------------------------- A1, B1: planar colour
def oracle_400_16(y, r, c, ctb):
    H, W = y.shape
    o = np.zeros((H, W * 4), np.uint8)
    O.ffo().ffo_yuv400_to_bgra32_16bit(o.reshape(-1), W * 4, np.ascontiguousarray(y).reshape(-1), W, r, c, ctb)
    return o


def planar_key(p, y, u, v):
    """the oracle on one picture's tight planes"""
    if p.bits == 8:
        return oracle_420_8(y, u, v, p.rows, p.cols)
    return oracle_420_16(y, u, v, p.rows, p.cols, p.unit) if p.chroma else oracle_400_16(y, p.rows, p.cols, p.unit)


def planar_samples(p, rng, lo, hi, sets):
    dt = np.uint8 if p.bits == 8 else np.int16
    y = rng.integers(lo, hi, (sets, p.H, p.W)).astype(dt)
    u, v = (rng.integers(lo, hi, (sets, p.H // 2, p.W // 2)).astype(dt) for _ in range(2))
    return y, u, v


def run_planar(p, y, u, v):
    """one call of layout p on planes [sets][.][.] (one set for plane strides 0): pictures, gaps and sources"""
    sets = y.shape[0]
    assert sets == (1 if p.plane_y == 0 else p.n)
    lay = Layout()
    at = p.place(lay.add)
    arena = lay.allocate()
    rects = []
    for i in range(sets):
        rects.append((at[0] + i * p.plane_y * p.es, p.y_stride * p.es, as_bytes(y[i])))
        if p.chroma:
            rects.append((at[1] + i * p.plane_uv * p.es, p.uv_stride * p.es, as_bytes(u[i])))
            rects.append((at[2] + i * p.plane_uv * p.es, p.uv_stride * p.es, as_bytes(v[i])))
    for off, pitch, rows in rects:
        arena.put(off, pitch, rows)
    assert p.call(capi.lib(), arena.ptr, at) == 0
    finish()
    keys = [planar_key(p, y[i], u[i], v[i]) for i in range(sets)]
    rects += [(at[3] + i * p.image_stride, p.pitch, keys[i % sets]) for i in range(p.n)]
    arena.check(rects)
    arena.free()


@pytest.mark.parametrize("y_extra", M.PLANAR_Y_EXTRAS)
@pytest.mark.parametrize("y_off", M.PLANAR_Y_OFFS)
def test_planar_8bit_alignment_product(y_off, y_extra):
    """d_y + 0, 1, 2 bytes x y_stride W, W + 1, W + 2, W + 4 (these two are the parameters) x d_u + 0, 1 x d_v + 0, 1 x uv_stride W / 2,
    W / 2 + 1 x odd or even plane strides larger than a plane: one call each, 3 x 2 macroblocks, three images.  Whichever kernel the entry's
    alignment predicate chooses reads its samples where the strides put them"""
    rng = np.random.default_rng(100 + 10 * y_off + y_extra)
    cases = M.planar_product(y_off, y_extra)
    assert len(cases) == 16 and any(p.packed() for p in cases) == (y_off == 0 and y_extra in (0, 4))
    for p in cases:
        run_planar(p, *planar_samples(p, rng, 0, 256, p.n))


def test_planar_8bit_all_chroma_pairs_misaligned():
    """all 65 536 (u, v) pairs through the kernel the predicate chooses for d_y + 1, d_u + 1, y_stride W + 1, uv_stride W / 2 + 1: 512 x 512"""
    uu, vv = np.meshgrid(np.arange(256), np.arange(256))
    p = M.Planar(8, 32, 32, 16, 1, y_off=1, u_off=1, v_off=0, y_stride=513, uv_stride=257)
    assert not p.packed()
    y = np.random.default_rng(0).integers(0, 256, (1, 512, 512)).astype(np.uint8)
    run_planar(p, y, uu.astype(np.uint8)[None], vv.astype(np.uint8)[None])


PLANAR_CALLS = [(8, True), (16, True), (16, False)]


@pytest.mark.parametrize("bits,chroma", PLANAR_CALLS)
def test_planar_pitch_and_image_stride_gaps(bits, chroma):
    """pitch 4 W + 16, image_stride H pitch + 48 on tight planes (the packed kernel of the 8-bit call): the gaps stay 0xA5"""
    p = M.Planar(bits, 2, 3, 16, 3, chroma=chroma)
    assert p.pitch == 4 * p.W + 16 and p.image_stride == p.H * p.pitch + 48 and p.packed()
    run_planar(p, *planar_samples(p, np.random.default_rng(200 + bits + chroma), 0, 256, 3))


@pytest.mark.parametrize("bits,chroma", PLANAR_CALLS)
def test_planar_plane_strides_0(bits, chroma):
    """one set of planes, n_images 3: three identical pictures"""
    p = M.Planar(bits, 2, 3, 16, 3, chroma=chroma, plane_y=0, plane_uv=0)
    run_planar(p, *planar_samples(p, np.random.default_rng(300 + bits + chroma), 0, 256, 1))


@pytest.mark.parametrize("lo,hi", M.PLANAR_DOMAINS)
@pytest.mark.parametrize("ctb,rows,cols", M.PLANAR_CTBS)
def test_planar_16bit_small_ctbs_and_strides(ctb, rows, cols, lo, hi):
    """ctbsize 2, 6 and 10: pictures whose row pairs are no multiple of 4 and whose pixel quads are no multiple of 64 -- partly empty
    workgroups in x and y -- at y_stride W + 3, uv_stride W / 2 + 1; both 16-bit calls, two images"""
    H, W = ctb * rows, ctb * cols
    assert H // 2 % 4 and H % 4 and W // 4 % 64 and W // 4 > 64 and W % 4 == 0
    rng = np.random.default_rng(400 + ctb)
    for chroma in (True, False):
        p = M.planar_16(chroma, ctb, rows, cols)
        run_planar(p, *planar_samples(p, rng, lo, hi, 2))


@pytest.mark.parametrize("bits,chroma,y_off", [(8, True, 0), (8, True, 1), (16, True, 0), (16, False, 0)])
def test_planar_strides_past_32_bits(bits, chroma, y_off):
    """B1: image_stride 2^32 + 16, plane_stride_y 2^31 + 4 samples (16 bit: 2^30 + 2), two images; the 8-bit call in both kernels.
    Allocations of 10 GiB (4:2:0) and 6 GiB (4:0:0)"""
    p = M.planar_far(bits, chroma, y_off)
    assert p.plane_y * p.es > 1 << 31 and p.image_stride > 1 << 32 and (bits != 8 or p.packed() == (y_off == 0))
    assert sum(p.spans()[k] for k in ((0, 1, 2, 3) if chroma else (0, 3))) < 11 << 30
    run_planar(p, *planar_samples(p, np.random.default_rng(500 + bits + chroma + y_off), 0, 256 if bits == 8 else 1024, 2))


# ---------------------------------------------------------------------------------------------------- A2, B1: the HEIF grid
def run_grid(g, seed):
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 256, (g.rows * g.cols, g.th, g.tw, 4), dtype=np.uint8)
    lay = Layout()
    at = g.place(lay.add)
    arena = lay.allocate()
    rects = [(at[0] + j * g.tile_stride, g.tile_pitch, M.pixel_rows(tiles[j])) for j in range(len(tiles))]
    for off, pitch, rows in rects:
        arena.put(off, pitch, rows)
    assert g.call(capi.lib(), arena.ptr, at) == 0
    finish()
    arena.check(rects + [(at[1], g.canvas_pitch, M.pixel_rows(expected_canvas(tiles, g.cols, g.ow, g.oh)))])
    arena.free()


@pytest.mark.parametrize("ow", list(M.GRID_TAIL))
def test_grid_vector_tail(ow):
    """k_grid_compose<4>'s partial vector: tile_w 64, out_w 177, 178, 179 (1, 2, 3 pixels of the last four), canvas_pitch a multiple of 16
    with 16 bytes and more of 0xA5 behind every row; the last tile row and the last tile column overhang"""
    g = M.GRID_TAIL[ow]
    assert g.vector() and ow % 4 and g.canvas_pitch % 16 == 0 and g.canvas_pitch >= 4 * ow + 16
    assert g.tw * g.cols > ow and g.th * g.rows > g.oh
    run_grid(g, 600 + ow)


@pytest.mark.parametrize("which", list(M.GRID_UNALIGNED))
def test_grid_per_pixel_kernel_by_each_alignment_input(which):
    """canvas base + 4, tiles base + 4, canvas_pitch, tile_pitch, tile_stride a multiple of 4 but not of 16, one at a time"""
    g = M.GRID_UNALIGNED[which]
    inputs = {"canvas": g.canvas_off, "tiles": g.tiles_off, "canvas_pitch": g.canvas_pitch, "tile_pitch": g.tile_pitch, "tile_stride": g.tile_stride}
    assert not g.vector() and [k for k, val in inputs.items() if val % 16] == [which] and inputs[which] % 4 == 0
    run_grid(g, 700 + len(which))


@pytest.mark.parametrize("tw", list(M.GRID_GAPS))
def test_grid_stride_gaps(tw):
    """tile_pitch 4 tile_w + 32, tile_stride tile_pitch tile_h + 64, canvas_pitch 4 out_w + 20; 3 x 2 tiles, both last ones overhanging"""
    g = M.GRID_GAPS[tw]
    assert (g.tile_pitch, g.tile_stride, g.canvas_pitch) == (4 * tw + 32, (4 * tw + 32) * g.th + 64, 4 * g.ow + 20)
    assert g.tw * g.cols > g.ow and g.th * g.rows > g.oh and g.vector() == (tw == 64)
    run_grid(g, 800 + tw)


@pytest.mark.parametrize("which", list(M.GRID_FAR))
def test_grid_strides_past_32_bits(which):
    """B1: tile_stride 2^31 + 16 with three tiles; canvas_pitch 2^31 + 16 with out_h 3: the third tile, the third row, start past 2^32.
    An allocation of 4 GiB each"""
    g = M.GRID_FAR[which]
    assert max(g.spans()) > 1 << 32 and g.vector()
    run_grid(g, 900 + len(which))


# ---------------------------------------------------------------------------------------------------- A3, B1: the JPEG batch call
JPEG_GEOMS = {**{k: v[:3] for k, v in M.JPEG_CLASSES.items()}, **M.JPEG_TWO_PASS}


def run_jpeg_batch(name, cols, rows, n, quant_stride, seed, image_stride=None):
    """n pictures of adversarial coefficients, a table set per picture (one for quant_stride 0), pitch 4 W + 16, image_stride H pitch + 32
    unless given; the key is the oracle on one picture at a time with that picture's tables"""
    import torch
    ncomp, h, v = JPEG_GEOMS[name]
    geom, ogeom = capi.jpeg_geom(cols, rows, ncomp, h, v), O.make_geom(cols, rows, ncomp, h, v)
    rng = np.random.default_rng(seed)
    blocks = synth.adversarial_blocks(rng, n * (geom.y_blocks + 2 * geom.c_blocks))
    rng.shuffle(blocks)
    cy = np.ascontiguousarray(blocks[:n * geom.y_blocks]).reshape(n, -1)
    cu, cv = (np.ascontiguousarray(blocks[n * geom.y_blocks + k * n * geom.c_blocks:][:n * geom.c_blocks]).reshape(n, -1) for k in (0, 1))
    sets = n if quant_stride else 1
    q = rng.integers(1, 65536, (sets, 4, 64)).astype(np.uint16)
    pitch = 4 * geom.width + 16
    image_stride = pitch * geom.height + 32 if image_stride is None else image_stride
    need = capi.lib().ffhip_jpeg_workspace_bytes(C.byref(geom), n)
    assert (need > 0) == (name in M.JPEG_TWO_PASS)
    lay = Layout()
    planes = [cy] + ([cu, cv] if ncomp == 3 else [])
    at = [lay.add(p.nbytes) for p in planes]
    at_q = lay.add(((sets - 1) * quant_stride + 256) * 2)
    at_o = lay.add((n - 1) * image_stride + (geom.height - 1) * pitch + 4 * geom.width)
    at_w = lay.add(need + 64) if need else None
    arena = lay.allocate()
    rects = [(a, p.nbytes, as_bytes(p.reshape(1, -1))) for a, p in zip(at, planes)]
    rects += [(at_q + 2 * i * quant_stride, 512, as_bytes(q[i].reshape(1, -1))) for i in range(sets)]
    for off, row, data in rects:
        arena.put(off, row, data)
    ptr = [arena.ptr + a for a in at] + [None, None]
    rc = capi.lib().ffhip_jpeg_recon_batch(C.byref(geom), n, ptr[0], ptr[1], ptr[2], arena.ptr + at_q, quant_stride, arena.ptr + at_o, pitch,
                                           image_stride, arena.ptr + at_w if need else None, need, None)
    assert rc == 0
    finish()
    if need:                                                    # what the workspace holds is the library's; behind it nothing changed
        assert not bool((arena.t[at_w + need:at_w + need + 64] != M.FILL).any())
        arena.t[at_w:at_w + need] = M.FILL
    for i in range(n):
        key = O.oracle_jpeg_recon(ogeom, cy[i], cu[i] if ncomp == 3 else None, cv[i] if ncomp == 3 else None, q[i % sets])[0]
        rects.append((at_o + i * image_stride, pitch, M.pixel_rows(key)))
    arena.check(rects)
    arena.free()


@pytest.mark.parametrize("size", [0, 1])
@pytest.mark.parametrize("name", list(JPEG_GEOMS))
def test_jpeg_batch_gaps_and_quant_strides(name, size):
    """every fused layout class and one two-pass geometry of each kind (their workspace inside the allocation, 64 bytes of 0xA5 behind what
    ffhip_jpeg_workspace_bytes asks for): 5 x 3 MCUs, and a row that ends in a partial unit; three pictures with gaps between rows and
    pictures; quant_stride 0, 256 and 264 with a table set per picture, so that a wrong stride changes pixels"""
    cols, rows = M.jpeg_batch_sizes(name)[size]
    if name in M.JPEG_CLASSES:
        assert cols % M.JPEG_CLASSES[name][3]
    for qs in (0, 256, 264):
        run_jpeg_batch(name, cols, rows, 3, qs, 1000 + 10 * size + qs)


@pytest.mark.parametrize("name", list(M.JPEG_CLASSES))
def test_jpeg_batch_image_stride_past_32_bits(name):
    """B1: image_stride 2^32 + 16, two pictures of 5 x 3 MCUs, every fused class; an allocation of 4 GiB"""
    run_jpeg_batch(name, 5, 3, 2, 264, 1100, image_stride=(1 << 32) + 16)


# ---------------------------------------------------------------------------------------------------- B2: counts
class FarRegion:
    """n units of `unit` bytes in an arena: zeros made on the device, but for the first and the last FAR_ENDS units, which come from the host"""

    def __init__(self, lay, n, unit):
        self.n, self.unit, self.off = n, unit, lay.add(n * unit)

    def fill(self, arena, head, tail):
        arena.t[self.off:self.off + self.n * self.unit].zero_()
        arena.put(self.off, head.nbytes, as_bytes(head.reshape(1, -1)))
        arena.put(self.off + (self.n - M.FAR_ENDS) * self.unit, tail.nbytes, as_bytes(tail.reshape(1, -1)))

    def holds(self, arena, head, tail):
        """the ends byte for byte on the host, zeros in between on the device; -> its bytes that are not 0xA5"""
        ends = M.FAR_ENDS * self.unit
        head, tail = as_bytes(head.reshape(1, -1)), as_bytes(tail.reshape(1, -1))
        assert head.shape == tail.shape == (1, ends)
        assert np.array_equal(arena.get(self.off, ends, 1, ends), head)
        assert np.array_equal(arena.get(self.off + self.n * self.unit - ends, ends, 1, ends), tail)
        a, b = self.off + ends, self.off + self.n * self.unit - ends
        assert not any(bool(arena.t[k:min(k + (1 << 30), b)].any()) for k in range(a, b, 1 << 30))
        return self.n * self.unit - int((head == M.FILL).sum()) - int((tail == M.FILL).sum())


def run_far(n, regions, small, call, keys):
    """regions: name -> (unit bytes, head, tail) of the inputs; small: name -> a whole small input; keys: (unit bytes, head, tail) of the
    output; call(addresses by name, address of the output) -> the library's code"""
    lay = Layout()
    far = {k: FarRegion(lay, n, unit) for k, (unit, _, _) in regions.items()}
    at = {k: lay.add(v.nbytes) for k, v in small.items()}
    out = FarRegion(lay, n, keys[0])
    arena = lay.allocate()
    for k, (_, head, tail) in regions.items():
        far[k].fill(arena, head, tail)
    for k, v in small.items():
        arena.put(at[k], v.nbytes, as_bytes(v.reshape(1, -1)))
    ptrs = {**{k: arena.ptr + f.off for k, f in far.items()}, **{k: arena.ptr + a for k, a in at.items()}}
    assert call(ptrs, arena.ptr + out.off) == 0
    finish()
    count = out.holds(arena, keys[1], keys[2]) + sum(far[k].holds(arena, head, tail) for k, (_, head, tail) in regions.items())
    for k, v in small.items():
        assert np.array_equal(arena.get(at[k], v.nbytes, 1, v.nbytes), as_bytes(v.reshape(1, -1)))
        count += int((as_bytes(v.reshape(1, -1)) != M.FILL).sum())
    assert arena.changed() == count
    arena.free()


def test_vp8_residual_batch_past_2_to_31_bytes():
    """the smallest n_mb whose levels pass 2^31 bytes, plus 9: zero levels with no tokens, but for 64 random macroblocks at either end;
    the oracle on those, and the oracle's word on a zero macroblock -- zeros -- in between.  Allocations of 2.0 GiB twice"""
    n, E = M.VP8_RESIDUAL_FAR, M.FAR_ENDS
    (lv0, info0), (lv1, info1) = synth.vp8_macroblocks(E, seed=1201, adversarial=True), synth.vp8_macroblocks(E, seed=1202)
    q = synth.vp8_quant(seed=12)
    zero = oracle_residual(np.zeros((1, 25, 16), np.int16), np.zeros((1, 32), np.uint8), q)
    assert not zero.any()
    run_far(n, {"levels": (800, lv0, lv1), "info": (32, info0, info1)}, {"quant": q},
            lambda p, out: capi.lib().ffhip_vp8_residual_batch(n, p["levels"], p["info"], p["quant"], out, None),
            (768, oracle_residual(lv0, info0, q), oracle_residual(lv1, info1, q)))


@pytest.mark.parametrize("nTbS,n_tu", M.HEVC_RESIDUAL_FAR)
def test_hevc_residual_batch_past_2_to_31_bytes(nTbS, n_tu):
    """32 x 32 with 2^20 + 8 TUs and 4 x 4 with 2^26 + 300: zero levels at qP 0, but for 64 random TUs of mixed flags at either end.
    Allocations of 2.0 GiB twice"""
    E, bd = M.FAR_ENDS, 10
    rng = np.random.default_rng(1300 + nTbS)
    scaling = rng.integers(1, 256, (6, nTbS * nTbS)).astype(np.uint8)
    ends = []
    for _ in range(2):
        lv = np.rint(rng.laplace(0, 10, (E, nTbS * nTbS))).astype(np.int16)
        lv[::7] = rng.integers(-32768, 32768, (len(lv[::7]), nTbS * nTbS)).astype(np.int16)
        info = np.zeros((E, 4), np.uint8)
        info[:, 0] = rng.integers(0, 52, E)
        flags = rng.choice([0, 0, 0, 2, 4, 2 | 8, 4 | 8] + ([1, 1] if nTbS == 4 else []), E)
        info[:, 1] = flags if nTbS == 4 else flags & ~8
        info[:, 2] = rng.integers(0, 6, E)
        ends.append((lv, info, oracle_tus(nTbS, lv, info, bd, False, scaling)))
    zero = oracle_tus(nTbS, np.zeros((1, nTbS * nTbS), np.int16), np.zeros((1, 4), np.uint8), bd, False, scaling)
    assert not zero.any()
    unit = nTbS * nTbS * 2
    run_far(n_tu, {"levels": (unit, ends[0][0], ends[1][0]), "info": (4, ends[0][1], ends[1][1])}, {"scaling": scaling},
            lambda p, out: capi.lib().ffhip_hevc_residual_batch(nTbS, n_tu, p["levels"], p["info"], p["scaling"], bd, 0, out, None),
            (unit, ends[0][2], ends[1][2]))


# ---------------------------------------------------------------------------------------------------- A5: HEVC intra
@pytest.mark.parametrize("entry", ["intra_recon", "decode_tiles"])
@pytest.mark.parametrize("bd", [8, 10])
def test_hevc_intra_plane_strides(bd, entry):
    """one 64 x 48 picture, 4:2:0: y_stride width + 12, uv_stride width / 2 + 6, the BGRA pitch padded by 16.  The planes' rows are
    zeroed by a put, the samples between them stay 0xA5; the TU list and the residual lie in the allocation too"""
    w, h = 64, 48
    ys, cs, pitch = w + 12, w // 2 + 6, 4 * w + 16
    tus, res = synth.hevc_intra_tus(w, h, 1400 + bd, adversarial_masks=True)
    if bd > 8:
        res = (res.astype(np.int32) * (1 << (bd - 8))).astype(np.int16)
    tus, res = np.ascontiguousarray(tus), np.ascontiguousarray(res)
    exp = O.oracle_hevc_intra(tus, res, w, h, True, bd, bd)
    geo = [(w, h, ys), (w // 2, h // 2, cs), (w // 2, h // 2, cs)]
    lay = Layout()
    at_t, at_r = lay.add(tus.nbytes), lay.add(res.nbytes)
    at_p = [lay.add(((ph - 1) * st + pw) * 2) for pw, ph, st in geo]
    at_o = lay.add((h - 1) * pitch + 4 * w)
    arena = lay.allocate()
    sources = [(at_t, tus.nbytes, tus.view(np.uint8).reshape(1, -1)), (at_r, res.nbytes, as_bytes(res.reshape(1, -1)))]
    for off, row, data in sources:
        arena.put(off, row, data)
    for a, (pw, ph, st) in zip(at_p, geo):
        arena.put(a, st * 2, np.zeros((ph, pw * 2), np.uint8))
    L, ptr = capi.lib(), arena.ptr
    args = (w, h, ys, w // 2, h // 2, cs, bd, bd)
    if entry == "intra_recon":
        rc = L.ffhip_hevc_intra_recon(tus.ctypes.data, ptr + at_t, len(tus), ptr + at_r, *[ptr + a for a in at_p], *args, None)
    else:
        first = np.zeros(1, np.int64)
        rc = L.ffhip_hevc_decode_tiles(tus.ctypes.data, ptr + at_t, len(tus), first.ctypes.data, 1, ptr + at_r, *[ptr + a for a in at_p], *args,
                                       ptr + at_o, pitch, None)
    assert rc == 0
    finish()
    rects = sources + [(a, st * 2, as_bytes(e)) for a, (pw, ph, st), e in zip(at_p, geo, exp)]
    if entry == "decode_tiles":
        rects.append((at_o, pitch, oracle_420_16(*exp, h // 2, w // 2, 2)))
    arena.check(rects)
    arena.free()


# ---------------------------------------------------------------------------------------------------- A4, B1: the VP8 frame calls
VP8_ENTRIES = ["predict_recon", "loopfilter", "predict_loopfilter", "decode_frames", "decode_frames_no_planes"]


def run_vp8(entry, c, r, n, ft, seed, plane_y=None, plane_uv=None, res_stride=None, image_stride=None):
    """n frames of c x r macroblocks through one frame call, the strides the issue's unless given: plane_stride_y 256 n_mb + 4,
    plane_stride_uv 64 n_mb + 4, residual_stride 384 n_mb + 2, pitch 64 c + 16, image_stride 16 r pitch + 16; a residual map; the planes
    zeroed by a put (ffhip_vp8_loopfilter's hold the oracle's prediction).  Against the oracle chain, frame by frame"""
    n_mb = c * r
    rng = np.random.default_rng(seed)
    modes = np.stack([synth.vp8_modes(c, r, seed=seed + i) for i in range(n)])
    modes[..., 18] = rng.integers(0, 4, modes[..., 18].shape)
    resid = np.stack([synth.vp8_residual(n_mb, seed=seed + 50 + i) for i in range(n)])
    resmap = np.stack([np.maximum.accumulate(np.where(rng.random(n_mb) < 0.3, 0, np.arange(n_mb))) for _ in range(n)]).astype(np.int32)
    filt = synth.vp8_filters(seed=seed)
    plane_y = 256 * n_mb + 4 if plane_y is None else plane_y
    plane_uv = 64 * n_mb + 4 if plane_uv is None else plane_uv
    res_stride = 384 * n_mb + 2 if res_stride is None else res_stride
    pitch = 64 * c + 16
    image_stride = pitch * 16 * r + 16 if image_stride is None else image_stride
    with_planes, with_bgra = entry != "decode_frames_no_planes", entry.startswith("decode_frames")
    pred = [O.oracle_vp8_frame(c, r, modes[i], resid[i], resmap[i]) for i in range(n)]
    if entry == "predict_recon":
        want = pred
    else:
        want = [oracle_lf(c, r, ft, modes[i], filt, pred[i]) if ft else pred[i] for i in range(n)]
    bgra = [oracle_chain(c, r, ft, modes[i], resid[i], filt, resmap[i])[0] for i in range(n)] if with_bgra else None
    lay = Layout()
    at_m, at_map, at_f = lay.add(modes.nbytes), lay.add(resmap.nbytes), lay.add(filt.nbytes)
    at_r = lay.add(((n - 1) * res_stride + 384 * n_mb) * 2)
    at_p = [lay.add((n - 1) * ps + size) for ps, size in ((plane_y, 256 * n_mb), (plane_uv, 64 * n_mb), (plane_uv, 64 * n_mb))] if with_planes else [None] * 3
    at_o = lay.add((n - 1) * image_stride + (16 * r - 1) * pitch + 64 * c) if with_bgra else None
    arena = lay.allocate()
    sources = [(at_m, modes.nbytes, modes.reshape(1, -1)), (at_map, resmap.nbytes, as_bytes(resmap.reshape(1, -1))), (at_f, filt.nbytes, as_bytes(filt.reshape(1, -1)))]
    if entry != "loopfilter":
        sources += [(at_r + 2 * i * res_stride, 768 * n_mb, as_bytes(resid[i].reshape(1, -1))) for i in range(n)]
    for off, row, data in sources:
        arena.put(off, row, data)
    strides = (plane_y, plane_uv, plane_uv)
    if with_planes:
        for i in range(n):
            for k in range(3):
                first = pred[i][k] if entry == "loopfilter" else np.zeros_like(pred[i][k])
                arena.put(at_p[k] + i * strides[k], first.shape[1], first)
    L, ptr = capi.lib(), arena.ptr
    P = [ptr + a if with_planes else None for a in at_p]
    if entry == "predict_recon":
        rc = L.ffhip_vp8_predict_recon(c, r, n, modes.ctypes.data, ptr + at_m, ptr + at_r, res_stride, ptr + at_map, *P, plane_y, plane_uv, None)
    elif entry == "loopfilter":
        rc = L.ffhip_vp8_loopfilter(c, r, n, ft, ptr + at_m, ptr + at_f, *P, plane_y, plane_uv, None)
    elif entry == "predict_loopfilter":
        rc = L.ffhip_vp8_predict_loopfilter(c, r, n, modes.ctypes.data, ptr + at_m, ptr + at_r, res_stride, ptr + at_map, ft, ptr + at_f, *P, plane_y, plane_uv, None)
    else:
        rc = L.ffhip_vp8_decode_frames(c, r, n, modes.ctypes.data, ptr + at_m, ptr + at_r, res_stride, ptr + at_map, ft, ptr + at_f, ptr + at_o, pitch,
                                       image_stride, *P, plane_y, plane_uv, None)
    assert rc == 0
    finish()
    rects = list(sources)
    if with_planes:
        rects += [(at_p[k] + i * strides[k], want[i][k].shape[1], np.ascontiguousarray(want[i][k])) for i in range(n) for k in range(3)]
    if with_bgra:
        rects += [(at_o + i * image_stride, pitch, bgra[i]) for i in range(n)]
    arena.check(rects)
    arena.free()


@pytest.mark.parametrize("ft", [0, 1, 2])
@pytest.mark.parametrize("c,r", [(3, 2), (1, 1)])
@pytest.mark.parametrize("entry", VP8_ENTRIES[:3])
def test_vp8_stage_calls_with_gaps(entry, c, r, ft):
    """ffhip_vp8_predict_recon, ffhip_vp8_loopfilter and ffhip_vp8_predict_loopfilter: three frames, bytes of 0xA5 between the planes and
    between the residual blocks of the frames"""
    run_vp8(entry, c, r, 3, ft, 1500 + 10 * c + ft)


@pytest.mark.parametrize("form", ["fused", "rows"])
@pytest.mark.parametrize("ft", [0, 1, 2])
@pytest.mark.parametrize("c,r", [(3, 2), (1, 1)])
@pytest.mark.parametrize("entry", VP8_ENTRIES[3:])
def test_vp8_decode_frames_with_gaps(entry, c, r, ft, form, monkeypatch):
    """ffhip_vp8_decode_frames with and without delivered planes, the frame kernel and the row kernels: gaps between planes, residual
    blocks, rows and pictures"""
    force(monkeypatch, form)
    run_vp8(entry, c, r, 3, ft, 1600 + 10 * c + ft)


@pytest.mark.parametrize("entry", VP8_ENTRIES[:4])
def test_vp8_frame_calls_strides_past_32_bits(entry, monkeypatch):
    """B1: plane_stride_y 2^31 + 4, residual_stride 2^30 + 2 elements, image_stride 2^32 + 16, two frames of 3 x 2 macroblocks (the row
    kernels; the frame kernel below).  Allocations of up to 8 GiB"""
    force(monkeypatch, "rows")
    run_vp8(entry, 3, 2, 2, 2, 1700, plane_y=(1 << 31) + 4, res_stride=(1 << 30) + 2, image_stride=(1 << 32) + 16)


@pytest.mark.parametrize("entry", VP8_ENTRIES[3:])
def test_vp8_frame_kernel_images_past_32_bits(entry):
    """B1: as many 1 x 1 frames as make the entry choose the frame kernel by itself, strides of 2^25 + 16 (2^24 + 16 elements of
    residual): the last frames' pixels, planes and residual lie past 2^32 bytes.  Allocations of 8 and 12 GiB"""
    form = capi.lib().ffhip_vp8_decode_frames_form
    n = next(k for k in range(1, 4096) if form(k) == 1)
    far = (1 << 25) + 16
    assert n * far > 1 << 32 and n * far * 3 < 16 << 30
    run_vp8(entry, 1, 1, n, 2, 1800, plane_y=far, res_stride=(1 << 24) + 16, image_stride=far)
