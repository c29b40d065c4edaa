"""CPU: reduced-size JPEG decode -- the block rule on the host (ffhip_jpeg_scaled_block) against the rule written in numpy from its text
(tests/jpeg_scaled_rule.py), its tie to the reference's full-size path (DC-only blocks), a sanity check against the reference's own picture,
the size helpers against their definitions, and the argument checks of the three device entries: FFHIP_EINVAL whether or not a device is
present."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import jpeg_scaled_rule as R
import oracle_lib as O
from ffpic_amd import capi, ops, synth, tensors

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
A = 1 << 20     # fake, 16-byte-aligned "device" addresses: nothing is dereferenced before the device check
DENOMS = (2, 4, 8)


@pytest.fixture(scope="module")
def L():
    return capi.lib()


@pytest.fixture
def no_gpu(L):
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present; covered by the -m gpu tests")
    return L


def lib_blocks(coef, quant, d):
    return np.stack([ops.jpeg_scaled_block(b, quant, d) for b in coef]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the block rule
def _rule_with(t, coef):
    """the three steps with the matrix t and quantisers of 1, for the test below to run with matrices other than the rule's"""
    n = len(t)
    F = np.asarray(coef, np.int64).reshape(-1, 8, 8)[:, :n, :n]
    c = R._int16((np.einsum("yv,bvu->byu", t, F) + 1024) >> 11)
    return np.maximum((np.einsum("xu,byu->byx", t, c) + (257 << 17)) >> 18, 0)


@pytest.mark.parametrize("d", DENOMS)
def test_the_library_matrices_are_their_definition(d):
    """Blocks with ONE coefficient set read the library's matrix out entry by entry.  coef[u] = k gives s[y][x] = (T[x][u] 4k + (257 << 17))
    >> 18, and coef[8v] = k gives c[y][0] = (T[y][v] k + 1024) >> 11: over a sweep of k the library must equal the steps run with the matrix
    computed from its DEFINITION, and the same steps with any one entry off by one must differ from it -- so the sweep does pin every entry."""
    n = 8 // d
    t = R.basis(n)
    assert np.abs(t).sum(1).max() == {1: 8192, 2: 16384, 4: 31520}[n]
    ks = np.arange(-1499, 6000, 7)                                 # |T k| / 2048 stays inside int16; below about -790 the clamp at 0 binds
    coef = np.zeros((2 * n, len(ks), 64), np.int16)
    for u in range(n):
        coef[2 * u, :, u], coef[2 * u + 1, :, 8 * u] = ks, ks
    coef = coef.reshape(-1, 64)
    got = lib_blocks(coef, np.ones(64, np.uint16), d)
    assert np.array_equal(got, _rule_with(t, coef))
    for x in range(n):
        for u in range(n):
            for off in (-1, 1):
                t2 = t.copy()
                t2[x, u] += off
                assert not np.array_equal(got, _rule_with(t2, coef)), (x, u, off)


@pytest.mark.parametrize("d", DENOMS)
def test_random_dense_blocks_equal_the_rule(d):
    rng = np.random.default_rng(300 + d)
    quant = rng.integers(1, 256, 64).astype(np.uint16)
    coef = rng.integers(-1024, 1024, (400, 64)).astype(np.int16)
    assert np.array_equal(lib_blocks(coef, quant, d), R.blocks(coef, quant, d))
    q = synth.quant_tables()
    coef = synth._blocks(rng, 400, q[0])                           # what a photograph looks like
    assert np.array_equal(lib_blocks(coef, q[0], d), R.blocks(coef, q[0], d))


@pytest.mark.parametrize("d", DENOMS)
def test_int16_extremes_equal_the_rule(d):
    """coefficients +-2047 against quantisers 255 (products of +-521 985: the int16 store of step 1 wraps, and so can step 2's), and 1
    against 65535 (the product is -1 as an int16)"""
    rng = np.random.default_rng(310 + d)
    coef = (rng.integers(0, 2, (300, 64)) * 4094 - 2047).astype(np.int16)
    coef[0], coef[1] = 2047, -2047
    quant = np.full(64, 255, np.uint16)
    got = lib_blocks(coef, quant, d)
    assert np.array_equal(got, R.blocks(coef, quant, d))
    assert got.max() <= 4068 and got.min() >= 0                    # the upper clamp of the full-size path cannot bind
    ones = np.ones((1, 64), np.int16)
    wide = np.full(64, 65535, np.uint16)
    assert np.array_equal(lib_blocks(ones, wide, d), R.blocks(ones, wide, d))
    # ... and what wraps really is exercised: the dequantised values differ from the plain products
    n = 8 // d
    assert np.any(R._int16(coef.reshape(-1, 8, 8)[:, :n, :n].astype(np.int64) * 255) != coef.reshape(-1, 8, 8)[:, :n, :n].astype(np.int64) * 255)


@pytest.mark.parametrize("d", (2, 4))
def test_a_horizontal_frequency_varies_along_x_only(d):
    """only coef[1] set (u = 1, v = 0): the samples vary along x and are constant along y -- a transposed rule fails here"""
    coef = np.zeros((1, 64), np.int16)
    coef[0, 0], coef[0, 1] = 64, 50
    quant = np.full(64, 8, np.uint16)
    got = lib_blocks(coef, quant, d)[0]
    assert np.array_equal(got, R.blocks(coef, quant, d)[0])
    assert np.all(got == got[0:1, :]) and len(set(got[0])) == 8 // d
    assert np.all(np.diff(got[0]) < 0)                              # the first cosine falls from left to right


def test_block_refusals(L):
    coef, quant, out = np.zeros(64, np.int16), np.ones(64, np.uint16), np.zeros(64, np.int16)
    p = lambda a: a.ctypes.data
    for d in (0, 1, 3, 16, -2):                                     # 1: the full-size rule is not this entry's
        assert L.ffhip_jpeg_scaled_block(p(coef), p(quant), d, p(out)) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_scaled_block(None, p(quant), 2, p(out)) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_scaled_block(p(coef), None, 2, p(out)) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_scaled_block(p(coef), p(quant), 2, None) == capi.FFHIP_EINVAL


# ---------------------------------------------------------------------------------------------------- the tie to the reference
def _full_size_grey(dc, q0, recon):
    """every pixel of a grey 1 x 1-MCU picture whose block holds only the DC coefficient, by the full-size path `recon`"""
    coef = np.zeros(64, np.int16)
    coef[0] = dc
    quant = np.ones((4, 64), np.uint16)
    quant[0, 0] = q0
    return np.asarray(recon(O.make_geom(1, 1, 1, 1, 1, (0, 0, 0)), coef, None, None, quant)).reshape(8, 8, 4)


@pytest.mark.parametrize("witness", ["oracle", "reference"])
def test_dc_only_blocks_equal_the_full_size_path(witness):
    """For every N a DC-only block gives, at every sample, the value the full-size path gives each of its 64 pixels -- exactly: the
    8-point matrix's first column is 8192 as well.  Held through the grey conversion (U = V = 0), which is monotonic in the sample
    below its clamp, and by the sample itself: B of the reference's picture is clamp(int(s + 2.128 x -128)), so s is pinned wherever B is
    inside 1..254, and the cases below are chosen there."""
    if witness == "reference" and not O.have_ref():
        pytest.skip("the reference is not built here")
    recon = O.oracle_jpeg_recon if witness == "oracle" else O.ref_jpeg_recon
    for dc, q0 in [(0, 1), (40, 16), (37, 8), (25, 16), (300, 1), (-20, 3), (1023, 2), (95, 4)]:
        full = _full_size_grey(dc, q0, recon).reshape(8, 8, 4)
        assert np.all(full == full[0, 0])                           # one value a channel
        coef = np.zeros(64, np.int16)
        coef[0] = dc
        quant = np.ones(64, np.uint16)
        quant[0] = q0
        for d in DENOMS:
            s = ops.jpeg_scaled_block(coef, quant, d).astype(np.int64)
            assert np.all(s == s[0, 0])
            px = R.bgra_of(s, np.zeros_like(s), np.zeros_like(s))
            assert np.array_equal(px[0, 0], full[0, 0]), (dc, q0, d)
            if 0 < full[0, 0, 0] < 255:                             # B unclamped: the sample itself
                assert int(np.trunc(float(s[0, 0]) + 2.128 * -128.0)) == full[0, 0, 0]


# ---------------------------------------------------------------------------------------------------- sanity against the reference's picture
# mean |scaled luma - box mean of the full-size luma| over the 640 x 480 fixture, measured on the CPU with the numpy rule (levels of 255):
MEASURED_MAD = {2: 0.8881, 4: 1.1075, 8: 0.5767}
LUMA = (0.07223, 0.71495, 0.21281)      # B, G, R: the combination of the conversion's three rows in which U and V cancel


def test_scaled_luma_against_the_box_mean_of_the_reference_decode(golden):
    """The reduced picture and the box mean of the full-size picture are two different low-pass filters of one signal (the truncated DCT
    keeps the block's low frequencies whole, the box mean attenuates them), so they differ by a level or two on a photograph -- the bound is
    the value measured here plus a quarter of it, for that reason and not for noise: everything is integers and deterministic.  A transposed
    or mis-scaled rule is off by tens of levels."""
    from test_oracle_golden import decode_fixture
    g = golden("jpeg_files.npz")
    dec, geom = decode_fixture("q85_420")
    full = O.oracle_jpeg_recon(geom, dec["coef"][0], dec["coef"][1], dec["coef"][2], dec["quant"])[0]
    H, W = [int(x) for x in g["q85_420_shape"][:2]]
    assert (W, H) == (640, 480)
    assert hashlib.sha256(full[:H, :W].tobytes()).digest() == g["q85_420_sha256"].tobytes()         # the reference's own decode of the file
    luma_full = full[:H, :W, :3].astype(np.float64) @ np.array(LUMA)
    for d in DENOMS:
        Y, _, _ = R.planes(geom.mcu_cols, geom.mcu_rows, 3, 2, 2, dec["coef"][0], dec["coef"][1], dec["coef"][2], dec["quant"], d, dec["qt_id"])
        box = luma_full.reshape(H // d, d, W // d, d).mean((1, 3))
        mad = float(np.abs(np.minimum(Y[:H // d, :W // d], 255) - box).mean())
        print(f"denominator {d}: mean absolute difference {mad:.4f}")
        assert mad <= MEASURED_MAD[d] * 1.25, (d, mad)
        # the library's block rule is that rule: every eighth luma block
        blocks = np.asarray(dec["coef"][0]).reshape(-1, 64)[::8]
        assert np.array_equal(lib_blocks(blocks, np.asarray(dec["quant"]).reshape(4, 64)[dec["qt_id"][0]], d),
                              R.blocks(blocks, np.asarray(dec["quant"]).reshape(4, 64)[dec["qt_id"][0]], d))


# ---------------------------------------------------------------------------------------------------- sizes, rectangles, the choice
SIZES = [(1, 1), (7, 9), (8, 8), (9, 17), (640, 480), (641, 479), (3840, 2160), (4001, 3003), (65535, 1)]


def test_scaled_size_is_the_ceiling(L):
    for w, h in SIZES:
        for d in (1, 2, 4, 8):
            assert ops.jpeg_scaled_size(w, h, d) == (R.scaled_len(w, d), R.scaled_len(h, d))
    a, b = C.c_int(), C.c_int()
    for d in (0, 3, 16, -1):
        assert L.ffhip_jpeg_scaled_size(10, 10, d, C.byref(a), C.byref(b)) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_scaled_size(0, 10, 2, C.byref(a), C.byref(b)) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_scaled_size(10, 10, 2, None, C.byref(b)) == capi.FFHIP_EINVAL


def test_rectangles_map_by_their_definition(L):
    rng = np.random.default_rng(320)
    for w, h in SIZES[1:]:
        rois = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 2, h // 3, w - w // 2, h - h // 3)]         # the whole; the last pixel; touching right and bottom
        for _ in range(20):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            rois.append((x0, y0, int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))))
        for roi in rois:
            for d in (1, 2, 4, 8):
                got = ops.jpeg_scaled_rect(w, h, d, roi)
                assert got == R.mapped_rect(w, h, d, roi), (w, h, d, roi)
                x0, y0, rw, rh = got
                sw, sh = R.scaled_len(w, d), R.scaled_len(h, d)
                assert rw >= 1 and rh >= 1 and x0 + rw <= sw and y0 + rh <= sh                  # inside the scaled picture
                assert x0 * d <= roi[0] and (x0 + rw) * d >= min(roi[0] + roi[2], w) and roi[0] - x0 * d < d        # covers the request, by less than d
                assert rw >= R.scaled_len(roi[2], d)                                            # at least what the choice counts on
    r, out = capi.Rect(0, 0, 11, 5), capi.Rect()
    assert L.ffhip_jpeg_scaled_rect(10, 10, 2, C.byref(r), C.byref(out)) == capi.FFHIP_EINVAL       # leaves the picture
    r = capi.Rect(3, 3, 0, 2)
    assert L.ffhip_jpeg_scaled_rect(10, 10, 2, C.byref(r), C.byref(out)) == capi.FFHIP_EINVAL       # empty
    r = capi.Rect(0, 0, 4, 4)
    assert L.ffhip_jpeg_scaled_rect(10, 10, 5, C.byref(r), C.byref(out)) == capi.FFHIP_EINVAL


def test_the_choice_is_the_largest_denominator_that_still_covers(L):
    for rw, rh in SIZES:
        for ow, oh in [(1, 1), (16, 16), (224, 224), (rw, rh), (R.scaled_len(rw, 8), R.scaled_len(rh, 8)), (R.scaled_len(rw, 8) + 1, 1),
                       (R.scaled_len(rw, 2), R.scaled_len(rh, 2) + 1), (rw + 1, 1), (10 ** 6, 10 ** 6)]:
            d = ops.jpeg_scale_choose(rw, rh, ow, oh)
            assert d == R.choose(rw, rh, ow, oh), (rw, rh, ow, oh)
            covers = lambda k: R.scaled_len(rw, k) >= ow and R.scaled_len(rh, k) >= oh
            assert d == 1 or covers(d)
            assert all(not covers(k) for k in (8, 4, 2) if k > d)
    assert ops.jpeg_scale_choose(3840, 2160, 224, 224) == 8
    assert ops.jpeg_scale_choose(1920, 1080, 224, 224) == 4
    assert ops.jpeg_scale_choose(640, 480, 224, 224) == 2
    assert ops.jpeg_scale_choose(100, 100, 224, 224) == 1              # a target larger than the picture
    for bad in [(0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 1, -3)]:
        assert L.ffhip_jpeg_scale_choose(*bad) == capi.FFHIP_EINVAL


# ---------------------------------------------------------------------------------------------------- the device entries' argument checks
def item(d=2, mcu_cols=5, mcu_rows=3, ncomp=3, h=2, v=2, pitch=None, bgra=A + 4096, y=A, u=A + 1024, v_=A + 2048, q=A + 3072):
    it = capi.JpegItem()
    it.geom = capi.jpeg_geom(mcu_cols, mcu_rows, ncomp, h, v)
    it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, it.d_bgra = y, u if ncomp == 3 else None, v_ if ncomp == 3 else None, q, bgra
    it.pitch = (mcu_cols * (8 // d if d in (1, 2, 4, 8) else 8) * h * 4 + 15) & ~15 if pitch is None else pitch
    return it


def call(L, items, denoms, n=None):
    arr = (capi.JpegItem * max(len(items), 1))(*items)
    den = (C.c_int * max(len(items), 1))(*denoms)
    return L.ffhip_jpeg_recon_items_scaled(arr, den, len(items) if n is None else n, None)


LAYOUTS = [dict(), dict(h=1, v=1), dict(h=2, v=1), dict(h=1, v=2), dict(h=4, v=1), dict(h=1, v=4), dict(ncomp=1, h=1, v=1)]


def test_good_items_of_every_class_and_denominator_reach_the_device_check(no_gpu):
    L = no_gpu
    items, denoms = [], []
    for kw in LAYOUTS:
        for d in (1, 2, 4, 8):
            items.append(item(d, **kw))
            denoms.append(d)
    assert call(L, items, denoms) == capi.FFHIP_ENODEV
    for it, d in zip(items, denoms):
        assert call(L, [it], [d]) == capi.FFHIP_ENODEV


def test_the_scaled_row_is_what_the_pitch_is_held_against(L):
    """5 MCUs of 4:2:0 are 80 pixels wide: 40, 20 and 10 at the three denominators"""
    for d, row in ((2, 160), (4, 80), (8, 40)):
        assert call(L, [item(d, pitch=row - 16)], [d]) == capi.FFHIP_EINVAL
        assert call(L, [item(d, pitch=(row + 15) // 16 * 16 + 4)], [d]) == capi.FFHIP_EINVAL          # not a multiple of 16
        assert call(L, [item(1, pitch=(row + 15) // 16 * 16)], [1]) == capi.FFHIP_EINVAL              # too short for the full-size picture
        if L.ffhip_device_count() == 0:         # good arguments with made-up addresses: only where nothing can be enqueued
            assert call(L, [item(d, pitch=(row + 15) // 16 * 16)], [d]) == capi.FFHIP_ENODEV


BAD_ITEMS = {
    "output misaligned": dict(bgra=A + 4104),
    "output NULL": dict(bgra=None),
    "luma plane misaligned": dict(y=A + 2),
    "chroma plane NULL": dict(u=None),
    "quantiser misaligned": dict(q=A + 3080),
    "two-pass layout: grey with h*v > 1": dict(ncomp=1, h=2, v=2),
    "two-pass layout: h = 3": dict(h=3, v=1),
    "two-pass layout: v = 3": dict(h=1, v=3),
    "zero MCU rows": dict(mcu_rows=0),
}


@pytest.mark.parametrize("why", list(BAD_ITEMS))
@pytest.mark.parametrize("d", DENOMS)
def test_item_refusals(L, why, d):
    kw = dict(BAD_ITEMS[why])
    if why == "chroma plane NULL":
        bad = item(d)
        bad.d_coef_u = None
    else:
        bad = item(d, **kw)
    assert call(L, [bad], [d]) == capi.FFHIP_EINVAL, why
    # one bad item refuses the whole call, wherever it stands and whatever stands beside it
    assert call(L, [item(1), item(4, h=1, v=1), bad], [1, 4, d]) == capi.FFHIP_EINVAL, why


@pytest.mark.parametrize("d", (0, 3, 16, -8, 5))
def test_bad_denominators_are_refused(L, d):
    assert call(L, [item(2)], [d]) == capi.FFHIP_EINVAL
    assert call(L, [item(2), item(2)], [2, d]) == capi.FFHIP_EINVAL


def test_item_counts_and_null_arrays(L):
    assert call(L, [], [], n=0) == 0
    assert L.ffhip_jpeg_recon_items_scaled(None, None, 0, None) == 0
    assert call(L, [item()], [2], n=-1) == capi.FFHIP_EINVAL
    arr = (capi.JpegItem * 1)(item())
    assert L.ffhip_jpeg_recon_items_scaled(arr, None, 1, None) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_recon_items_scaled(None, (C.c_int * 1)(2), 1, None) == capi.FFHIP_EINVAL


def _files(n):
    data = open(os.path.join(GOLDEN, "file_q85_420.jpg"), "rb").read()
    bufs = [C.create_string_buffer(data, len(data)) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(data)] * n)
    return bufs, ptrs, lens


def test_files_entry_checks(L):
    n = 2
    bufs, ptrs, lens = _files(n)
    outs = (C.c_void_p * n)(A, A + (1 << 22))
    pitch = (C.c_int64 * n)(320 * 4, 80 * 4)
    status = (C.c_int * n)()
    geoms = (capi.JpegGeom * n)()
    f = L.ffhip_jpeg_decode_files_mixed_device_scaled
    den = (C.c_int * n)(2, 8)
    assert f(ptrs, lens, n, 2, outs, pitch, None, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(None, lens, n, 2, outs, pitch, den, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, outs, None, den, geoms, status, None) == capi.FFHIP_EINVAL
    for bad in (0, 3, 16):
        assert f(ptrs, lens, n, 2, outs, pitch, (C.c_int * n)(2, bad), geoms, status, None) == capi.FFHIP_EINVAL
    assert f(None, None, 0, 2, None, None, None, None, None, None) == 0
    if L.ffhip_device_count() == 0:
        assert f(ptrs, lens, n, 2, outs, pitch, den, geoms, status, None) == capi.FFHIP_ENODEV
        assert list(status) == [0, 0]
        # a pitch below the SCALED row, a misaligned output: that file's refusal
        pitch[1] = 80 * 4 - 16
        outs[0] = A + 8
        assert f(ptrs, lens, n, 2, outs, pitch, den, geoms, status, None) == capi.FFHIP_ENODEV
        assert list(status) == [capi.FFHIP_EINVAL, capi.FFHIP_EINVAL]
        # ... and the pitch of the scaled picture is too short for the full-size one
        outs[0], pitch[1] = A, 80 * 4
        assert f(ptrs, lens, n, 2, outs, pitch, (C.c_int * n)(2, 1), geoms, status, None) == capi.FFHIP_ENODEV
        assert list(status) == [0, capi.FFHIP_EINVAL]


def test_tensor_entry_checks(L):
    n = 2
    bufs, ptrs, lens = _files(n)
    fmt = tensors.tensor_format("uint8")
    outs = (capi.TensorOut * n)(capi.TensorOut(A, 16, 256), capi.TensorOut(A + 4096, 16, 256))
    size = (capi.Size * n)(capi.Size(16, 16), capi.Size(16, 16))
    status = (C.c_int * n)()
    used = (C.c_int * n)()
    f = L.ffhip_jpeg_decode_files_tensor_scaled
    AAF = capi.FFHIP_RESIZE_ANTIALIAS
    auto = (C.c_int * n)(0, 0)
    assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, None, AAF, auto, used, None, status, None) == capi.FFHIP_EINVAL      # "choose" without out_size
    assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, None, AAF, (C.c_int * n)(2, 0), used, None, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, size, AAF, None, used, None, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, size, 7, auto, used, None, status, None) == capi.FFHIP_EINVAL         # an unknown filter
    for bad in (3, 16, -1):
        assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, size, AAF, (C.c_int * n)(bad, 2), used, None, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, None, outs, None, size, AAF, auto, used, None, status, None) == capi.FFHIP_EINVAL
    if L.ffhip_device_count() == 0:
        assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, size, AAF, auto, used, None, status, None) == capi.FFHIP_ENODEV
        assert list(used) == [8, 8] and list(status) == [0, 0]                      # 640 x 480 still covers 16 x 16 at 1/8
        big = (capi.Size * n)(capi.Size(16, 16), capi.Size(200, 200))
        assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, big, AAF, auto, used, None, status, None) == capi.FFHIP_ENODEV
        assert list(used) == [8, 2]
        outs2 = (capi.TensorOut * n)(capi.TensorOut(A, 320, 320 * 240), capi.TensorOut(A + (1 << 22), 80, 80 * 60))
        assert f(ptrs, lens, n, 2, C.byref(fmt), outs2, None, None, AAF, (C.c_int * n)(2, 8), used, None, status, None) == capi.FFHIP_ENODEV


def test_python_reduce_argument():
    with pytest.raises(ValueError):
        tensors._reduce("auto", None)
    for bad in (0, 3, 16, "half", True):
        with pytest.raises(ValueError):
            tensors._reduce(bad, (16, 16))
    assert tensors._reduce("auto", (16, 16)) == 0 and tensors._reduce(4, None) == 4 and tensors._reduce(1, None) == 1


def test_exports_and_the_workgroup_constant(L):
    for name in ("ffhip_jpeg_scaled_block", "ffhip_jpeg_scaled_size", "ffhip_jpeg_scaled_rect", "ffhip_jpeg_scale_choose",
                 "ffhip_jpeg_recon_items_scaled", "ffhip_jpeg_decode_files_mixed_device_scaled", "ffhip_jpeg_decode_files_tensor_scaled"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert L.ffhip_jpeg_scaled_wg_blocks() == 64
