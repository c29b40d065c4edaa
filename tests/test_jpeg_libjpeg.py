"""libjpeg's pixel rule on the host (ffhip_jpeg_libjpeg_block / ffhip_jpeg_libjpeg_picture) against PIL (libjpeg-turbo):
equality is exact, over the display rectangle, for files whose coefficients come from 8-bit samples.  No device."""
import ctypes as C

import numpy as np
import pytest

import jpeg_entropy
import jpeg_libjpeg_cases as LC
from ffpic_amd import capi, ops


def rgb_of(bgra):
    assert (bgra[..., 3] == 255).all()
    return bgra[..., 2::-1]


def assert_equals_pil(got_rgb, data, name):
    want = LC.pil_rgb(data)
    assert got_rgb.shape == want.shape, (name, got_rgb.shape, want.shape)
    diff = got_rgb.astype(int) - want
    assert not diff.any(), (name, int((diff != 0).sum()), int(np.abs(diff).max()), np.argwhere(diff != 0)[:4].tolist())


@pytest.mark.parametrize("size", LC.WRITER_SIZES, ids=lambda s: "{}x{}_h{}v{}".format(*s))
def test_written_files_equal_pil(size):
    p = LC.writer_picture(*size)
    got = ops.jpeg_libjpeg_picture(p.geom, p.width, p.height, *p.coef, p.quant)
    assert_equals_pil(rgb_of(got), p.data, p.name)


@pytest.mark.parametrize("name", ["420", "422", "444", "420_3x2", "grey"])
def test_pil_written_files_equal_pil(name):
    data = LC.pil_files()[name]
    d = jpeg_entropy.decode(data)
    geom = capi.jpeg_geom(d["mcu_cols"], d["mcu_rows"], d["ncomp"], d["h"], d["v"], d["qt_id"])
    got = ops.jpeg_libjpeg_picture(geom, d["width"], d["height"], *d["coef"], d["quant"])
    assert_equals_pil(rgb_of(got), data, name)


def test_progressive_twin_equals_pil():
    files = LC.pil_files()
    data = files["420_progressive"]
    g, w, h, progressive = ops.jpeg_probe_any(data)
    assert progressive and (w, h) == (61, 45)
    geom, cy, cu, cv, quant = ops.jpeg_progressive_decode(data)
    got = ops.jpeg_libjpeg_picture(geom, w, h, cy, cu, cv, quant)
    assert_equals_pil(rgb_of(got), data, "420_progressive")
    assert np.array_equal(LC.pil_rgb(data), LC.pil_rgb(files["420"]))       # PIL gives the twins the same pixels


# ---------------------------------------------------------------------------------------------------- the block rule, restated
def _pass(v, s):
    """one 1-D pass on int64 arrays [8][n] wrapped to int32 after every step"""
    w = lambda x: ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    z1 = w((v[2] + v[6]) * 4433); t2 = w(z1 - w(v[6] * 15137)); t3 = w(z1 + w(v[2] * 6270))
    t0 = w((v[0] + v[4]) << 13); t1 = w(w(v[0] - v[4]) << 13)
    t10, t13, t11, t12 = w(t0 + t3), w(t0 - t3), w(t1 + t2), w(t1 - t2)
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = w(a0 + a3), w(a1 + a2), w(a0 + a2), w(a1 + a3)
    z5 = w(w(z3 + z4) * 9633)
    a0, a1, a2, a3 = w(a0 * 2446), w(a1 * 16819), w(a2 * 25172), w(a3 * 12299)
    z1, z2, z3, z4 = w(z1 * -7373), w(z2 * -20995), w(w(z3 * -16069) + z5), w(w(z4 * -3196) + z5)
    a0, a1, a2, a3 = w(a0 + w(z1 + z3)), w(a1 + w(z2 + z4)), w(a2 + w(z2 + z3)), w(a3 + w(z1 + z4))
    outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([w(w(o) + (1 << (s - 1))) >> s for o in outs])


def blocks_restated(coef, quant):
    """[n][64] int16 x [n][64] uint16 -> [n][64] uint8"""
    n = coef.shape[0]
    c = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(n, 8, 8)
    c = ((c + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    ws = _pass(c.transpose(1, 2, 0).reshape(8, 8 * n), 11).reshape(8, 8, n)             # [row v][column u][n]: over v for every column
    out = _pass(ws.transpose(1, 0, 2).reshape(8, 8 * n), 18).reshape(8, 8, n)           # [x][y][n]: over u for every row
    o = ((out + 128 + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    return np.clip(o, 0, 255).transpose(2, 1, 0).reshape(n, 64).astype(np.uint8)


def test_block_equals_the_rule_restated_over_the_full_range():
    rng = np.random.default_rng(2024)
    coef = rng.integers(-32768, 32768, (2000, 64)).astype(np.int16)
    quant = rng.integers(0, 65536, (2000, 64)).astype(np.uint16)
    coef[:8], quant[:8] = [-32768, 32767] * 32, 65535                                   # the corners
    coef[8:16] = 0
    want = blocks_restated(coef, quant)
    got = np.stack([ops.jpeg_libjpeg_block(c, q).reshape(64) for c, q in zip(coef, quant)])
    assert np.array_equal(got, want), int((got != want).sum())
    assert (got[8:16] == 128).all()


def test_flat_patch_keeps_its_colour():
    """DESIGN.md 4.16's example: a flat (250, 20, 30) patch comes back as PIL gives it, not colour-shifted"""
    data = LC.pil_write(np.full((16, 16, 3), (250, 20, 30), np.uint8), quality=95, subsampling=0)
    d = jpeg_entropy.decode(data)
    geom = capi.jpeg_geom(d["mcu_cols"], d["mcu_rows"], d["ncomp"], d["h"], d["v"], d["qt_id"])
    got = rgb_of(ops.jpeg_libjpeg_picture(geom, 16, 16, *d["coef"], d["quant"]))
    assert_equals_pil(got, data, "flat")
    assert np.abs(got.astype(int) - (250, 20, 30)).max() <= 2


# ---------------------------------------------------------------------------------------------------- refusals
def _picture_rc(geom, width, height, cy="ok", cu="ok", cv="ok", quant="ok", out="ok", pitch=None):
    p = LC.writer_picture(41, 23, 2, 2)
    buf = np.zeros((64, 64, 4), np.uint8)
    arg = lambda a, real: None if a is None else C.c_void_p(real.ctypes.data)
    return capi.lib().ffhip_jpeg_libjpeg_picture(C.byref(geom) if geom is not None else None, width, height, arg(cy, p.coef[0]), arg(cu, p.coef[1]),
                                                 arg(cv, p.coef[2]), arg(quant, p.quant), arg(out, buf), 64 * 4 if pitch is None else pitch)


def test_picture_refusals():
    g = LC.writer_picture(41, 23, 2, 2).geom                 # 3 x 2 MCUs of 16 x 16
    assert _picture_rc(g, 41, 23) == 0
    assert _picture_rc(g, 48, 32) == 0 and _picture_rc(g, 33, 17) == 0
    for w, h in [(49, 23), (32, 23), (41, 33), (41, 16), (0, 23), (41, 0), (-1, 23)]:     # past the coded size, or not reaching the last MCU
        assert _picture_rc(g, w, h) == capi.FFHIP_EINVAL, (w, h)
    for kw in [dict(cy=None), dict(cu=None), dict(cv=None), dict(quant=None), dict(out=None)]:
        assert _picture_rc(g, 41, 23, **kw) == capi.FFHIP_EINVAL, kw
    assert _picture_rc(None, 41, 23) == capi.FFHIP_EINVAL
    assert _picture_rc(g, 41, 23, pitch=4 * 41 - 1) == capi.FFHIP_EINVAL
    for bad in [capi.jpeg_geom(3, 2, 3, 3, 1), capi.jpeg_geom(3, 2, 1, 2, 2), capi.jpeg_geom(3, 2, 2, 1, 1), capi.jpeg_geom(0, 2),
                capi.jpeg_geom(3, 2, 3, 2, 2, (0, 4, 1))]:                                  # what ffhip_jpeg_recon_items refuses
        assert _picture_rc(bad, 8 * bad.h * 3, 8 * bad.v * 2) == capi.FFHIP_EINVAL
    grey = capi.jpeg_geom(3, 2, 1, 1, 1)
    assert _picture_rc(grey, 24, 16, cu=None, cv=None) == 0


def test_block_refusals():
    L = capi.lib()
    a = np.zeros(64, np.int16)
    p = C.c_void_p(a.ctypes.data)
    assert L.ffhip_jpeg_libjpeg_block(None, p, p) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_libjpeg_block(p, None, p) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_libjpeg_block(p, p, None) == capi.FFHIP_EINVAL
