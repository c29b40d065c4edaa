"""CPU: the argument checks of the batch and planar entry points, at the limits include/ffpic_hip.h and the checks state.  One past each
limit is FFHIP_EINVAL on any machine; the layouts test_batch_limits_gpu.py runs are not refused, which a machine without a device shows as
FFHIP_ENODEV.  The order of the two codes is asserted as each entry has it: ffhip_heif_grid_compose alone asks for the device first.
Addresses are made up: nothing is dereferenced before the device check, and with a device only refused calls are made."""
import ctypes as C

import numpy as np
import pytest

import limits as M
from ffpic_amd import capi

EINVAL, ENODEV = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV
BASE = 1 << 40                                                  # a made-up device address, 256-aligned like an arena's


_NO_DEVICE = []


def no_device():
    """asked once: the admitted calls below are made at made-up addresses and must never reach a device"""
    if not _NO_DEVICE:
        _NO_DEVICE.append(capi.lib().ffhip_device_count() <= 0)
    return _NO_DEVICE[0]


def code(layout):
    lay = M.Layout()
    return layout.call(capi.lib(), BASE, layout.place(lay.add))


# ---------------------------------------------------------------------------------------------------- planar colour
def planar(bits, chroma, **kw):
    return M.Planar(bits, 2, 3, 16, 3, chroma=chroma, **kw)


PLANAR_CALLS = [(8, True), (16, True), (16, False)]


@pytest.mark.parametrize("bits,chroma", PLANAR_CALLS)
def test_planar_one_past_each_limit(bits, chroma):
    W, H = 48, 32
    bad = [planar(bits, chroma, pitch=4 * W + 8), planar(bits, chroma, pitch=4 * W - 16), planar(bits, chroma, image_stride=H * (4 * W + 16) + 8),
           planar(bits, chroma, y_stride=W - 1)]
    if chroma:
        bad.append(planar(bits, chroma, uv_stride=W // 2 - 1))
    many = planar(bits, chroma, plane_y=0, plane_uv=0, image_stride=0)
    many.n = 65536
    bad.append(many)
    for p in bad:
        assert code(p) == EINVAL
    p = planar(bits, chroma)                                    # d_bgra + 8
    at = list(p.place(M.Layout().add))
    at[3] += 8
    assert p.call(capi.lib(), BASE, at) == EINVAL
    if bits == 16:                                              # the block size: even, 2 at least; the width a multiple of 4
        for unit, cols in ((1, 4), (3, 4), (0, 4), (2, 3), (6, 1)):
            assert code(M.Planar(16, 2, cols, unit, 1, chroma=chroma, y_stride=64, uv_stride=32, pitch=256)) == EINVAL


def planar_sides(bits, chroma, rows, cols, unit, pitch):
    """the call's word on a picture of rows x cols blocks at made-up addresses, with strides that fit ints"""
    L = capi.lib()
    o, y, u, v, big = BASE, BASE + (1 << 36), BASE + (2 << 36), BASE + (3 << 36), 0x7ffffffc
    if bits == 8:
        return L.ffhip_yuv420_to_bgra(o, pitch, y, u, v, big, big, rows, cols, 1, 0, 0, 0, None)
    if chroma:
        return L.ffhip_yuv420_to_bgra_16(o, pitch, y, u, v, big, big, rows, cols, unit, 1, 0, 0, 0, None)
    return L.ffhip_yuv400_to_bgra_16(o, pitch, y, big, rows, cols, unit, 1, 0, 0, None)


@pytest.mark.parametrize("bits,chroma", PLANAR_CALLS)
def test_planar_sides_are_checked_in_64_bits(bits, chroma):
    """cols x block, rows x block and 4 x width were int products: sides whose products wrap to something small and legal are refused, and so
    are heights beyond the 65535 workgroups of a launch.  The largest sides are taken"""
    unit = 16 if bits == 8 else 2
    top = 0x7ffffff0                                            # the largest pitch: 2^29 - 4 pixels
    wide = top // 4 // unit
    tall = (8 if chroma else 4) * 65535 // unit
    assert planar_sides(bits, chroma, 1, wide + 1, unit, top) == EINVAL
    assert planar_sides(bits, chroma, tall + 1, 1 if unit == 16 else 2, unit, 64) == EINVAL
    # 2^32 / block + 4 / block... columns: the int product was 4 or 16 pixels
    wrap = ((1 << 32) + 16) // unit
    if wrap <= 0x7fffffff:
        assert planar_sides(bits, chroma, 1, wrap, unit, 64) == EINVAL
        assert planar_sides(bits, chroma, wrap, 1 if unit == 16 else 2, unit, 64) == EINVAL
    assert planar_sides(bits, chroma, 1, (1 << 30) // unit + 4 // min(unit, 4), unit, 64) == EINVAL       # 4 x width wrapped to 16 or 64
    if no_device():
        assert planar_sides(bits, chroma, 1, wide, unit, top) == ENODEV
        assert planar_sides(bits, chroma, tall, 1 if unit == 16 else 2, unit, 64) == ENODEV


def planar_layouts():
    out = [p for y_off in M.PLANAR_Y_OFFS for extra in M.PLANAR_Y_EXTRAS for p in M.planar_product(y_off, extra)]
    out.append(M.Planar(8, 32, 32, 16, 1, y_off=1, u_off=1, y_stride=513, uv_stride=257))
    for bits, chroma in PLANAR_CALLS:
        out += [planar(bits, chroma), planar(bits, chroma, plane_y=0, plane_uv=0)]
    out += [M.planar_16(chroma, *ctb) for chroma in (True, False) for ctb in M.PLANAR_CTBS]
    out += [M.planar_far(8, True, 0), M.planar_far(8, True, 1), M.planar_far(16, True), M.planar_far(16, False)]
    return out


def test_planar_layouts_of_the_gpu_cases_are_admitted():
    layouts = planar_layouts()
    assert len(layouts) == 12 * 16 + 1 + 6 + 6 + 4
    if no_device():
        assert [code(p) for p in layouts] == [ENODEV] * len(layouts)
    # n_images 0 is nothing to do, on any machine, and still checked
    p = planar(8, True)
    p.n = 0
    assert code(p) == 0
    p = planar(8, True, pitch=4 * 48 + 8)
    p.n = 0
    assert code(p) == EINVAL


# ---------------------------------------------------------------------------------------------------- the HEIF grid
def grid_layouts():
    return [*M.GRID_TAIL.values(), *M.GRID_UNALIGNED.values(), *M.GRID_GAPS.values(), *M.GRID_FAR.values()]


def test_grid_asks_for_the_device_first():
    """without a device every call is FFHIP_ENODEV, refused arguments too; with one, one past each limit is FFHIP_EINVAL"""
    g = dict(rows=2, cols=3, tw=64, th=8, ow=178, oh=13)
    bad = [M.Grid(**g, canvas_pitch=4 * 178 - 4), M.Grid(**g, tile_pitch=4 * 64 - 4, tile_stride=4 * 64 * 8), M.Grid(**g, tile_stride=4 * 64 * 8 - 4),
           M.Grid(**g, canvas_pitch=4 * 178 + 2), M.Grid(**g, tile_pitch=4 * 64 + 2), M.Grid(**g, tile_stride=4 * 64 * 8 + 2),
           M.Grid(**g, canvas_off=2), M.Grid(**g, tiles_off=2),
           M.Grid(**{**g, "ow": 193}), M.Grid(**{**g, "ow": 128}), M.Grid(**{**g, "oh": 17}), M.Grid(**{**g, "oh": 8})]
    want = ENODEV if no_device() else EINVAL
    assert [code(b) for b in bad] == [want] * len(bad)
    if no_device():
        assert [code(b) for b in grid_layouts()] == [ENODEV] * 12


def test_grid_layouts_choose_the_kernel_they_are_there_for():
    assert all(g.vector() for g in M.GRID_TAIL.values()) and not any(g.vector() for g in M.GRID_UNALIGNED.values())
    assert [g.vector() for g in M.GRID_GAPS.values()] == [True, False] and all(g.vector() for g in M.GRID_FAR.values())
    aligned = M.Grid(2, 3, 64, 8, 178, 13, canvas_pitch=736)                 # what GRID_UNALIGNED departs from, one input at a time
    assert aligned.vector()


# ---------------------------------------------------------------------------------------------------- the JPEG batch call
def jpeg_code(layout="420", n=3, quant_stride=264, pitch_extra=16, stride_extra=32, coef_off=0, quant_off=0, out_off=0, ws=None, geom=None):
    ncomp, h, v, _ = M.JPEG_CLASSES[layout] if geom is None else geom + (0,)
    g = capi.jpeg_geom(5, 3, ncomp, h, v)
    pitch = 4 * g.width + pitch_extra
    y, u, v_, q, o, w = (BASE + (k << 32) for k in range(6))
    need = capi.lib().ffhip_jpeg_workspace_bytes(C.byref(g), n)
    ws_ptr, ws_bytes = (None, 0) if need == 0 else ((w, need) if ws is None else ws)
    return capi.lib().ffhip_jpeg_recon_batch(C.byref(g), n, y + coef_off, u if ncomp == 3 else None, v_ if ncomp == 3 else None, q + quant_off,
                                             quant_stride, o + out_off, pitch, pitch * g.height + stride_extra, ws_ptr, ws_bytes, None), need


TWO_PASS = [(1, 2, 2), (3, 3, 1)]                              # grey 2 x 2, h = 3: the geometries with a workspace


@pytest.mark.parametrize("layout", list(M.JPEG_CLASSES))
def test_jpeg_batch_one_past_each_limit(layout):
    for kw in (dict(pitch_extra=8), dict(pitch_extra=-16), dict(stride_extra=8), dict(stride_extra=-16), dict(quant_stride=260), dict(quant_stride=248),
               dict(quant_stride=8), dict(coef_off=8), dict(quant_off=8), dict(out_off=8)):
        assert jpeg_code(layout, **kw)[0] == EINVAL, kw
    if no_device():
        assert jpeg_code(layout, n=1, stride_extra=-16)[0] == ENODEV                     # one picture: image_stride is not looked at
        for qs in (0, 256, 264):
            assert jpeg_code(layout, quant_stride=qs) == (ENODEV, 0)
        ncomp, h, v, _ = M.JPEG_CLASSES[layout]
        g = capi.jpeg_geom(5, 3, ncomp, h, v)
        y, u, v_, q, o = (BASE + (k << 32) for k in range(5))
        pitch = 4 * g.width + 16
        assert capi.lib().ffhip_jpeg_recon_batch(C.byref(g), 2, y, u if ncomp == 3 else None, v_ if ncomp == 3 else None, q, 264, o, pitch, (1 << 32) + 16,
                                                 None, 0, None) == ENODEV                # B1's stride


@pytest.mark.parametrize("geom", TWO_PASS)
def test_jpeg_batch_two_pass_workspace(geom):
    need = capi.lib().ffhip_jpeg_workspace_bytes(C.byref(capi.jpeg_geom(5, 3, *geom)), 3)
    assert need > 0 and need % 16 == 0
    w = BASE + (5 << 32)
    if no_device():                                             # (an admitted call: never with a device, the addresses are made up)
        assert jpeg_code(geom=geom) == (ENODEV, need)           # the workspace is looked at behind the device check
        assert jpeg_code(geom=geom, ws=(w, need - 1))[0] == ENODEV
    for kw in (dict(pitch_extra=8), dict(quant_stride=260), dict(stride_extra=8)):
        assert jpeg_code(geom=geom, **kw)[0] == EINVAL


# ---------------------------------------------------------------------------------------------------- the VP8 frame calls
def vp8_code(entry, c=3, r=2, n=3, ft=2, res_off=0, y_off=0, modes_off=0, out_off=0, res_extra=2, plane_extra=4, pitch_extra=16, stride_extra=16,
             planes=True, far=None):
    L, n_mb = capi.lib(), c * r
    h_modes = np.zeros((64, 20), np.uint8)                      # a host pointer that is not NULL: the records are read behind the device check
    modes, res, filt, y, u, v, o = (BASE + (k << 36) for k in range(7))
    rs, py, puv = 384 * n_mb + res_extra, 256 * n_mb + plane_extra, 64 * n_mb + plane_extra
    pitch = 64 * c + pitch_extra
    hm = h_modes.ctypes.data
    if far:                                                     # B1's strides: (plane_stride_y, residual_stride, image_stride)
        py, rs = far[:2]
    if entry == "predict_recon":
        return L.ffhip_vp8_predict_recon(c, r, n, hm, modes + modes_off, res + res_off, rs, None, y + y_off, u, v, py, puv, None)
    if entry == "loopfilter":
        return L.ffhip_vp8_loopfilter(c, r, n, ft, modes + modes_off, filt, y + y_off, u, v, py, puv, None)
    if entry == "predict_loopfilter":
        return L.ffhip_vp8_predict_loopfilter(c, r, n, hm, modes + modes_off, res + res_off, rs, None, ft, filt, y + y_off, u, v, py, puv, None)
    yy, uu, vv = (y + y_off, u, v) if planes else (None, None, None)
    return L.ffhip_vp8_decode_frames(c, r, n, hm, modes + modes_off, res + res_off, rs, None, ft, filt, o + out_off, pitch,
                                     far[2] if far else pitch * 16 * r + stride_extra,
                                     yy, uu, vv, py, puv, None)


@pytest.mark.parametrize("entry", ["predict_recon", "predict_loopfilter", "decode_frames"])
def test_vp8_prediction_calls_one_past_each_limit(entry):
    for kw in (dict(res_off=2), dict(res_extra=1), dict(y_off=2), dict(c=1 << 15, r=1 << 15, n=1), dict(c=1 << 10, r=1 << 10, n=1 << 10)):
        if entry == "decode_frames" and "c" in kw:
            kw = dict(kw, pitch_extra=0, stride_extra=0)
        assert vp8_code(entry, **kw) == EINVAL, kw
    if entry == "decode_frames":
        for kw in (dict(pitch_extra=8), dict(pitch_extra=-16), dict(stride_extra=8), dict(out_off=8), dict(modes_off=2), dict(plane_extra=2), dict(ft=3),
                   dict(c=1 << 12, r=1 << 11, n=1, pitch_extra=0, stride_extra=0)):          # n_mb = 2^23
            assert vp8_code(entry, **kw) == EINVAL, kw
    if no_device():
        for c, r in ((3, 2), (1, 1)):
            assert vp8_code(entry, c=c, r=r) == ENODEV
        assert vp8_code(entry, n=2, far=((1 << 31) + 4, (1 << 30) + 2, (1 << 32) + 16)) == ENODEV
        if entry == "decode_frames":
            assert vp8_code(entry, planes=False) == ENODEV
            assert vp8_code(entry, c=1, r=1, n=128, far=((1 << 25) + 16, (1 << 24) + 16, (1 << 25) + 16)) == ENODEV


def test_vp8_loopfilter_one_past_each_limit():
    assert vp8_code("loopfilter", ft=3) == EINVAL
    assert vp8_code("loopfilter", c=1 << 15, r=1 << 15, n=1) == EINVAL
    assert vp8_code("loopfilter", ft=0) == 0                    # WEBP_FILTER_NONE: nothing to do, on any machine
    if no_device():
        assert vp8_code("loopfilter", ft=1) == vp8_code("loopfilter", ft=2) == ENODEV
        assert vp8_code("loopfilter", n=2, far=((1 << 31) + 4, 0, 0)) == ENODEV
        assert vp8_code("loopfilter", c=1 << 15, r=1 << 15 - 1, n=1) == ENODEV             # n_mb x n_images = 2^29


# ---------------------------------------------------------------------------------------------------- the residual batches
def test_residual_batches_one_past_each_limit():
    L = capi.lib()
    lev, info, q, res = (BASE + (k << 40) for k in range(4))
    assert M.VP8_RESIDUAL_FAR * 800 > 1 << 31 > (M.VP8_RESIDUAL_FAR - 10) * 800
    assert all(n * n * 2 * n_tu > 1 << 31 for n, n_tu in M.HEVC_RESIDUAL_FAR)
    for args in ((-1, lev, info, q, res), (5, lev + 8, info, q, res), (5, lev, info + 2, q, res), (5, lev, info, q + 2, res), (5, lev, info, q, res + 8),
                 (0x7fffffff * 8 + 1, lev, info, q, res)):
        assert L.ffhip_vp8_residual_batch(*args, None) == EINVAL
    for args in ((5, 7, lev, info, None, 8, 0, res), (4, -1, lev, info, None, 8, 0, res), (4, 7, lev, info, None, 7, 0, res), (4, 7, lev, info, None, 17, 0, res),
                 (4, 7, lev + 8, info, None, 8, 0, res), (4, 7, lev, info + 2, None, 8, 0, res), (4, 7, lev, info, q + 2, 8, 0, res), (4, 7, lev, info, None, 8, 0, res + 8)):
        assert L.ffhip_hevc_residual_batch(*args, None) == EINVAL
    assert L.ffhip_vp8_residual_batch(0, None, None, None, None, None) == 0 == L.ffhip_hevc_residual_batch(4, 0, None, None, None, 8, 0, None, None)
    if no_device():
        assert L.ffhip_vp8_residual_batch(M.VP8_RESIDUAL_FAR, lev, info, q, res, None) == ENODEV
        for n, n_tu in M.HEVC_RESIDUAL_FAR:
            assert L.ffhip_hevc_residual_batch(n, n_tu, lev, info, q, 10, 0, res, None) == ENODEV


# ---------------------------------------------------------------------------------------------------- HEVC intra
def hevc_code(entry, w=64, h=48, y_extra=12, uv_extra=6, pitch_extra=16, out_off=0, bd=8, n_tus=5):
    L = capi.lib()
    h_tus = np.zeros(32 * 8, np.uint8)                          # a host pointer that is not NULL: the records are read behind the device check
    tus, res, y, u, v, o = (BASE + (k << 32) for k in range(6))
    args = (w, h, w + y_extra, w // 2, h // 2, w // 2 + uv_extra, bd, bd)
    if entry == "intra_recon":
        return L.ffhip_hevc_intra_recon(h_tus.ctypes.data, tus, n_tus, res, y, u, v, *args, None)
    first = np.zeros(1, np.int64)
    return L.ffhip_hevc_decode_tiles(h_tus.ctypes.data, tus, n_tus, first.ctypes.data, 1, res, y, u, v, *args, o + out_off, 4 * w + pitch_extra, None)


@pytest.mark.parametrize("entry", ["intra_recon", "decode_tiles"])
def test_hevc_intra_one_past_each_limit(entry):
    for kw in (dict(y_extra=-1), dict(bd=7), dict(bd=16), dict(n_tus=-1), dict(n_tus=1 << 31)):
        assert hevc_code(entry, **kw) == EINVAL, kw
    if entry == "decode_tiles":
        for kw in (dict(pitch_extra=8), dict(pitch_extra=-16), dict(out_off=8), dict(w=62), dict(h=47)):
            assert hevc_code(entry, **kw) == EINVAL, kw
    if no_device():
        assert hevc_code(entry) == hevc_code(entry, bd=10) == ENODEV
