"""CPU: the argument checks of ffhip_jpeg_recon_items_libjpeg and of FFHIP_JPEG_PIXELS_LIBJPEG on the two file calls come before the device is
needed -- FFHIP_EINVAL whether or not a device is present, FFHIP_ENODEV for good arguments where there is none -- and the Python arguments'
ValueErrors."""
import ctypes as C
import os

import pytest

from ffpic_amd import capi, ops, tensors

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
A = 1 << 20     # fake, 16-byte-aligned "device" addresses: nothing is dereferenced before the device check
LJ, PROG = capi.FFHIP_JPEG_PIXELS_LIBJPEG, capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE
LAYOUTS = [dict(), dict(h=1, v=1), dict(h=2, v=1), dict(h=1, v=2), dict(h=4, v=1), dict(h=1, v=4), dict(ncomp=1, h=1, v=1)]


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def item(mcu_cols=5, mcu_rows=3, ncomp=3, h=2, v=2, pitch=None, bgra=A + 4096, y=A, u=A + 1024, v_=A + 2048, q=A + 3072):
    it = capi.JpegItem()
    it.geom = capi.jpeg_geom(mcu_cols, mcu_rows, ncomp, h, v)
    it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, it.d_bgra = y, u if ncomp == 3 else None, v_ if ncomp == 3 else None, q, bgra
    it.pitch = mcu_cols * 8 * h * 4 if pitch is None else pitch
    return it


def full(it):
    return it.geom.width, it.geom.height


def call(L, items, sizes, n=None):
    arr = (capi.JpegItem * max(len(items), 1))(*items)
    shown = (capi.Size * max(len(items), 1))(*[capi.Size(w, h) for w, h in sizes])
    return L.ffhip_jpeg_recon_items_libjpeg(arr, shown, len(items) if n is None else n, None)


def test_flag_value_and_exports(L):
    assert LJ == 0x10 and PROG == 1
    for name in ("ffhip_jpeg_libjpeg_block", "ffhip_jpeg_libjpeg_picture", "ffhip_jpeg_recon_items_libjpeg"):
        assert hasattr(L, name) and name in capi.EXPORTS


def test_good_items_of_every_class_reach_the_device_check(L):
    items = [item(**kw) for kw in LAYOUTS]
    sizes = [full(it) for it in items]
    sizes[0] = (full(items[0])[0] - 15, full(items[0])[1] - 15)          # the smallest size that still ends inside the last MCU
    if L.ffhip_device_count() == 0:                                       # made-up addresses: only where nothing can be enqueued
        assert call(L, items, sizes) == capi.FFHIP_ENODEV
        for it, s in zip(items, sizes):
            assert call(L, [it], [s]) == capi.FFHIP_ENODEV


BAD_ITEMS = {
    "output misaligned": dict(bgra=A + 4104),
    "output NULL": dict(bgra=None),
    "pitch below the coded row": dict(pitch=5 * 16 * 4 - 16),
    "pitch no multiple of 16": dict(pitch=5 * 16 * 4 + 4),
    "luma plane misaligned": dict(y=A + 2),
    "luma plane NULL": dict(y=None),
    "chroma plane misaligned": dict(v_=A + 2056),
    "quantiser misaligned": dict(q=A + 3080),
    "quantiser NULL": dict(q=None),
    "two-pass layout: grey with h*v > 1": dict(ncomp=1, h=2, v=2),
    "two-pass layout: h = 3": dict(h=3, v=1),
    "two-pass layout: v = 3": dict(h=1, v=3),
    "zero MCU rows": dict(mcu_rows=0),
}


@pytest.mark.parametrize("why", list(BAD_ITEMS) + ["chroma plane NULL"])
def test_item_refusals(L, why):
    if why == "chroma plane NULL":
        bad = item()
        bad.d_coef_u = None
    else:
        bad = item(**BAD_ITEMS[why])
    size = (bad.geom.mcu_cols * 8 * bad.geom.h, max(bad.geom.mcu_rows, 1) * 8 * bad.geom.v)
    assert call(L, [bad], [size]) == capi.FFHIP_EINVAL, why
    # one bad item refuses the whole call, wherever it stands
    good = item(h=1, v=1)
    assert call(L, [good, bad], [full(good), size]) == capi.FFHIP_EINVAL, why
    assert call(L, [bad, good], [size, full(good)]) == capi.FFHIP_EINVAL, why


@pytest.mark.parametrize("size", [(81, 48), (64, 48), (80, 49), (80, 32), (0, 48), (80, 0), (-3, 48)])
def test_display_sizes_that_do_not_fit_the_geometry(L, size):
    """5 x 3 MCUs of 16 x 16: the width lies in 65..80, the height in 33..48"""
    assert call(L, [item()], [size]) == capi.FFHIP_EINVAL
    assert call(L, [item(h=1, v=1), item()], [(40, 24), size]) == capi.FFHIP_EINVAL


def test_item_counts_and_null_arrays(L):
    assert call(L, [], [], n=0) == 0
    assert L.ffhip_jpeg_recon_items_libjpeg(None, None, 0, None) == 0
    assert call(L, [item()], [(80, 48)], n=-1) == capi.FFHIP_EINVAL
    arr = (capi.JpegItem * 1)(item())
    assert L.ffhip_jpeg_recon_items_libjpeg(arr, None, 1, None) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_recon_items_libjpeg(None, (capi.Size * 1)(capi.Size(80, 48)), 1, None) == capi.FFHIP_EINVAL


def _files(n):
    data = open(os.path.join(GOLDEN, "file_q85_420.jpg"), "rb").read()       # 640 x 480, 4:2:0
    bufs = [C.create_string_buffer(data, len(data)) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(data)] * n)
    return bufs, ptrs, lens


def test_files_entry_flag_checks(L):
    n = 2
    bufs, ptrs, lens = _files(n)
    outs = (C.c_void_p * n)(A, A + (1 << 22))
    pitch = (C.c_int64 * n)(640 * 4, 640 * 4)
    status = (C.c_int * n)()
    geoms = (capi.JpegGeom * n)()
    f = L.ffhip_jpeg_decode_files_mixed_device_ex
    ones = (C.c_int * n)(1, 1)
    for flags in (LJ, LJ | PROG):
        for den in ((2, 1), (1, 8), (4, 4)):                                  # the flag with a denominator other than 1: the whole call
            assert f(ptrs, lens, n, 2, outs, pitch, (C.c_int * n)(*den), flags, geoms, status, None) == capi.FFHIP_EINVAL
        assert f(None, lens, n, 2, outs, pitch, None, flags, geoms, status, None) == capi.FFHIP_EINVAL
    for unknown in (2, 4, 8, 0x20, LJ | 2, 0x80000000):
        assert f(ptrs, lens, n, 2, outs, pitch, None, unknown, geoms, status, None) == capi.FFHIP_EINVAL
    if L.ffhip_device_count() == 0:
        for den in (None, ones):
            assert f(ptrs, lens, n, 2, outs, pitch, den, LJ, geoms, status, None) == capi.FFHIP_ENODEV
            assert list(status) == [0, 0]
            assert f(ptrs, lens, n, 2, outs, pitch, den, LJ | PROG, geoms, status, None) == capi.FFHIP_ENODEV
        pitch[1] = 640 * 4 - 16                                                # that file's refusal
        assert f(ptrs, lens, n, 2, outs, pitch, None, LJ, geoms, status, None) == capi.FFHIP_ENODEV
        assert list(status) == [0, capi.FFHIP_EINVAL]


def test_tensor_entry_flag_checks(L):
    n = 2
    bufs, ptrs, lens = _files(n)
    fmt = tensors.tensor_format("uint8")
    outs = (capi.TensorOut * n)(capi.TensorOut(A, 640, 640 * 480), capi.TensorOut(A + (1 << 22), 640, 640 * 480))
    small = (capi.TensorOut * n)(capi.TensorOut(A, 16, 256), capi.TensorOut(A + 4096, 16, 256))
    size = (capi.Size * n)(capi.Size(16, 16), capi.Size(16, 16))
    status, used, turned = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    upright = (C.c_int * n)(1, 1)
    f = L.ffhip_jpeg_decode_files_tensor_ex
    AAF = capi.FFHIP_RESIZE_ANTIALIAS
    for flags in (LJ, LJ | PROG):
        for den in ((2, 1), (1, 8), (0, 0), (1, 0)):                          # "choose" is a denominator other than 1 too
            assert f(ptrs, lens, n, 2, C.byref(fmt), small, None, size, AAF, (C.c_int * n)(*den), used, upright, turned, flags, None, status,
                     None) == capi.FFHIP_EINVAL, (flags, den)
    for unknown in (2, 0x20, LJ | 4):
        assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, None, AAF, None, used, upright, turned, unknown, None, status, None) == capi.FFHIP_EINVAL
    if L.ffhip_device_count() == 0:
        for den in (None, (C.c_int * n)(1, 1)):
            assert f(ptrs, lens, n, 2, C.byref(fmt), outs, None, None, AAF, den, used, upright, turned, LJ, None, status, None) == capi.FFHIP_ENODEV
            assert list(status) == [0, 0]
        assert f(ptrs, lens, n, 2, C.byref(fmt), small, None, size, AAF, None, used, upright, turned, LJ | PROG, None, status, None) == capi.FFHIP_ENODEV


def test_python_pixels_argument():
    data = open(os.path.join(GOLDEN, "file_q85_420.jpg"), "rb").read()
    for bad in ("PIL", "", None, 1, "Libjpeg"):
        with pytest.raises(ValueError):
            tensors.decode_jpeg_to_tensors([data], pixels=bad)
        with pytest.raises(ValueError):
            ops.jpeg_decode_files_mixed_device([data], pixels=bad)
    for reduce in (2, 4, 8, "auto"):
        with pytest.raises(ValueError):
            tensors.decode_jpeg_to_tensors([data], pixels="libjpeg", reduce=reduce, size=(16, 16))
