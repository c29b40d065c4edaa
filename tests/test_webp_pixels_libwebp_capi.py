"""The C entries of pixels='libwebp' through ctypes, without a GPU: every new entry refuses unknown flag bits and NULLs with FFHIP_EINVAL,
good arguments get FFHIP_ENODEV where there is no device, and with flags == 0 the _ex probe and parse return what the plain ones return."""
import ctypes as C

import numpy as np
import pytest

from ffpic_amd import capi, ops, tensors
from test_webp_front_capi import NAMES as FIXTURES, file_bytes
from webp_pixels_cases import CORPUS, data_of

EINVAL, ENODEV, LIBWEBP = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV, capi.FFHIP_WEBP_PIXELS_LIBWEBP
BAD_FLAGS = [0x1, 0x20, 0x11, 0x80000000, 0xffffffff]


def _buf(data):
    return np.frombuffer(data, dtype=np.uint8)


def test_exports_and_flag_value():
    L = capi.lib()
    assert LIBWEBP == 0x10
    for name in ("ffhip_webp_probe_ex", "ffhip_webp_parse_ex", "ffhip_webp_parse_device_ex", "ffhip_webp_decode_files_device_ex",
                 "ffhip_webp_decode_files_tensor_ex", "ffhip_vp8_libwebp_residual_mb", "ffhip_webp_libwebp_color"):
        assert name in capi.EXPORTS and hasattr(L, name), name


def test_probe_and_parse_ex_arguments():
    L = capi.lib()
    b = _buf(data_of(CORPUS[0]))
    v = [C.c_int() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    for flags in BAD_FLAGS:
        assert L.ffhip_webp_probe_ex(b.ctypes.data, b.size, flags, *refs) == EINVAL
    assert L.ffhip_webp_probe_ex(None, b.size, LIBWEBP, *refs) == EINVAL
    assert L.ffhip_webp_probe_ex(b.ctypes.data, b.size, LIBWEBP, None, None, None, None) == 0        # any output may be NULL
    assert L.ffhip_webp_probe_ex(b.ctypes.data, 11, LIBWEBP, *refs) == EINVAL
    p, keep = ops._webp_parsed(64)
    for flags in BAD_FLAGS:
        assert L.ffhip_webp_parse_ex(b.ctypes.data, b.size, flags, C.byref(p)) == EINVAL
    assert L.ffhip_webp_parse_ex(None, b.size, LIBWEBP, C.byref(p)) == EINVAL
    assert L.ffhip_webp_parse_ex(b.ctypes.data, b.size, LIBWEBP, None) == EINVAL
    for field in ("modes", "levels", "mbinfo", "resmap"):
        q, keep2 = ops._webp_parsed(64)
        setattr(q, field, None)
        assert L.ffhip_webp_parse_ex(b.ctypes.data, b.size, LIBWEBP, C.byref(q)) == EINVAL, field
    big = _buf(data_of("pil_noise_64x48_q60_m6"))
    q, keep2 = ops._webp_parsed(11)                               # room for fewer macroblocks than the file has
    assert L.ffhip_webp_parse_ex(big.ctypes.data, big.size, LIBWEBP, C.byref(q)) == EINVAL
    assert L.ffhip_webp_parse_ex(b.ctypes.data, b.size, LIBWEBP, C.byref(p)) == 0


def test_verdicts_stay():
    """lossless, animated and inter-frame files keep their codes under the rule"""
    riff = lambda body: b"RIFF" + (4 + len(body)).to_bytes(4, "little") + b"WEBP" + body
    v = [C.c_int() for _ in range(4)]
    L = capi.lib()

    def code(data):
        b = _buf(data)
        return L.ffhip_webp_probe_ex(b.ctypes.data, b.size, LIBWEBP, *[C.byref(x) for x in v])
    assert code(riff(b"VP8L" + (8).to_bytes(4, "little") + bytes(8))) == capi.FFHIP_EWEBP_LOSSLESS
    assert code(riff(b"ANIM" + (6).to_bytes(4, "little") + bytes(6))) == capi.FFHIP_EWEBP_ANIMATION
    assert code(riff(b"VP8X" + (10).to_bytes(4, "little") + bytes([2]) + bytes(9))) == capi.FFHIP_EWEBP_ANIMATION
    good = bytearray(data_of(CORPUS[0]))
    at = good.index(b"VP8 ") + 8
    good[at] |= 1
    assert code(bytes(good)) == capi.FFHIP_EWEBP_INTER_FRAME
    # an ALPH chunk of any size in front of the frame: the colour decodes
    plain = data_of("pil_noise_16x16_q100_m4")
    with_alpha = riff(b"ALPH" + (5).to_bytes(4, "little") + bytes(5) + b"\x00" + plain[12:])
    assert code(with_alpha) == 0 and (v[0].value, v[1].value) == (16, 16)
    a, b = ops.webp_parse(with_alpha, pixels="libwebp"), ops.webp_parse(plain, pixels="libwebp")
    assert np.array_equal(a["levels"], b["levels"]) and np.array_equal(a["modes"], b["modes"])


def test_host_bodies_arguments():
    L = capi.lib()
    lv, q, res, nz = np.zeros((25, 16), np.int16), np.full(6, 8, np.uint16), np.zeros((24, 16), np.int16), C.c_int()
    args = [lv.ctypes.data, 1, q.ctypes.data, res.ctypes.data, C.byref(nz)]
    assert L.ffhip_vp8_libwebp_residual_mb(*args) == 0
    for k in (0, 2, 3, 4):
        bad = list(args)
        bad[k] = None
        assert L.ffhip_vp8_libwebp_residual_mb(*bad) == EINVAL, k
    y, u, out = np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((4, 24), np.uint8)
    good = [y.ctypes.data, 6, u.ctypes.data, u.ctypes.data, 3, 6, 4, out.ctypes.data, 24]
    assert L.ffhip_webp_libwebp_color(*good) == 0
    for k, val in ((0, None), (2, None), (3, None), (7, None), (1, 5), (4, 2), (8, 23), (5, 0), (6, 0), (5, 16385)):
        bad = list(good)
        bad[k] = val
        assert L.ffhip_webp_libwebp_color(*bad) == EINVAL, (k, val)


def test_device_entries_check_arguments_before_the_device():
    L = capi.lib()
    data = data_of("pil_noise_16x16_q100_m4")
    bufs, ptrs, lens = ops.file_args([data])
    status = (C.c_int * 1)()
    outs = (C.c_void_p * 1)(0x1000)
    pitch = (C.c_int64 * 1)(64)
    planes = (C.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    p, keep = ops._webp_parsed(4)
    parsed = (capi.WebpParsed * 1)(p)
    for flags in BAD_FLAGS:
        assert L.ffhip_webp_parse_device_ex(ptrs, lens, 1, flags, parsed, status, None) == EINVAL
        assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, None, flags, None, status, None) == EINVAL
    assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, planes, 0, None, status, None) == EINVAL   # planes need the rule
    assert L.ffhip_webp_parse_device_ex(ptrs, lens, -1, LIBWEBP, parsed, status, None) == EINVAL
    for k in (0, 1, 4, 5):
        bad = [ptrs, lens, 1, LIBWEBP, parsed, status, None]
        bad[k] = None
        assert L.ffhip_webp_parse_device_ex(*bad) == EINVAL, k
    for k in (0, 1, 4, 5, 9):
        bad = [ptrs, lens, 1, 1, outs, pitch, None, LIBWEBP, None, status, None]
        bad[k] = None
        assert L.ffhip_webp_decode_files_device_ex(*bad) == EINVAL, k
    assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 0, 1, None, None, None, LIBWEBP, None, None, None) == 0
    if L.ffhip_device_count() == 0:                     # good arguments, no device
        assert L.ffhip_webp_parse_device_ex(ptrs, lens, 1, LIBWEBP, parsed, status, None) == ENODEV
        assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, None, LIBWEBP, None, status, None) == ENODEV
        assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, planes, LIBWEBP, None, status, None) == ENODEV
        assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, None, 0, None, status, None) == ENODEV
        pitch[0] = 48                                       # a pitch below 64 * mbcols is that file's EINVAL, found before the device is asked for
        assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, 1, 1, outs, pitch, None, LIBWEBP, None, status, None) == ENODEV and status[0] == EINVAL


def test_tensor_ex_checks_arguments_before_the_device():
    """good arguments but for the one under test: a valid format (uint8, scale 1, bias 0) and a valid output, so that nothing but the flag bit
    or the missing pointer can be what is refused"""
    L = capi.lib()
    data = data_of("pil_noise_16x16_q100_m4")
    bufs, ptrs, lens = ops.file_args([data])
    status = (C.c_int * 1)()
    fmt = tensors.tensor_format()
    touts = (capi.TensorOut * 1)(capi.TensorOut(0x10000, 16, 256))           # [3][16][16] uint8, dense
    size = (capi.Size * 1)(capi.Size(8, 8))
    turn, turned = (C.c_int * 1)(6), (C.c_int * 1)()

    def call(flags, **kw):
        a = dict(files=ptrs, lens=lens, n=1, fmt=C.byref(fmt), outs=touts, size=None, orient=None, status=status)
        a.update(kw)
        return L.ffhip_webp_decode_files_tensor_ex(a["files"], a["lens"], a["n"], 2, a["fmt"], a["outs"], None, a["size"], capi.FFHIP_RESIZE_ANTIALIAS, a["orient"],
                                                   turned if a["orient"] else None, flags, None, a["status"], None)
    for flags in BAD_FLAGS:
        assert call(flags) == EINVAL, hex(flags)
        assert call(flags, size=size, orient=turn) == EINVAL, hex(flags)
    for flags in (0, LIBWEBP):
        for missing in ("files", "lens", "fmt", "outs", "status"):
            assert call(flags, **{missing: None}) == EINVAL, (flags, missing)
        assert call(flags, n=-1) == EINVAL
        assert call(flags, orient=(C.c_int * 1)(9)) == EINVAL
        bad_fmt = tensors.tensor_format()
        bad_fmt.scale[0] = 2.0                                              # uint8 takes scale 1 only
        assert call(flags, fmt=C.byref(bad_fmt)) == EINVAL
        assert L.ffhip_webp_decode_files_tensor_ex(None, None, 0, 2, C.byref(fmt), None, None, None, capi.FFHIP_RESIZE_ANTIALIAS, None, None, flags, None, None, None) == 0
        if L.ffhip_device_count() == 0:                 # good arguments: the file is probed (and accepted), then the device is missed
            status[0] = -1
            assert call(flags) == ENODEV and status[0] == 0
            assert call(flags, size=size, orient=turn) == ENODEV


def test_the_diagnostic_entries_check_arguments():
    L = capi.lib()
    it = capi.Vp8Item()
    it.mbcols, it.mbrows, it.filter_type = 1, 1, 0
    it.d_modes, it.d_levels, it.d_mbinfo, it.d_bgra, it.pitch = 0x1000, 0x2000, 0x3000, 0x4000, 64
    items, display = (capi.Vp8Item * 1)(it), (capi.Size * 1)(capi.Size(16, 16))
    assert L.ffhip_debug_vp8_decode_items_libwebp(items, 0, display, None) == 0
    assert L.ffhip_debug_vp8_decode_items_libwebp(None, 1, display, None) == EINVAL
    assert L.ffhip_debug_vp8_decode_items_libwebp(items, 1, None, None) == EINVAL
    assert L.ffhip_debug_vp8_decode_items_libwebp(items, -1, display, None) == EINVAL
    for w, h in ((0, 16), (16, 0), (17, 16), (16, 17)):                 # the picture lies inside its macroblock grid
        assert L.ffhip_debug_vp8_decode_items_libwebp(items, 1, (capi.Size * 1)(capi.Size(w, h)), None) == EINVAL, (w, h)
    for field, val in (("d_levels", None), ("d_resmap", 0x5000), ("d_residual", 0x6000), ("pitch", 48), ("d_bgra", 0x4004), ("filter_type", 3)):
        bad = capi.Vp8Item.from_buffer_copy(it)
        setattr(bad, field, val)
        assert L.ffhip_debug_vp8_decode_items_libwebp((capi.Vp8Item * 1)(bad), 1, display, None) == EINVAL, field
    good = [0x1000, 0x2000, 0x3000, 16, 8, 16, 16, 1, 256, 64, 0x4000, 64, 1024, None]
    assert L.ffhip_debug_vp8_upsample_color(*(good[:7] + [0] + good[8:])) == 0
    for k, val in ((0, None), (1, None), (2, None), (10, None), (0, 0x1002), (3, 18), (3, 12), (4, 6), (4, 4), (5, 0), (6, 0), (5, 16385), (10, 0x4008),
                   (11, 60), (11, 72), (7, -1)):
        bad = list(good)
        bad[k] = val
        assert L.ffhip_debug_vp8_upsample_color(*bad) == EINVAL, (k, val)
    if L.ffhip_device_count() == 0:
        assert L.ffhip_debug_vp8_decode_items_libwebp(items, 1, display, None) == ENODEV
        assert L.ffhip_debug_vp8_upsample_color(*good) == ENODEV


@pytest.mark.parametrize("name", FIXTURES)
def test_flags_zero_is_the_plain_call(name):
    L = capi.lib()
    data = file_bytes(name)
    b = _buf(data)
    va, vb = [C.c_int() for _ in range(4)], [C.c_int() for _ in range(4)]
    ra = L.ffhip_webp_probe(b.ctypes.data, b.size, *[C.byref(x) for x in va])
    rb = L.ffhip_webp_probe_ex(b.ctypes.data, b.size, 0, *[C.byref(x) for x in vb])
    assert ra == rb and [x.value for x in va] == [x.value for x in vb]
    if ra:
        return
    n_mb = va[2].value * va[3].value
    pa, ka = ops._webp_parsed(n_mb)
    pb, kb = ops._webp_parsed(n_mb)
    assert L.ffhip_webp_parse(b.ctypes.data, b.size, C.byref(pa)) == L.ffhip_webp_parse_ex(b.ctypes.data, b.size, 0, C.byref(pb))
    for key in ka:
        assert np.array_equal(ka[key], kb[key]), key
    assert bytes(pa.info) == bytes(pb.info)
