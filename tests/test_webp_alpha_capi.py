"""CPU: the host side of FFHIP_WEBP_ALPHA over all cases of webp_alpha_cases.py -- ffhip_webp_alpha_probe and ffhip_webp_alpha_plane against
the answer key and the witness, every refusal, nothing written for a refused file, the flag's rules on every call that takes `flags`
(FFHIP_EINVAL before FFHIP_ENODEV), and ffhip_vp8l_picture on its own goldens behind the split of ffhip_vp8l_open."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vp8l_cases
import webp_alpha_cases as K
import webp_alpha_spec as S
from ffpic_amd import capi, ops, tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_vp8l  # noqa: E402
import make_golden_webp_alpha as golden  # noqa: E402

CASE_IDS = [c.name for c in K.cases()]
BOTH = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_probe_and_host_plane(k):
    c = K.cases()[k]
    buf = np.frombuffer(c.data, np.uint8)
    if c.plane is None:
        assert ops.webp_alpha_probe(c.data) == (0, 0, 0, 0) and S.find(c.data) is None
        out = np.full(4096, 0xA5, np.uint8)
        assert capi.lib().ffhip_webp_alpha_plane(buf.ctypes.data, buf.size, out.ctypes.data, 64) == capi.FFHIP_EINVAL and (out == 0xA5).all()
        return
    h, w = c.plane.shape
    assert ops.webp_alpha_probe(c.data) == (1, c.compression, c.filter, c.pre)
    got = ops.webp_alpha_plane(c.data)
    assert np.array_equal(got, c.plane), np.argwhere(got != c.plane)[:4].tolist()
    assert np.array_equal(got, S.plane(c.data))
    pitch = w + 5                                                 # a pitch of its own: nothing behind a row's samples is written
    out = np.full((h, pitch), 0xA5, np.uint8)
    assert capi.lib().ffhip_webp_alpha_plane(buf.ctypes.data, buf.size, out.ctypes.data, pitch) == 0
    assert np.array_equal(out[:, :w], c.plane) and (out[:, w:] == 0xA5).all()


def test_host_plane_gives_the_goldens_alpha():
    for name, data, pixels in golden.load():
        assert np.array_equal(ops.webp_alpha_plane(data), pixels[..., 3]), name
        assert ops.webp_alpha_probe(data)[0] == 1, name


def test_refusals():
    L = capi.lib()
    v = [C.c_int() for _ in range(4)]
    for d in K.damaged_cases():
        buf = np.frombuffer(d.data, np.uint8)
        out = np.full(4096, 0xA5, np.uint8)                       # the damaged files are 7 x 5
        assert L.ffhip_webp_alpha_plane(buf.ctypes.data, buf.size, out.ctypes.data, 64) == capi.FFHIP_EINVAL, d.name
        assert (out == 0xA5).all() or d.name.startswith(("lossless", "one-symbol")), d.name   # a header refusal writes nothing
        assert L.ffhip_webp_alpha_probe(buf.ctypes.data, buf.size, *v) in (0, capi.FFHIP_EINVAL), d.name
        assert ops.webp_probe(d.data, "libwebp")[:2] == (7, 5), d.name                         # the colour stays decodable
    good = np.frombuffer(K.cases()[0].data, np.uint8)
    out = np.zeros(64, np.uint8)
    assert L.ffhip_webp_alpha_probe(None, 10, *v) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_alpha_probe(good.ctypes.data, good.size, None, v[1], v[2], v[3]) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_alpha_plane(good.ctypes.data, good.size, None, 64) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_alpha_plane(good.ctypes.data, good.size, out.ctypes.data, 0) == capi.FFHIP_EINVAL   # a pitch below the width
    assert L.ffhip_webp_alpha_probe(good.ctypes.data, 11, *v) == capi.FFHIP_EINVAL
    lossless = np.frombuffer(vp8l_cases.cases()[0].data, np.uint8)
    assert L.ffhip_webp_alpha_probe(lossless.ctypes.data, lossless.size, *v) == capi.FFHIP_EWEBP_LOSSLESS


def test_the_cut_stream_libwebp_accepts():
    f = K.lenient_end()
    assert np.array_equal(ops.webp_alpha_plane(f), S.plane(f))


def test_truncated_and_bit_flipped_copies_follow_the_witness():
    by = {c.name: c for c in K.cases()}
    stored = {n: d for n, d, _ in golden.load()}
    sources = [(n, by[n].data) for n in ("w17-h3-raw-f2", "predictor-f1", "palette-f2", "cache-f3", "palette-one-symbol-codes")]
    sources += [(n, stored[n]) for n in ("mask-17x9-m4-a100", "grad-17x9-m0-a100", "noise-3x5-m4-a50")]
    for name, data in K.mangled(sources):
        try:
            want = S.plane(data)
        except S.Refused:
            want = None
        try:
            got = ops.webp_alpha_plane(data)
        except capi.FfhipError as e:
            assert str(capi.FFHIP_EINVAL) in str(e), name
            got = None
        assert (got is None) == (want is None) and (got is None or np.array_equal(got, want)), name


def _file_args(files):
    bufs, ptrs, lens = ops.file_args(files)
    n = len(files)
    return bufs, ptrs, lens, (C.c_void_p * n)(*([16] * n)), (C.c_int64 * n)(*([64] * n)), (C.c_int * n)()


def test_flag_rules():
    L = capi.lib()
    files = [c.data for c in K.cases()[:2]]
    bufs, ptrs, lens, outs, pitches, status = _file_args(files)
    call = L.ffhip_webp_decode_files_device_ex
    for flags in (capi.FFHIP_WEBP_ALPHA, BOTH | 0x40, capi.FFHIP_WEBP_ALPHA | 1):   # without the libwebp bit; with an unknown bit
        assert call(ptrs, lens, 2, 1, outs, pitches, None, flags, None, status, None) == capi.FFHIP_EINVAL
    assert call(ptrs, lens, 0, 1, outs, pitches, None, BOTH, None, status, None) == 0
    assert call(None, lens, 2, 1, outs, pitches, None, BOTH, None, status, None) == capi.FFHIP_EINVAL
    if L.ffhip_device_count() == 0:                               # the argument errors above came first
        assert call(ptrs, lens, 2, 1, outs, pitches, None, BOTH, None, status, None) == capi.FFHIP_ENODEV
    buf = np.frombuffer(files[0], np.uint8)
    v = [C.c_int() for _ in range(4)]
    parsed, arrays = ops._webp_parsed(4)
    for flags in (capi.FFHIP_WEBP_ALPHA, BOTH):                   # every other call that takes flags refuses the bit
        assert L.ffhip_webp_probe_ex(buf.ctypes.data, buf.size, flags, *[C.byref(x) for x in v]) == capi.FFHIP_EINVAL
        assert L.ffhip_webp_parse_ex(buf.ctypes.data, buf.size, flags, C.byref(parsed)) == capi.FFHIP_EINVAL
        assert L.ffhip_webp_parse_device_ex(ptrs, lens, 2, flags, (capi.WebpParsed * 2)(parsed, parsed), status, None) == capi.FFHIP_EINVAL
        fmt = tensors.tensor_format()
        touts = (capi.TensorOut * 2)(capi.TensorOut(16, 1, 1), capi.TensorOut(16, 1, 7))
        assert L.ffhip_webp_decode_files_tensor_ex(ptrs, lens, 2, 1, C.byref(fmt), touts, None, None, capi.FFHIP_RESIZE_BILINEAR, None, None, flags, None,
                                                   status, None) == capi.FFHIP_EINVAL
    with pytest.raises(ValueError):
        ops.webp_decode_files_device(files, alpha=True)           # alpha=True needs pixels='libwebp'


def test_vp8l_picture_still_gives_its_goldens():
    for name, data, pixels in make_golden_vp8l.load():
        assert np.array_equal(ops.vp8l_picture(data), pixels), name
    for c, want in list(zip(vp8l_cases.cases(), vp8l_cases.expected()))[::7]:
        assert np.array_equal(ops.vp8l_picture(c.data), want), c.name


def test_python_entries_exist():
    assert callable(ops.webp_alpha_probe) and callable(ops.webp_alpha_plane) and callable(ops.webp_alpha_last) and callable(ops.webp_alpha_times)
    assert capi.FFHIP_WEBP_ALPHA == 0x20 and len(ops.webp_alpha_last()) == 4
    assert len(ops.webp_alpha_times()) == 4
