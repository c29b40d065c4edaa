"""CPU: the host entries of the JPEG encoder against the witness (tests/jpeg_encode_spec.py, itself held to PIL by
test_jpeg_encode_spec.py): tables, block, header and whole pictures through every source form; the bound against every case's real size;
the cap; every argument check of the device calls in front of their device check; the host C under the sanitizers as a program of its own."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_encode_spec as spec
from ffpic_amd import capi, ops
from jpeg_encode_cases import CASES, SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, NOSPACE = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV, capi.FFHIP_EJPEG_NOSPACE


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_tables_equal_the_witness(L):
    for q in range(-3, 104):
        assert np.array_equal(ops.jpeg_encode_tables(q), spec.tables(q)[:2]), q
    assert L.ffhip_jpeg_encode_tables(50, None) == EINVAL


def test_block_equals_the_witness(L):
    rng = np.random.default_rng(7)
    blocks = [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(200)]
    blocks += [(rng.integers(0, 2, 64, dtype=np.uint8) * 255).astype(np.uint8) for _ in range(100)]
    blocks += [np.zeros(64, np.uint8), np.full(64, 255, np.uint8), (np.indices((8, 8)).sum(0) % 2 * 255).astype(np.uint8).reshape(64),
               np.tile(np.array([0, 255], np.uint8), 32), np.repeat(np.array([255, 0], np.uint8), 32)]
    for k, b in enumerate(blocks):
        q = spec.tables((1, 50, 75, 100)[k % 4])[k % 2]
        want = spec.fdct_quant(b.reshape(1, 8, 8), q)[0]
        assert np.array_equal(ops.jpeg_encode_block(b, q), want), k
    assert max(abs(int(x)) for x in ops.jpeg_encode_block(blocks[-3], spec.tables(100)[0])) > 512     # an AC coefficient of size 10
    s, q, out = np.zeros(64, np.uint8), np.ones(64, np.uint16), np.zeros(64, np.int16)
    assert L.ffhip_jpeg_encode_block(None, q.ctypes.data, out.ctypes.data) == EINVAL
    assert L.ffhip_jpeg_encode_block(s.ctypes.data, None, out.ctypes.data) == EINVAL
    assert L.ffhip_jpeg_encode_block(s.ctypes.data, q.ctypes.data, None) == EINVAL
    q[5] = 0
    assert L.ffhip_jpeg_encode_block(s.ctypes.data, q.ctypes.data, out.ctypes.data) == EINVAL


@pytest.mark.parametrize("case", SMALL[::5] + CASES[-2:], ids=lambda c: c.id)
def test_header_equals_the_witness(L, case):
    data = case.key[2]
    head = ops.jpeg_encode_header(case.width, case.height, case.layout, case.quality, case.restart)
    assert len(head) <= capi.FFHIP_JPEG_ENC_HEADER_MAX and head[-3:] == b"\x00\x3f\x00" and data[:len(head)] == head
    n = C.c_size_t()
    out = np.full(len(head) + 8, 0xA5, np.uint8)
    assert L.ffhip_jpeg_encode_header(case.width, case.height, spec.LAYOUT_ID[case.layout], case.quality, case.restart, out.ctypes.data, len(head) - 1,
                                      C.byref(n)) == NOSPACE and n.value == len(head) and (out == 0xA5).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_picture_equals_the_witness_and_the_bound_holds(L, case):
    want = case.key[2]
    px = case.pixels
    assert ops.jpeg_encode_picture(px, case.layout, case.quality, case.restart) == want
    bound = ops.jpeg_encode_bound(case.width, case.height, case.layout, case.restart)
    assert len(want) <= bound
    if px.ndim == 3 and case.width * case.height < 10000:                       # the other source forms: planar, BGR through the strides, BGRA
        planar = np.ascontiguousarray(px.transpose(2, 0, 1)).transpose(1, 2, 0)
        assert ops.jpeg_encode_picture(planar, case.layout, case.quality, case.restart) == want
        bgr = np.ascontiguousarray(px[..., ::-1])[..., ::-1]
        assert bgr.strides[2] == -1 and ops.jpeg_encode_picture(bgr, case.layout, case.quality, case.restart) == want
        bgra = np.full((case.height, case.width + 3, 4), 0x5A, np.uint8)
        bgra[:, :case.width, :3] = px[..., ::-1]
        src = capi.jpeg_source(bgra.ctypes.data, case.width, case.height, bgra.strides[0], 4, channels=4)
        out, n = np.zeros(bound, np.uint8), C.c_size_t()
        assert L.ffhip_jpeg_encode_picture(C.byref(src), spec.LAYOUT_ID[case.layout], case.quality, case.restart, out.ctypes.data, bound, C.byref(n)) == 0
        assert out[:n.value].tobytes() == want


@pytest.mark.parametrize("case", SMALL[::7], ids=lambda c: c.id)
def test_a_cap_one_byte_short(L, case):
    want = case.key[2]
    px = np.ascontiguousarray(case.pixels)
    src = ops.jpeg_host_source(px)
    out, n = np.full(len(want) + 64, 0xA5, np.uint8), C.c_size_t()
    rc = L.ffhip_jpeg_encode_picture(C.byref(src), spec.LAYOUT_ID[case.layout], case.quality, case.restart, out.ctypes.data, len(want) - 1, C.byref(n))
    assert rc == NOSPACE and n.value == len(want)
    assert (out[len(want) - 1:] == 0xA5).all() and out[:len(want) - 1].tobytes() == want[:-1]


def test_the_bound_is_what_the_header_derives(L):
    """header + per interval 2 ceil(1660 blocks / 8) + 2; 0 for what the encoder refuses"""
    for (w, h, layout, r) in [(100, 75, "4:4:4", 0), (100, 75, "4:2:0", 3), (17, 13, "grey", 1), (65535, 65535, "4:2:2", 0), (40, 24, "4:2:2", 2)]:
        hh, vv, ncomp = spec.LAYOUTS[layout]
        mcus, bpm = -(-w // (8 * hh)) * -(-h // (8 * vv)), (hh * vv + 2 if ncomp == 3 else 1)
        per = r or mcus
        blocks = [per * bpm] * (mcus // per) + ([mcus % per * bpm] if mcus % per else [])
        want = len(ops.jpeg_encode_header(w, h, layout, 50, r)) + sum(2 * -(-1660 * b // 8) + 2 for b in blocks)
        assert ops.jpeg_encode_bound(w, h, layout, r) == want
    for bad in [(0, 8, 0, 0), (8, 0, 0, 0), (65536, 8, 0, 0), (8, 65536, 0, 0), (8, 8, 4, 0), (8, 8, -1, 0), (8, 8, 0, -1), (8, 8, 0, 65536)]:
        assert L.ffhip_jpeg_encode_bound(*bad) == 0, bad


A = 1 << 20            # fake, aligned "device" addresses: nothing is dereferenced in front of the device check


def _source(**kw):
    args = dict(pixels=A, width=40, height=24, row_stride=120, pixel_stride=3, chan=(0, 1, 2), channels=3)
    args.update(kw)
    return capi.jpeg_source(**args)


def _calls(L, src, layout=2, quality=75, restart=0, coef=(A, A + 4096, A + 8192), out=A, cap=4096, width=None, height=None, reserved=0, which=(1, 1, 1)):
    """the device calls on one item -> the return codes of (fdct, huff, encode), None for a call that `which` leaves out.  The addresses are
    fake: with a device present only a call that is refused in front of the device check may be made"""
    f = capi.JpegFdctItem()
    f.src, f.layout, f.quality = src, layout, quality
    f.d_coef_y, f.d_coef_u, f.d_coef_v = coef
    h = capi.JpegHuffItem()
    h.width, h.height, h.layout, h.quality, h.restart = src.width if width is None else width, src.height if height is None else height, layout, quality, restart
    h.d_coef_y, h.d_coef_u, h.d_coef_v, h.d_out, h.cap = *coef, out, cap
    e = capi.JpegEncodeItem()
    e.src, e.layout, e.quality, e.restart, e.reserved, e.d_out, e.cap = src, layout, quality, restart, reserved, out, cap
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    return (L.ffhip_jpeg_fdct_items(C.byref(f), 1, None) if which[0] else None,
            L.ffhip_jpeg_huff_encode_items(C.byref(h), 1, lens, status, None) if which[1] else None,
            L.ffhip_jpeg_encode_items(C.byref(e), 1, lens, status, None) if which[2] else None)


GREY = dict(layout=3, coef=(A, None, None))
# what -> (arguments, which of (fdct, huff, encode) must refuse it)
REFUSED = {
    "width 0": (dict(src=_source(width=0)), (1, 1, 1)),
    "width 65536": (dict(src=_source(width=65536)), (1, 1, 1)),
    "height 0": (dict(src=_source(height=0)), (1, 1, 1)),
    "height 65536": (dict(src=_source(height=65536)), (1, 1, 1)),
    "layout 4": (dict(src=_source(), layout=4), (1, 1, 1)),
    "layout -1": (dict(src=_source(), layout=-1), (1, 1, 1)),
    "restart -1": (dict(src=_source(), restart=-1), (0, 1, 1)),
    "restart 65536": (dict(src=_source(), restart=65536), (0, 1, 1)),
    "pixels NULL": (dict(src=_source(pixels=None)), (1, 0, 1)),
    "two channels": (dict(src=_source(channels=2)), (1, 0, 1)),
    "a grey source into a colour layout": (dict(src=_source(channels=1)), (1, 0, 1)),
    "a colour source into the grey layout": (dict(src=_source(), **GREY), (1, 0, 1)),
    "a BGRA source into the grey layout": (dict(src=_source(channels=4, pixel_stride=4, row_stride=160), **GREY), (1, 0, 1)),
    "BGRA with a pixel stride of 3": (dict(src=_source(channels=4)), (1, 0, 1)),
    "BGRA off 4 bytes": (dict(src=_source(channels=4, pixel_stride=4, row_stride=160, pixels=A + 2)), (1, 0, 1)),
    "BGRA with a pitch off 4": (dict(src=_source(channels=4, pixel_stride=4, row_stride=162)), (1, 0, 1)),
    "a reserved field set": (dict(src=_source(), reserved=1), (0, 0, 1)),
    "a stride of 2^30": (dict(src=_source(row_stride=1 << 30)), (1, 0, 1)),
    "a BGRA pitch of 2^30": (dict(src=_source(channels=4, pixel_stride=4, row_stride=1 << 30)), (1, 0, 1)),
    "a BGRA pitch of -2^30": (dict(src=_source(channels=4, pixel_stride=4, row_stride=-(1 << 30))), (1, 0, 1)),
    "luma plane NULL": (dict(src=_source(), coef=(None, A, A)), (1, 1, 0)),
    "luma plane misaligned": (dict(src=_source(), coef=(A + 8, A, A)), (1, 1, 0)),
    "chroma plane NULL": (dict(src=_source(), coef=(A, None, A)), (1, 1, 0)),
    "chroma plane misaligned": (dict(src=_source(), coef=(A, A, A + 2)), (1, 1, 0)),
    "chroma planes with the grey layout": (dict(src=_source(channels=1, pixel_stride=1, row_stride=40), layout=3), (1, 1, 0)),
    "a cap without an output": (dict(src=_source(), out=None), (0, 1, 1)),
    "a picture whose bound reaches 2^32": (dict(src=_source(width=20000, height=20000, row_stride=60000), layout=0), (0, 1, 1)),
}


@pytest.mark.parametrize("why", list(REFUSED))
def test_device_calls_refuse_in_front_of_the_device_check(L, why):
    """FFHIP_EINVAL with or without a device.  The calls the argument does not reach are well-formed calls on fake addresses: they are made
    only on a machine without a device, where they answer FFHIP_ENODEV as for good arguments"""
    kw, refused = REFUSED[why]
    have = L.ffhip_device_count() > 0
    got = _calls(L, which=refused if have else (1, 1, 1), **kw)
    for rc, bad in zip(got, refused):
        if bad:
            assert rc == EINVAL, (why, got)
        elif have:
            assert rc is None, (why, got)
        else:
            assert rc == ENODEV, (why, got)


def test_device_calls_reach_the_device_check_with_good_arguments(L):
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    for fn, kind in (("ffhip_jpeg_fdct_items", capi.JpegFdctItem), ("ffhip_jpeg_huff_encode_items", capi.JpegHuffItem), ("ffhip_jpeg_encode_items", capi.JpegEncodeItem)):
        tail = (None,) if kind is capi.JpegFdctItem else (lens, status, None)
        assert getattr(L, fn)(None, -1, *tail) == EINVAL and getattr(L, fn)(None, 1, *tail) == EINVAL
        if kind is not capi.JpegFdctItem:
            assert getattr(L, fn)(C.byref(kind()), 1, None, status, None) == EINVAL and getattr(L, fn)(C.byref(kind()), 1, lens, None, None) == EINVAL
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present; covered by the -m gpu tests")
    assert _calls(L, _source()) == (ENODEV,) * 3
    assert _calls(L, _source(channels=1, pixel_stride=1, row_stride=40), **GREY) == (ENODEV,) * 3
    assert _calls(L, _source(channels=4, pixel_stride=4, row_stride=160), layout=0, cap=0, out=None) == (ENODEV,) * 3
    assert _calls(L, _source(row_stride=-120, pixel_stride=-3, pixels=A + 4000)) == (ENODEV,) * 3       # negative strides are a source form


def test_host_encoder_clean_under_sanitizers(tmp_path):
    """tests/tools/jpeg_enc_asan_main.c with ffhip_jpeg_enc.c under -fsanitize=address,undefined: pictures in heap buffers of exactly their
    size into outputs of exactly cap bytes.  A stand-alone program with the sanitizers' runtimes linked into it: nothing is loaded into Python"""
    gcc = shutil.which("gcc") or "gcc"                                # the compiler the library's own C sources are built with
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "jpeg_enc_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "tools", "jpeg_enc_asan_main.c"), os.path.join(csrc, "ffhip_jpeg_enc.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 576"), r.stdout
