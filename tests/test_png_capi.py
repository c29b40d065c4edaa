"""CPU: the host side of the PNG calls over all cases of png_cases.py -- the probe's fields, ffhip_png_picture against the witness, every
refusal of the pixel rule as FFHIP_EINVAL, the eXIf orientation -- the argument checks of the device and tensor entries (FFHIP_EINVAL before
FFHIP_ENODEV), and the stand-alone sanitizer program over the host decoder."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import png_cases
import png_spec
import png_writer as W
from ffpic_amd import capi, ops, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [c.name for c in png_cases.cases()]


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_probe_and_host_picture(k):
    c = png_cases.cases()[k]
    info, want = ops.png_probe(c.data), png_spec.layout(c.data)
    for field, v in want.items():
        got = getattr(info, field)
        assert (list(got) if hasattr(got, "__len__") else got) == v, field
    assert np.array_equal(ops.png_picture(c.data), png_cases.expected()[k])
    pitch = 4 * info.width + 12                                       # a pitch of its own: nothing behind a row's pixels is written
    L = capi.lib()
    out = np.full((info.height, pitch), 0xA5, np.uint8)
    buf = np.frombuffer(c.data, np.uint8)
    capi.check(L.ffhip_png_picture(buf.ctypes.data, buf.size, out.ctypes.data, pitch))
    assert np.array_equal(out[:, :4 * info.width].reshape(info.height, info.width, 4), png_cases.expected()[k])
    assert (out[:, 4 * info.width:] == 0xA5).all()


@pytest.mark.parametrize("name,data", png_cases.damaged(), ids=[n for n, _ in png_cases.damaged()])
def test_refusals(name, data):
    with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EINVAL)):
        ops.png_picture(data)
    header_only = name.startswith(("crc_ihdr", "depth_", "colour_", "compression", "filter_method", "interlace", "width_", "height_"))
    if header_only:                                                   # what the probe sees too
        with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EINVAL)):
            ops.png_probe(data)
    else:
        ops.png_probe(data)                                           # cheap: the header's CRC only


def test_extra_bytes_and_ignored_chunks():
    rng = np.random.default_rng(5)
    s = png_cases.random_samples(rng, 4, 6, 6, 8)
    raw = W.filtered_stream(s, 6, 8, [4, 1, 3, 2])
    want = W.expected_bgra(s, 6, 8)
    assert np.array_equal(ops.png_picture(W.write(s, 6, 8, stream=raw + b"\x07" * 40)), want)            # bytes beyond the filtered size
    junk = [W.chunk(b"gAMA", b"\x00\x01\x86\xa0"), W.chunk(b"sRGB", b"\x00", crc=1), W.chunk(b"bKGD", b"\x00" * 6), W.chunk(b"acTL", b"\x00" * 8)]
    data = W.write(s, 6, 8, filters=[4, 1, 3, 2], before_idat=junk, after_idat=[W.chunk(b"fdAT", b"\x00" * 9), W.chunk(b"tEXt", b"k\x00v", crc=0)])
    assert np.array_equal(ops.png_picture(data), want)                # ancillary chunks: skipped by length, their CRC not looked at
    with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EINVAL)):
        ops.png_picture(W.write(s, 6, 8, before_idat=[W.chunk(b"ABCD", b"")]))                            # a critical chunk nobody knows


def test_exif_orientation():
    s = np.zeros((2, 3, 3), np.int64)
    for o in range(1, 9):
        for big in (False, True):
            assert ops.png_exif_orientation(W.write(s, 2, 8, exif=W.exif_payload(o, big))) == o
    assert ops.png_exif_orientation(W.write(s, 2, 8, after_idat=[W.chunk(b"eXIf", W.exif_payload(6))])) == 6  # behind the picture
    assert ops.png_exif_orientation(W.write(s, 2, 8)) == 1
    good = W.write(s, 2, 8, exif=W.exif_payload(6))
    assert ops.png_exif_orientation(W.write(s, 2, 8, exif=W.exif_payload(9))) == 1
    assert ops.png_exif_orientation(W.write(s, 2, 8, exif=W.exif_payload(6)[:13])) == 1
    assert ops.png_exif_orientation(W.write(s, 2, 8, exif=b"XX" + W.exif_payload(6)[2:])) == 1
    for n in range(1, len(good)):                                     # any cut: 1 or the tag, never a failure
        assert ops.png_exif_orientation(good[:n]) in (1, 6)


def _file_args(files):
    bufs, ptrs, lens = ops.file_args(files)
    n = len(files)
    return bufs, ptrs, lens, (C.c_void_p * n)(*([16] * n)), (C.c_int64 * n)(*([64] * n)), (C.c_int * n)()


def test_device_entry_checks_arguments_before_the_device():
    L = capi.lib()
    files = [c.data for c in png_cases.cases()[:2]]
    bufs, ptrs, lens, outs, pitches, status = _file_args(files)
    call = L.ffhip_png_decode_files_device
    for bad in ((None, lens, 2, 1, outs, pitches, None, status, None), (ptrs, None, 2, 1, outs, pitches, None, status, None),
                (ptrs, lens, 2, 1, None, pitches, None, status, None), (ptrs, lens, 2, 1, outs, None, None, status, None),
                (ptrs, lens, 2, 1, outs, pitches, None, None, None), (ptrs, lens, -1, 1, outs, pitches, None, status, None)):
        assert call(*bad) == capi.FFHIP_EINVAL
    assert call(ptrs, lens, 0, 1, outs, pitches, None, status, None) == 0
    if L.ffhip_device_count() == 0:
        assert call(ptrs, lens, 2, 1, outs, pitches, None, status, None) == capi.FFHIP_ENODEV


def test_tensor_entry_checks_arguments_before_the_device():
    L = capi.lib()
    files = [c.data for c in png_cases.cases()[:2]]
    bufs, ptrs, lens, _, _, status = _file_args(files)
    fmt = tensors.tensor_format()
    outs = (capi.TensorOut * 2)(capi.TensorOut(16, 65, 65 * 130), capi.TensorOut(16, 65, 65 * 130))
    call = L.ffhip_png_decode_files_tensor
    good = [ptrs, lens, 2, 1, C.byref(fmt), outs, None, None, capi.FFHIP_RESIZE_BILINEAR, None, None, 0, None, status, None]

    def with_(at, v):
        a = list(good)
        a[at] = v
        return a

    for bad in (with_(0, None), with_(1, None), with_(4, None), with_(5, None), with_(13, None), with_(11, 1), with_(11, 0x10), with_(8, 7)):
        assert call(*bad) == capi.FFHIP_EINVAL
    assert call(*with_(2, 0)) == 0
    if L.ffhip_device_count() == 0:
        assert call(*good) == capi.FFHIP_ENODEV


def test_python_entries_exist_and_the_existing_entry_points_keep_their_names():
    assert callable(tensors.decode_png_to_tensors) and callable(ops.png_decode_files_device)
    assert tensors.entry_point("webp", True, 1, True) == "ffhip_webp_decode_files_tensor_oriented"
    assert tensors.webp_entry_point("libwebp") == "ffhip_webp_decode_files_tensor_ex"
    assert tensors.entry_point("jpeg", False, 2, True) == "ffhip_jpeg_decode_files_tensor_scaled"


def test_host_decoder_under_the_sanitizers(tmp_path):
    """tests/tools/png_host_asan_main.c: ffhip_inflate and ffhip_png_picture on every prefix and every single-byte change of four small
    files, into exact-size heap buffers, under -fsanitize=address,undefined.  A stand-alone program with the sanitizers' runtimes linked into it: nothing is preloaded or loaded into Python"""
    gcc = shutil.which("gcc") or "gcc"                                # the compiler the library's own C sources are built with
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "png_host_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, os.path.join(ROOT, "tests", "tools", "png_host_asan_main.c"), os.path.join(csrc, "ffhip_inflate.c"),
                           os.path.join(csrc, "ffhip_png.c"), "-o", exe, "-lpthread"])
    rng = np.random.default_rng(11)
    names = []
    for k, (ctype, depth, inter, how) in enumerate(((2, 8, False, dict(filters=[4, 3, 2, 1, 0])), (3, 2, True, dict(level=9)),
                                                    (6, 16, True, dict(strategy=zlib.Z_FIXED, idat_sizes=[1, 0, 5])), (0, 1, False, dict(level=0)))):
        pal = png_cases.random_palette(rng, 3) if ctype == 3 else None
        s = png_cases.random_samples(rng, 5, 6, ctype, depth, 3 if ctype == 3 else None)
        path = str(tmp_path / f"f{k}.png")
        with open(path, "wb") as f:
            f.write(W.write(s, ctype, depth, interlace=inter, palette=pal, **how))
        names.append(path)
    r = subprocess.run([exe] + names, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
