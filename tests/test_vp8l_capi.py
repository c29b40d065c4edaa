"""CPU: the host side of the lossless WebP calls over all cases of vp8l_cases.py -- the probe, the info and ffhip_vp8l_picture against the
answer key and against the golden's pixels, every refusal and its code, nothing written for a refused file, the argument checks of the
device and tensor entries (FFHIP_EINVAL before FFHIP_ENODEV), the existing WebP calls' unchanged answer, and the stand-alone sanitizer
program over the host decoder."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import vp8l_cases
import vp8l_writer as W
from ffpic_amd import capi, ops, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_vp8l as golden  # noqa: E402

CASE_IDS = [c.name for c in vp8l_cases.cases()]


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_probe_info_and_host_picture(k):
    c, want = vp8l_cases.cases()[k], vp8l_cases.expected()[k]
    h, w = c.argb.shape
    assert ops.vp8l_probe(c.data) == (w, h, int(c.alpha))
    info = ops.vp8l_info(c.data)
    assert (info.width, info.height, info.has_alpha) == (w, h, int(c.alpha))
    assert tuple(info.transforms[:info.n_transforms]) == c.types and (info.cache_bits, info.has_meta) == (c.cache_bits, int(c.meta))
    assert info.residual_width == -(-w // info.pixels_per_word) and (info.pixels_per_word > 1) == (info.palette_size in range(1, 17))
    assert np.array_equal(ops.vp8l_picture(c.data), want)
    pitch = 4 * w + 12                                            # a pitch of its own: nothing behind a row's pixels is written
    buf = np.frombuffer(c.data, np.uint8)
    out = np.full((h, pitch), 0xA5, np.uint8)
    assert capi.lib().ffhip_vp8l_picture(buf.ctypes.data, buf.size, out.ctypes.data, pitch) == 0
    assert np.array_equal(out[:, :4 * w].reshape(h, w, 4), want) and (out[:, 4 * w:] == 0xA5).all()


def test_host_picture_gives_the_goldens_pixels():
    for name, data, pixels in golden.load():
        assert np.array_equal(ops.vp8l_picture(data), pixels), name


def test_refusals_and_their_codes():
    L = capi.lib()
    for d in vp8l_cases.damaged_cases():
        buf = np.frombuffer(d.data, np.uint8)
        out = np.full(16384, 0xA5, np.uint8)                      # the damaged files are 5 x 4 or smaller
        rc = L.ffhip_vp8l_picture(buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, 64)
        assert rc == d.code, d.name
        assert (out == 0xA5).all(), d.name                        # a refused file writes nothing
        info = capi.Vp8lInfo()
        assert L.ffhip_vp8l_read_info(buf.ctypes.data if buf.size else None, buf.size, C.byref(info)) in (0, d.code), d.name
    w, h, a = C.c_int(), C.c_int(), C.c_int()
    good = np.frombuffer(vp8l_cases.cases()[0].data, np.uint8)
    assert L.ffhip_vp8l_probe(None, 10, w, h, a) == capi.FFHIP_EINVAL and L.ffhip_vp8l_probe(good.ctypes.data, good.size, None, h, a) == capi.FFHIP_EINVAL
    assert L.ffhip_vp8l_picture(good.ctypes.data, good.size, None, 64) == capi.FFHIP_EINVAL
    out = np.zeros(64, np.uint8)
    assert L.ffhip_vp8l_picture(good.ctypes.data, good.size, out.ctypes.data, 3) == capi.FFHIP_EINVAL   # a pitch below 4 x width


def test_existing_webp_calls_still_answer_lossless():
    for c in vp8l_cases.cases()[:3]:
        with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EWEBP_LOSSLESS)):
            ops.webp_probe(c.data)
        with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EWEBP_LOSSLESS)):
            ops.webp_probe(c.data, "libwebp")
    assert "vp8l" in capi.lib().ffhip_strerror(capi.FFHIP_EWEBP_LOSSLESS).decode().lower()


def test_exif_orientation_of_a_lossless_file():
    by = {c.name: c for c in vp8l_cases.cases()}
    assert ops.webp_exif_orientation(by["exif-6"].data) == 6 and ops.webp_exif_orientation(by["size-5x7"].data) == 1


def _file_args(files):
    bufs, ptrs, lens = ops.file_args(files)
    n = len(files)
    return bufs, ptrs, lens, (C.c_void_p * n)(*([16] * n)), (C.c_int64 * n)(*([64] * n)), (C.c_int * n)()


def test_device_entry_checks_arguments_before_the_device():
    L = capi.lib()
    files = [c.data for c in vp8l_cases.cases()[:2]]
    bufs, ptrs, lens, outs, pitches, status = _file_args(files)
    call = L.ffhip_vp8l_decode_files_device
    for bad in ((None, lens, 2, 1, outs, pitches, None, status, None), (ptrs, None, 2, 1, outs, pitches, None, status, None),
                (ptrs, lens, 2, 1, None, pitches, None, status, None), (ptrs, lens, 2, 1, outs, None, None, status, None),
                (ptrs, lens, 2, 1, outs, pitches, None, None, None), (ptrs, lens, -1, 1, outs, pitches, None, status, None)):
        assert call(*bad) == capi.FFHIP_EINVAL
    assert call(ptrs, lens, 0, 1, outs, pitches, None, status, None) == 0
    if L.ffhip_device_count() == 0:
        assert call(ptrs, lens, 2, 1, outs, pitches, None, status, None) == capi.FFHIP_ENODEV


def test_tensor_entry_checks_arguments_before_the_device():
    L = capi.lib()
    files = [c.data for c in vp8l_cases.cases()[:2]]
    bufs, ptrs, lens, _, _, status = _file_args(files)
    fmt = tensors.tensor_format()
    outs = (capi.TensorOut * 2)(capi.TensorOut(16, 1, 1), capi.TensorOut(16, 1, 7))
    call = L.ffhip_vp8l_decode_files_tensor
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
    assert callable(tensors.decode_webp_lossless_to_tensors) and callable(ops.vp8l_decode_files_device)
    assert callable(ops.vp8l_last) and callable(ops.vp8l_times) and callable(ops.vp8l_probe) and callable(ops.vp8l_picture)
    assert tensors.entry_point("webp", True, 1, True) == "ffhip_webp_decode_files_tensor_oriented"
    assert tensors.webp_entry_point("libwebp") == "ffhip_webp_decode_files_tensor_ex"
    assert tensors.entry_point("jpeg", False, 2, True) == "ffhip_jpeg_decode_files_tensor_scaled"
    assert callable(tensors.decode_png_to_tensors)


def test_host_decoder_under_the_sanitizers(tmp_path):
    """tests/tools/vp8l_host_asan_main.c: ffhip_vp8l_probe, _read_info and _picture on every prefix and every single-byte change of four small
    files, into exact-size heap buffers, under -fsanitize=address,undefined.  A stand-alone program with the sanitizers' runtimes linked
    into it: nothing is preloaded or loaded into Python"""
    gcc = shutil.which("gcc") or "gcc"                                # the compiler the library's own C sources are built with
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "vp8l_host_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "tools", "vp8l_host_asan_main.c"),
                           os.path.join(csrc, "ffhip_vp8l.c"), "-o", exe])
    by = {c.name: c for c in vp8l_cases.cases()}
    names = []
    for k, name in enumerate(("size-5x7", "palette-16-all-steps", "meta-three-groups", "cache-4")):   # every transform, a meta image, a cache, copies
        path = str(tmp_path / f"f{k}.bin")
        with open(path, "wb") as f:
            f.write(by[name].data)
        names.append(path)
    r = subprocess.run([exe] + names, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
