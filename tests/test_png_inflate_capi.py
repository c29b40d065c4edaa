"""CPU: the argument checks of the three entries of "PNG, inflate on the device" (FFHIP_EINVAL before FFHIP_ENODEV, unknown png_flags
refused, n == 0 accepted), the Python names, and the stand-alone sanitizer program over the host model of k_inflate."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import inflate_cases as IC
import png_cases
from ffpic_amd import capi, ops, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_streams_entry_checks_arguments_before_the_device():
    L = capi.lib()
    z = IC.valid()["fixed"][0]
    buf = (C.c_char * len(z)).from_buffer_copy(z)
    src, lens = (C.c_void_p * 2)(C.addressof(buf), C.addressof(buf)), (C.c_size_t * 2)(len(z), len(z))
    dst, caps = (C.c_void_p * 2)(4096, 8192), (C.c_size_t * 2)(16, 16)
    got, status = (C.c_size_t * 2)(), (C.c_int * 2)()
    call = L.ffhip_inflate_streams_device
    good = [src, lens, 2, dst, caps, got, status, None]
    for at in (0, 1, 3, 4, 5, 6):
        bad = list(good)
        bad[at] = None
        assert call(*bad) == capi.FFHIP_EINVAL, at
    assert call(src, lens, -1, dst, caps, got, status, None) == capi.FFHIP_EINVAL
    assert call((C.c_void_p * 2)(C.addressof(buf), None), lens, 2, dst, caps, got, status, None) == capi.FFHIP_EINVAL   # bytes nowhere
    assert call(src, lens, 2, (C.c_void_p * 2)(4096, None), caps, got, status, None) == capi.FFHIP_EINVAL               # room nowhere
    assert call(src, lens, 0, dst, caps, got, status, None) == 0
    assert call(None, None, 0, None, None, None, None, None) == 0
    if L.ffhip_device_count() == 0:
        assert call(*good) == capi.FFHIP_ENODEV
        assert call(src, lens, 2, (C.c_void_p * 2)(4096, None), (C.c_size_t * 2)(16, 0), got, status, None) == capi.FFHIP_ENODEV  # no room asked for


def _file_args(files):
    bufs, ptrs, lens = ops.file_args(files)
    n = len(files)
    return bufs, ptrs, lens, (C.c_void_p * n)(*([16] * n)), (C.c_int64 * n)(*([64] * n)), (C.c_int * n)()


@pytest.mark.parametrize("png_flags", [0, capi.FFHIP_PNG_INFLATE_DEVICE])
def test_device_ex_entry_checks_arguments_before_the_device(png_flags):
    L = capi.lib()
    files = [c.data for c in png_cases.cases()[:2]]
    bufs, ptrs, lens, outs, pitches, status = _file_args(files)
    call = L.ffhip_png_decode_files_device_ex
    good = [ptrs, lens, 2, 1, outs, pitches, None, status, png_flags, None]
    for at in (0, 1, 4, 5, 7):
        bad = list(good)
        bad[at] = None
        assert call(*bad) == capi.FFHIP_EINVAL, at
    assert call(ptrs, lens, -1, 1, outs, pitches, None, status, png_flags, None) == capi.FFHIP_EINVAL
    for unknown in (2, 0x10, 0x80000000, png_flags | 4):
        assert call(ptrs, lens, 2, 1, outs, pitches, None, status, unknown, None) == capi.FFHIP_EINVAL
        assert call(ptrs, lens, 0, 1, outs, pitches, None, status, unknown, None) == capi.FFHIP_EINVAL
    assert call(ptrs, lens, 0, 1, outs, pitches, None, status, png_flags, None) == 0
    if L.ffhip_device_count() == 0:
        assert call(*good) == capi.FFHIP_ENODEV


@pytest.mark.parametrize("png_flags", [0, capi.FFHIP_PNG_INFLATE_DEVICE])
def test_tensor_ex_entry_checks_arguments_before_the_device(png_flags):
    L = capi.lib()
    files = [c.data for c in png_cases.cases()[:2]]
    bufs, ptrs, lens, _, _, status = _file_args(files)
    fmt = tensors.tensor_format()
    outs = (capi.TensorOut * 2)(capi.TensorOut(16, 65, 65 * 130), capi.TensorOut(16, 65, 65 * 130))
    call = L.ffhip_png_decode_files_tensor_ex
    good = [ptrs, lens, 2, 1, C.byref(fmt), outs, None, None, capi.FFHIP_RESIZE_BILINEAR, None, None, 0, None, png_flags, None, status, None]

    def with_(at, v):
        a = list(good)
        a[at] = v
        return a

    for bad in (with_(0, None), with_(1, None), with_(4, None), with_(5, None), with_(15, None), with_(11, 1), with_(11, 0x10), with_(8, 7),
                with_(13, 2), with_(13, png_flags | 0x10), with_(2, -1)):
        assert call(*bad) == capi.FFHIP_EINVAL
    assert call(*with_(2, 0)) == 0
    if L.ffhip_device_count() == 0:
        assert call(*good) == capi.FFHIP_ENODEV


def test_diagnostics_entry_and_python_names():
    assert capi.lib().ffhip_debug_png_inflate(None) == capi.FFHIP_EINVAL
    assert len(ops.png_inflate_last()) == 4
    assert capi.FFHIP_PNG_INFLATE_DEVICE == 1
    assert ops.png_inflate_flags("host") == 0 and ops.png_inflate_flags("device") == capi.FFHIP_PNG_INFLATE_DEVICE
    for call in (lambda: ops.png_inflate_flags("gpu"), lambda: ops.png_decode_files_device([], inflate="both"),
                 lambda: tensors.decode_png_to_tensors([], inflate=None)):
        with pytest.raises(ValueError):
            call()
    assert callable(ops.inflate_streams_device) and callable(ops.inflate_model) and callable(ops.inflate_upto)
    # the names the entry-point functions gave before there was the keyword
    assert tensors.alpha_entry_point("png") == "ffhip_png_decode_files_tensor"
    assert tensors.alpha_entry_point("png", "straight") == "ffhip_png_decode_files_tensor_alpha"
    assert tensors.entry_point("webp", True, 1, True) == "ffhip_webp_decode_files_tensor_oriented"
    assert tensors.entry_point("jpeg", False, 2, True) == "ffhip_jpeg_decode_files_tensor_scaled"


def test_model_under_the_sanitizers(tmp_path):
    """tests/tools/inflate_model_asan_main.c: ffhip_inflate_model on every proper prefix and every single-bit flip of the damaged set's
    stream, into heap buffers of exactly cap bytes, under -fsanitize=address,undefined, every verdict against ffhip_inflate_upto's.  A
    stand-alone program with the sanitizers' runtimes linked into it: nothing is preloaded or loaded into Python"""
    gcc = shutil.which("gcc") or "gcc"
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "inflate_model_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "tools", "inflate_model_asan_main.c"),
                           os.path.join(csrc, "ffhip_inflate_model.c"), os.path.join(csrc, "ffhip_inflate.c"), "-o", exe])
    z, _, bad = IC.damaged()
    path = str(tmp_path / "stream.z")
    with open(path, "wb") as f:
        f.write(z)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"ok: {len(bad)} streams"
