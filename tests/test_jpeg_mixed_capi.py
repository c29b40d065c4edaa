"""CPU: the argument checks of the mixed-batch entry points (ffhip_jpeg_recon_items, ffhip_jpeg_decode_files_mixed_device).
Every refusal is FFHIP_EINVAL whether or not a device is present; good arguments reach the device check (FFHIP_ENODEV here)."""
import ctypes as C
import os

import pytest

from ffpic_amd import capi

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
A = 1 << 20     # fake, 16-byte-aligned "device" addresses: nothing is dereferenced before the device check


@pytest.fixture(scope="module")
def L():
    return capi.lib()


@pytest.fixture
def no_gpu(L):
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present; covered by the -m gpu tests")
    return L


def item(mcu_cols=5, mcu_rows=3, ncomp=3, h=2, v=2, pitch=None, bgra=A + 4096, y=A, u=A + 1024, v_=A + 2048, q=A + 3072):
    it = capi.JpegItem()
    it.geom = capi.jpeg_geom(mcu_cols, mcu_rows, ncomp, h, v)
    it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, it.d_bgra = y, u if ncomp == 3 else None, v_ if ncomp == 3 else None, q, bgra
    it.pitch = mcu_cols * 8 * h * 4 if pitch is None else pitch
    return it


def call(L, items, n=None):
    arr = (capi.JpegItem * max(len(items), 1))(*items)
    return L.ffhip_jpeg_recon_items(arr, len(items) if n is None else n, None)


GOOD = [dict(), dict(h=1, v=1), dict(h=2, v=1), dict(h=1, v=2), dict(h=4, v=1), dict(h=1, v=4), dict(ncomp=1, h=1, v=1),
        dict(mcu_cols=1, mcu_rows=1), dict(mcu_cols=300, mcu_rows=2, h=1, v=1)]


@pytest.mark.parametrize("kw", GOOD)
def test_valid_items_reach_the_device_check(no_gpu, kw):
    L = no_gpu
    assert call(L, [item(**kw)]) == capi.FFHIP_ENODEV


def test_mixed_classes_and_sizes_reach_the_device_check(no_gpu):
    L = no_gpu
    assert call(L, [item(**kw) for kw in GOOD] + [item(pitch=5 * 64 + 1024)]) == capi.FFHIP_ENODEV


def test_empty_call_is_a_no_op(L):
    assert call(L, [], n=0) == 0
    assert L.ffhip_jpeg_recon_items(None, 0, None) == 0


BAD = {
    "pitch below 4 x coded width": dict(pitch=5 * 64 - 16),
    "pitch not a multiple of 16": dict(pitch=5 * 64 + 4),
    "pitch x 16 reaches 2^31": dict(pitch=1 << 27),
    "output misaligned": dict(bgra=A + 4104),
    "output NULL": dict(bgra=None),
    "luma plane misaligned": dict(y=A + 2),
    "chroma plane misaligned": dict(u=A + 1032),
    "quantiser misaligned": dict(q=A + 3080),
    "luma plane NULL": dict(y=None),
    "two-pass layout: grey with h*v > 1": dict(ncomp=1, h=2, v=2),
    "two-pass layout: h = 3": dict(h=3, v=1),
    "two-pass layout: v = 3": dict(h=1, v=3),
    "more than 4096 quads per row": dict(mcu_cols=4 * 4096 + 1, mcu_rows=1, pitch=(4 * 4096 + 1) * 64),
    "zero MCU columns": dict(mcu_cols=0),
    "h * v > 4": dict(h=4, v=2),
}


@pytest.mark.parametrize("why", list(BAD))
def test_refusals(L, why):
    assert call(L, [item(**BAD[why])]) == capi.FFHIP_EINVAL, why
    # one bad item refuses the whole call, wherever it stands
    assert call(L, [item(), item(h=1, v=1), item(**BAD[why])]) == capi.FFHIP_EINVAL, why


def test_chroma_planes_required_for_three_components(L):
    it = item()
    it.d_coef_u = None
    assert call(L, [it]) == capi.FFHIP_EINVAL


def test_negative_count(L):
    assert call(L, [item()], n=-1) == capi.FFHIP_EINVAL
    assert L.ffhip_jpeg_recon_items(None, 1, None) == capi.FFHIP_EINVAL


def _files(n):
    data = open(os.path.join(GOLDEN, "file_q85_420.jpg"), "rb").read()
    bufs = [C.create_string_buffer(data, len(data)) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(data)] * n)
    return bufs, ptrs, lens


def test_file_entry_refuses_null_arrays(L):
    n = 2
    bufs, ptrs, lens = _files(n)
    outs = (C.c_void_p * n)(A, A + (1 << 22))
    pitch = (C.c_int64 * n)(640 * 4, 640 * 4)
    status = (C.c_int * n)()
    geoms = (capi.JpegGeom * n)()
    f = L.ffhip_jpeg_decode_files_mixed_device
    assert f(None, lens, n, 2, outs, pitch, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, None, n, 2, outs, pitch, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, None, pitch, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, outs, None, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, n, 2, outs, pitch, geoms, None, None) == capi.FFHIP_EINVAL
    assert f(ptrs, lens, -1, 2, outs, pitch, geoms, status, None) == capi.FFHIP_EINVAL
    assert f(None, None, 0, 2, None, None, None, None, None) == 0


def test_file_entry_reports_geometries_then_no_device(no_gpu):
    L = no_gpu
    n = 2
    bufs, ptrs, lens = _files(n)
    outs = (C.c_void_p * n)(A, A + (1 << 22))
    pitch = (C.c_int64 * n)(640 * 4, 640 * 4)
    status = (C.c_int * n)()
    geoms = (capi.JpegGeom * n)()
    assert L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n, 2, outs, pitch, geoms, status, None) == capi.FFHIP_ENODEV
    assert list(status) == [0, 0]
    assert (geoms[1].mcu_cols, geoms[1].mcu_rows, geoms[1].ncomp, geoms[1].h, geoms[1].v) == (40, 30, 3, 2, 2)
    # a pitch the items kernels refuse is that file's refusal
    pitch[1] = 640 * 4 - 16
    assert L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n, 2, outs, pitch, geoms, status, None) == capi.FFHIP_ENODEV
    assert status[0] == 0 and status[1] == capi.FFHIP_EINVAL


def test_the_slots_arithmetic_on_the_cpu_under_the_sanitizers(tmp_path):
    """tests/tools/check_slots.cpp: ffhip_planes.h -- a chunk's planes and tables inside a slot's block for every chunk
    size up to the slot's, and the split of copy_out's rows over host threads.  A stand-alone program with the sanitizers' runtimes
    linked into it"""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "check_slots")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(root, "ffpic_amd", "csrc"),
                           os.path.join(root, "tests", "tools", "check_slots.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok: 525 blocks, "), r.stdout
