"""CPU: the host PNG encoder (ffhip_png_filter_picture, ffhip_png_encode_picture) against the numpy witness
(tests/png_encode_spec.py), PIL, the PNG witness of the decoder (tests/png_spec.py) and the library's own host decoder: the filtered bytes
through every source form, the files' pixels, chunks, CRCs and bounds, the argument checks, the size conditions, and both host encoders in a
stand-alone program under the sanitizers.  Also the part loop of the device entry points (ffhip_parts.h), in a stand-alone program."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_encode_spec as spec
import png_spec
from ffpic_amd import capi, ops
from png_encode_cases import CASES, CHUNK, FORMS, source_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in CASES]
KEYS = {}


def key(case):
    """(the witness's filtered bytes, row types, row sums, the host entry's file) of a case, made once"""
    if case.id not in KEYS:
        KEYS[case.id] = spec.filtered(case.samples, case.filter) + (ops.png_encode_picture(case.samples, case.filter),)
    return KEYS[case.id]


def host_source(case, form):
    host, off, row, pixel, chan = source_form(case.samples, form)
    return host, capi.png_source(host.ctypes.data + off, case.width, case.height, row, pixel, chan)


def test_the_witness_sees_a_tie_and_all_five_types():
    by_id = {c.id: c for c in CASES}
    _, types, sums = spec.filtered(by_id["tie"].samples)
    row = sums[1]
    assert sorted(row)[0] == sorted(row)[1] and types[1] == int(np.flatnonzero(row == row.min())[0]) and (row == row.min()).sum() >= 2
    for name in ("all-five-1", "all-five-3"):
        _, types, _ = spec.filtered(by_id[name].samples)
        assert set(types) == {0, 1, 2, 3, 4}, (name, types)
    ups = spec.filtered(by_id["17x33x1-vstripes-b"].samples)[1]
    subs = spec.filtered(by_id["100x64x3-hstripes-b"].samples)[1]
    assert set(ups[1:]) == {2} and subs[0] == 1 and subs.count(1) >= len(subs) // 2 and set(subs) <= {1, 4}   # Paeth beats Sub where the pixel above is nearer


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filter_picture_equals_the_witness_in_every_form(case):
    want = key(case)[0]
    assert len(want) == ops.png_filtered_size(case.width, case.height, case.channels)
    for form in FORMS:
        host, src = host_source(case, form)
        assert ops.png_filter_picture(src, case.filter) == want, form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_files_chunks_stream_and_pixels(case):
    want, _, _, f = key(case)
    assert len(f) <= ops.png_encode_bound(case.width, case.height, case.channels)
    chunks = spec.chunks(f)                                               # signature, every CRC against zlib.crc32, nothing behind IEND
    kinds = [k for k, _ in chunks]
    n_idat = -(-len(want) // CHUNK) + 1
    assert kinds == [b"IHDR"] + [b"IDAT"] * n_idat + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", case.width, case.height, 8, spec.COLOR_TYPE[case.channels], 0, 0, 0)
    idat = b"".join(body for k, body in chunks if k == b"IDAT")
    assert idat[:2] == b"\x78\x01" and len(chunks[-2][1]) == 4
    assert zlib.decompress(idat) == want                                  # criterion 2: the filtered picture, byte for byte
    bgra = spec.to_bgra(case.samples)
    assert np.array_equal(png_spec.decode(f), bgra)
    assert np.array_equal(ops.png_picture(f), bgra)
    for form in ("CHW", "BGRA", "bottom-up"):                             # the file is a function of the samples, not of where they lie
        host, src = host_source(case, form)
        assert ops.png_encode_picture(src, case.filter) == f, form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pil_opens_the_files(case):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(key(case)[3]))
    im.load()
    assert im.mode == spec.MODE[case.channels] and im.size == (case.width, case.height)
    assert np.array_equal(np.asarray(im).reshape(case.samples.shape), case.samples)


def test_a_cap_one_byte_short():
    L = capi.lib()
    for case in CASES[3::7]:
        f = key(case)[3]
        host, src = host_source(case, "HWC")
        for cap in (len(f), len(f) - 1, 7, 0):
            out = np.full(len(f) + 64, 0xA5, np.uint8)
            n = C.c_size_t()
            rc = L.ffhip_png_encode_picture(C.byref(src), case.filter, out.ctypes.data, cap, C.byref(n))
            assert rc == (0 if cap == len(f) else capi.FFHIP_EPNG_NOSPACE) and n.value == len(f), (case.id, cap)
            assert out[:cap].tobytes() == f[:cap] and (out[cap:] == 0xA5).all(), (case.id, cap)


def test_arguments():
    L = capi.lib()
    px = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros(4096, np.uint8)
    n = C.c_size_t()

    def calls(src, filter=5, o=out.ctypes.data, cap=4096, ln=C.byref(n)):
        return (L.ffhip_png_encode_picture(src, filter, o, cap, ln), L.ffhip_png_filter_picture(src, filter, o, cap, ln))

    good = ops.png_host_source(px)
    assert calls(C.byref(good)) == (0, 0)
    assert calls(None) == (capi.FFHIP_EINVAL,) * 2
    assert calls(C.byref(good), ln=None) == (capi.FFHIP_EINVAL,) * 2
    assert calls(C.byref(good), o=None) == (capi.FFHIP_EINVAL,) * 2
    assert calls(C.byref(good), filter=6) == (capi.FFHIP_EINVAL,) * 2 and calls(C.byref(good), filter=-1) == (capi.FFHIP_EINVAL,) * 2
    for field, value in (("width", 0), ("width", 65536), ("height", 0), ("height", 65536), ("channels", 0), ("channels", 5), ("reserved", 1),
                         ("pixels", None), ("row_stride", 1 << 30), ("pixel_stride", -(1 << 30))):
        bad = ops.png_host_source(px)
        setattr(bad, field, value)
        assert calls(C.byref(bad)) == (capi.FFHIP_EINVAL,) * 2, field
    bad = ops.png_host_source(px)
    bad.chan[2] = 1 << 30
    assert calls(C.byref(bad)) == (capi.FFHIP_EINVAL,) * 2
    assert L.ffhip_png_filter_picture(C.byref(good), 5, out.ctypes.data, 4 * 13 - 1, C.byref(n)) == capi.FFHIP_EPNG_NOSPACE and n.value == 4 * 13
    assert ops.png_encode_bound(0, 1, 1) == 0 and ops.png_encode_bound(1, 1, 5) == 0 and ops.png_encode_bound(65536, 1, 1) == 0
    with pytest.raises(ValueError):
        ops.png_filter_id("best")
    with pytest.raises(ValueError):
        ops.png_host_source(np.zeros((4, 4, 5), np.uint8))


def test_the_bound_is_the_stored_form():
    for w, h, c in ((1, 1, 1), (100, 64, 3), (910, 9, 4), (65535, 3, 4)):
        flen = h * (1 + w * c)
        chunks = -(-flen // CHUNK)
        assert ops.png_encode_bound(w, h, c) == 33 + 12 * chunks + ops.deflate_bound(flen) + 12 + 12
    noise = np.random.default_rng(8).integers(0, 256, (64, 300, 4), dtype=np.uint8)     # full noise: never longer than the bound
    assert len(ops.png_encode_picture(noise)) <= ops.png_encode_bound(300, 64, 4)
    assert len(ops.png_encode_picture(noise, 0)) <= ops.png_encode_bound(300, 64, 4)


def test_a_flat_picture_is_small():
    flat = np.full((256, 256, 4), 200, np.uint8)
    f = ops.png_encode_picture(flat)
    assert len(f) <= 4096, len(f)                                         # 258-byte matches: an encoder without them cannot
    assert np.array_equal(ops.png_picture(f), spec.to_bgra(flat))


def test_both_host_encoders_under_the_sanitizers(tmp_path):
    """tests/tools/png_enc_asan_main.c: a few hundred streams and pictures in heap buffers of exactly their size, into outputs of exactly cap,
    under -fsanitize=address,undefined.  A stand-alone program with the sanitizers' runtimes linked into it: nothing is preloaded or loaded
    into Python"""
    gcc = shutil.which("gcc") or "gcc"
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "png_enc_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "tools", "png_enc_asan_main.c"),
                           os.path.join(csrc, "ffhip_deflate.c"), os.path.join(csrc, "ffhip_png_enc.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().startswith("ok: ") and r.stdout.strip().endswith("pictures")


def test_the_part_loop_on_the_cpu_under_the_sanitizers(tmp_path):
    """tests/tools/check_parts.cpp: ffhip_parts_run (ffhip_parts.h, the part loop of the four encoders' entry points) over
    seeded lists of weights: the cut, the cap on a part's items, and what a part's return code does to the call's.  A stand-alone program
    with the sanitizers' runtimes linked into it"""
    gxx = shutil.which("g++") or "g++"
    exe = str(tmp_path / "check_parts")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ffpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "check_parts.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok: 400 lists, "), r.stdout
