"""CPU: the host entries of the lossy WebP encoder (include/ffpic_hip.h "Lossy WebP encoding") against the numpy witness
tests/vp8_encode_spec.py, array for array, and their files against PIL (libwebp) and the spec decoder tests/vp8_spec.py; the bound, the cap,
argument errors, source forms; size and fidelity on the golden photographs against PIL's method 0; the host side under the sanitizers as a
program of its own."""
import ctypes as C
import glob
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import vp8_encode_spec as E
import vp8_spec as S
from ffpic_amd import capi, ops
from vp8_encode_cases import CASES, picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = [c.id for c in CASES]
# the worst deficit against libwebp's method 0 at equal size over the golden photographs and qualities 30, 50, 75, 90, measured with the host
# entry (4.71 dB, the 1080p WebP picture at quality 75; DESIGN.md 4.36 has the table), rounded up to the next 0.1 dB
FIDELITY_DB = 4.8
FILES = {}


def host_file(case):
    if case.id not in FILES:
        FILES[case.id] = ops.vp8_encode_picture(case.pixels, case.quality, case.filter)
    return FILES[case.id]


def test_the_header_states_the_constants():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    assert "#define FFHIP_EVP8_NOSPACE (-1401)" in text and "#define FFHIP_EVP8_PARTITION (-1402)" in text
    assert capi.FFHIP_EVP8_NOSPACE == -1401 and capi.FFHIP_EVP8_PARTITION == -1402
    assert "(5 y_ac_qi) >> 4" in text and "not libwebp's gamma-aware averaging" in text
    assert [ops.vp8_encode_quality_index(q) for q in range(101)] == list(E.QUALITY_QI)
    for q in (-1, 101):
        assert capi.lib().ffhip_vp8_encode_quality_index(q) == capi.FFHIP_EINVAL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_and_macroblocks_equal_the_witness(case):
    for got, want in zip(ops.vp8_encode_planes(case.pixels), E.planes(case.pixels)):
        assert np.array_equal(got, want)
    got, want = ops.vp8_encode_mbs(case.pixels, case.quality), E.encode_mbs(case.pixels, case.quality)
    for k in ("ymode", "uvmode", "levels", "y", "u", "v"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_file_against_pil_the_spec_decoder_and_the_witness(case):
    data = host_file(case)
    h, w = case.pixels.shape[:2]
    assert 0 < len(data) <= ops.vp8_encode_bound(w, h) and len(data) % 2 == 0
    d = S.decode(data, rules=S.SPEC)
    im = Image.open(io.BytesIO(data))
    assert im.size == (w, h) and not d["refused"] and np.array_equal(np.asarray(im.convert("RGB")), d["rgb"])
    hd = E.header(case.pixels, case.quality, case.filter)                     # a spec parse shows the witness's header
    assert d["nbr_partitions"] == 1 << hd["log2_parts"] and [int(v) for v in d["quant"][0]] == E.steps(hd["y_ac_qi"])
    assert d["filter_type"] == (2 if hd["level"] else 0)
    if hd["level"]:
        assert tuple(int(v) for v in d["filters"][0, 0]) == tuple(int(v) for v in S._filters(S._Rules(S.SPEC), 0, 0, [0] * 4, hd["level"], 0, 0, 0, 0, 1)[0, 0])
    m = ops.vp8_encode_mbs(case.pixels, case.quality)
    assert np.array_equal(d["levels"], m["levels"]) and np.array_equal(d["modes"][:, 0], m["ymode"]) and np.array_equal(d["modes"][:, 1], m["uvmode"])
    assert np.array_equal(d["skip"], (~m["levels"].reshape(len(m["ymode"]), -1).any(axis=1)))
    if case.filter == 0:
        for k in "yuv":
            assert np.array_equal(d[k], m[k]), k
    assert data == E.file(case.pixels, case.quality, case.filter)             # prob_skip_false, flush and padding agree: byte for byte


def test_nospace_writes_nothing_at_or_beyond_cap():
    for case in CASES[::3]:
        want = host_file(case)
        src = ops.jpeg_host_source(case.pixels)
        for cap in (len(want) - 1, len(want), 0, 29, 31):
            out = np.full(len(want) + 64, 0xA5, np.uint8)
            n = C.c_size_t()
            rc = capi.lib().ffhip_vp8_encode_picture(C.byref(src), case.quality, case.filter, out.ctypes.data if cap else None, cap, C.byref(n))
            assert rc == (0 if cap >= len(want) else capi.FFHIP_EVP8_NOSPACE) and n.value == len(want), (case.id, cap)
            assert out[:min(cap, len(want))].tobytes() == want[:cap] and (out[min(cap, len(want)):] == 0xA5).all(), (case.id, cap)


def test_the_bound_holds_and_grows():
    assert ops.vp8_encode_bound(0, 4) == 0 and ops.vp8_encode_bound(4, 16384) == 0 and ops.vp8_encode_bound(16383, 16383) > 0
    assert ops.vp8_encode_bound(1, 1) == 30 + (7 * (1094 + 7) + 7) // 8 + 4 + (7 * 7321 + 7) // 8 + 4 + 1
    assert ops.vp8_encode_bound(16, 130) > ops.vp8_encode_bound(16, 128) > ops.vp8_encode_bound(16, 16)
    noise = np.random.default_rng(1).integers(0, 2, (64, 64, 3), dtype=np.uint8) * 255
    assert len(ops.vp8_encode_picture(noise, 100, 0)) <= ops.vp8_encode_bound(64, 64)


def test_argument_errors():
    L = capi.lib()
    px = picture(8, 8, 1)
    out, n = np.zeros(4096, np.uint8), C.c_size_t()

    def call(src, quality=75, filter=0, o=out.ctypes.data, cap=4096, length=n):
        return L.ffhip_vp8_encode_picture(C.byref(src) if src is not None else None, quality, filter, o, cap, C.byref(length) if length is not None else None)

    good = ops.jpeg_host_source(px)
    assert call(good) == 0
    E_ = capi.FFHIP_EINVAL
    assert call(None) == E_ and call(good, quality=101) == E_ and call(good, quality=-1) == E_ and call(good, filter=64) == E_ and call(good, filter=-2) == E_
    assert call(good, o=None) == E_ and call(good, length=None) == E_
    for change in (dict(width=0), dict(height=0), dict(width=16384), dict(height=16384), dict(channels=4), dict(channels=2), dict(reserved=1), dict(pixels=None)):
        bad = ops.jpeg_host_source(px)
        for k, v in change.items():
            setattr(bad, k, v)
        assert call(bad) == E_, change
        y = np.zeros(1 << 16, np.uint8)
        assert L.ffhip_vp8_encode_planes(C.byref(bad), y.ctypes.data, y.ctypes.data, y.ctypes.data) == E_
    assert L.ffhip_vp8_encode_planes(C.byref(good), None, out.ctypes.data, out.ctypes.data) == E_
    item = capi.Vp8EncodeItem()
    item.src, item.quality, item.filter, item.d_out, item.cap = good, 75, 0, 16, 100
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    assert L.ffhip_vp8_encode_items(None, 1, lens, status, None) == E_ and L.ffhip_vp8_encode_items(C.byref(item), -1, lens, status, None) == E_
    assert L.ffhip_vp8_encode_items(C.byref(item), 1, None, status, None) == E_ and L.ffhip_vp8_encode_items(C.byref(item), 1, lens, None, None) == E_
    item.quality = 101
    assert L.ffhip_vp8_encode_items(C.byref(item), 1, lens, status, None) == E_
    item.quality, item.src.channels = 75, 4
    assert L.ffhip_vp8_encode_items(C.byref(item), 1, lens, status, None) == E_
    item.src.channels, item.d_out = 3, None
    assert L.ffhip_vp8_encode_items(C.byref(item), 1, lens, status, None) == E_
    if L.ffhip_device_count() == 0:
        item.d_out = 16
        assert L.ffhip_vp8_encode_items(C.byref(item), 1, lens, status, None) == capi.FFHIP_ENODEV


def test_strided_bgr_and_planar_sources():
    px = picture(33, 19, 12)
    want = ops.vp8_encode_picture(px, 60, 5)
    wide = np.zeros((19, 50, 3), np.uint8)
    wide[:, 7:40] = px
    assert ops.vp8_encode_picture(wide[:, 7:40], 60, 5) == want                # a padded pitch and an offset
    bgr = np.ascontiguousarray(px[..., ::-1])
    assert ops.vp8_encode_picture(bgr[..., ::-1], 60, 5) == want               # BGR in memory: a negative channel stride
    chw = np.ascontiguousarray(px.transpose(2, 0, 1))
    assert ops.vp8_encode_picture(chw.transpose(1, 2, 0), 60, 5) == want       # planar
    flipped = np.ascontiguousarray(px[::-1, ::-1])
    assert ops.vp8_encode_picture(flipped[::-1, ::-1], 60, 5) == want          # negative row and pixel strides
    grey = px[..., 1]
    assert ops.vp8_encode_picture(grey, 60, 5) == ops.vp8_encode_picture(np.repeat(grey[..., None], 3, 2), 60, 5)   # grey is R = G = B


def photographs():
    """the decoded golden photographs, a 640 x 480 crop of the larger ones"""
    names = sorted(glob.glob(os.path.join(GOLDEN, "file_q*.jpg"))) + [os.path.join(GOLDEN, "file_1080p_q75.webp")]
    return [(os.path.basename(n), np.ascontiguousarray(np.asarray(Image.open(n).convert("RGB"))[:480, :640])) for n in names]


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def fidelity_table(pictures):
    """-> [(name, quality, size, psnr, size of PIL's method 0 at equal quality, libwebp's quality, size and psnr at the largest quality whose
    size is ours at most)]"""
    rows = []
    for name, px in pictures:
        made = {}

        def pil_file(q):
            if q not in made:
                b = io.BytesIO()
                Image.fromarray(px).save(b, "WEBP", quality=q, method=0)
                made[q] = b.getvalue()
            return made[q]
        for quality in (30, 50, 75, 90):
            data = ops.vp8_encode_picture(px, quality, -1)
            lo, hi = 0, 100                                                    # the sizes rise with the quality
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if len(pil_file(mid)) <= len(data) else (lo, mid - 1)
            rows.append((name, quality, len(data), psnr(pil_rgb(data), px), len(pil_file(quality)), lo, len(pil_file(lo)), psnr(pil_rgb(pil_file(lo)), px)))
    return rows


def test_size_and_fidelity_against_libwebp_method_0():
    rows = fidelity_table(photographs())
    for k in range(0, len(rows), 4):
        sizes, psnrs = [r[2] for r in rows[k:k + 4]], [r[3] for r in rows[k:k + 4]]
        assert sizes == sorted(sizes) and len(set(sizes)) == 4 and psnrs == sorted(psnrs), rows[k][0]
    for name, quality, size, p, same_q, lib_q, lib_size, lib_p in rows:
        print(f"{name} q{quality}: {size} B {p:.2f} dB; PIL method 0 at q{quality} {same_q} B; at q{lib_q} {lib_size} B {lib_p:.2f} dB; deficit {lib_p - p:.2f}")
    for name, quality, size, p, same_q, lib_q, lib_size, lib_p in rows:
        assert p >= lib_p - FIDELITY_DB, (name, quality, p, lib_p)


def test_host_encoder_clean_under_sanitizers(tmp_path):
    """tests/tools/check_vp8_enc.cpp with ffhip_vp8_enc.c under -fsanitize=address,undefined: the small cases in heap buffers of exactly
    their size, every cap from 0 to the file's length into outputs of exactly cap bytes.  A stand-alone program with the sanitizers' runtimes
    linked into it: nothing is loaded into Python"""
    gcc = shutil.which("gcc") or "gcc"
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "check_vp8_enc")
    subprocess.check_call([gcc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "tools", "check_vp8_enc.cpp"),
                           os.path.join(csrc, "ffhip_vp8_enc.c"), os.path.join(csrc, "ffhip_jpeg_enc.c"), "-o", exe, "-lstdc++"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
