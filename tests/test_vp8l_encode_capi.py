"""CPU: the host lossless WebP encoder (ffhip_vp8l_encode_residual, ffhip_vp8l_encode_picture).  The residual words and the
tiles' modes against the numpy witness (tests/vp8l_encode_spec.py) in every source form; the files' pixels through PIL, the VP8L witness of
the decoder (tests/vp8l_spec.py) and the library's own host decoder; the probe, the bound, the cap, the argument checks, the size conditions,
and the host encoder in a stand-alone program under the sanitizers.  The witness restates TRANSFORMS only: PARSE and CODES are held by the
three decoders and, on the device, by equality with these files."""
import ctypes as C
import heapq
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vp8l_encode_spec as spec
import vp8l_spec
from ffpic_amd import capi, ops
from png_encode_cases import FORMS, source_form
from vp8l_encode_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = [c.id for c in CASES]
FILES = {}
# the real pictures of tests/golden that DESIGN.md 4.33's table uses
CORPUS = ["file_1080p_q75.webp", "file_q85_420.jpg", "file_q80_grey.jpg", "file_q85_114.jpg", "file_q85_411.jpg", "file_q85_420_dri.jpg",
          "file_q88_422.jpg", "file_q92_444.jpg"]


def host_file(case):
    if case.id not in FILES:
        FILES[case.id] = ops.vp8l_encode_picture(case.samples, case.flags)
    return FILES[case.id]


def host_source(case, form):
    host, off, row, pixel, chan = source_form(case.samples, form)
    return host, capi.png_source(host.ctypes.data + off, case.width, case.height, row, pixel, chan)


def test_the_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    for name, value in (("FFHIP_VP8L_ENC_SUBTRACT_GREEN", "0x1"), ("FFHIP_VP8L_ENC_PREDICT", "0x2"), ("FFHIP_VP8L_ENC_TILE_BITS", spec.TILE_BITS),
                        ("FFHIP_VP8L_ENC_CHUNK", spec.CHUNK), ("FFHIP_EVP8L_NOSPACE", "(-1301)")):
        assert f"#define {name} {value}" in text, name
    assert (capi.FFHIP_VP8L_ENC_SUBTRACT_GREEN, capi.FFHIP_VP8L_ENC_PREDICT) == (spec.SUBTRACT_GREEN, spec.PREDICT) == (1, 2)
    assert capi.FFHIP_VP8L_ENC_TILE_BITS == spec.TILE_BITS and capi.FFHIP_VP8L_ENC_CHUNK == spec.CHUNK and capi.FFHIP_EVP8L_NOSPACE == -1301
    assert C.sizeof(capi.Vp8lEncodeItem) == C.sizeof(capi.PngSource) + 24


def test_the_witness_sees_ties_and_many_modes():
    """a flat picture ties all of modes 1..13 at zero (mode 1, not 0, wins: black is far away); the scenes use several modes"""
    by_id = {c.id: c for c in CASES}
    _, modes, sums = spec.residual(by_id["70x70x4-flat"].samples, 3)
    assert (modes == 1).all() and (sums[..., 1:] == 0).all() and (sums[..., 0] > 0).all()
    _, modes, _ = spec.residual(by_id["300x300x3-scene"].samples, 3)
    assert len(set(modes.reshape(-1).tolist())) >= 5


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_residual_equals_the_witness_in_every_form(case):
    want, modes, _ = spec.residual(case.samples, case.flags)
    if case.samples.size <= 70 * 70 * 4:
        spec.check_against_writer(case.samples, case.flags, want, modes)   # the witness against the decoders' answer key
    for form in FORMS:
        host, src = host_source(case, form)
        res, got_modes = ops.vp8l_encode_residual(src, case.flags)
        assert np.array_equal(res, want), (form, np.argwhere(res != want)[:4].tolist())
        assert (got_modes is None and modes is None) or np.array_equal(got_modes, modes), form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_files_decode_to_the_samples(case):
    f = host_file(case)
    assert len(f) <= ops.vp8l_encode_bound(case.width, case.height) and len(f) % 2 == 0
    size, chunk = struct.unpack("<I", f[4:8])[0], struct.unpack("<I", f[16:20])[0]
    assert f[:4] == b"RIFF" and f[8:16] == b"WEBPVP8L" and size == len(f) - 8 and chunk + (chunk & 1) == len(f) - 20 and f[20] == 0x2F
    assert ops.vp8l_probe(f) == (case.width, case.height, int(case.channels in (2, 4)))
    info = ops.vp8l_info(f)
    assert info.cache_bits == 0 and not info.has_meta
    bgra = spec.to_bgra(case.samples)
    assert np.array_equal(vp8l_spec.decode(f), bgra)
    assert np.array_equal(ops.vp8l_picture(f), bgra)
    for form in ("CHW", "BGRA", "bottom-up", "reversed"):                 # the file is a function of the samples, not of where they lie
        host, src = host_source(case, form)
        assert ops.vp8l_encode_picture(src, case.flags) == f, form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pil_opens_the_files(case):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(host_file(case)))
    im.load()
    assert im.size == (case.width, case.height) and im.mode == ("RGBA" if case.channels in (2, 4) else "RGB")
    assert np.array_equal(np.asarray(im.convert("RGBA")), spec.rgba_of(case.samples))      # transparent pixels' colours too


def test_a_cap_one_byte_short():
    L = capi.lib()
    for case in CASES[2::5]:
        f = host_file(case)
        host, src = host_source(case, "HWC")
        for cap in (len(f), len(f) - 1, 21, 0):
            out = np.full(len(f) + 64, 0xA5, np.uint8)
            n = C.c_size_t()
            rc = L.ffhip_vp8l_encode_picture(C.byref(src), case.flags, out.ctypes.data, cap, C.byref(n))
            assert rc == (0 if cap == len(f) else capi.FFHIP_EVP8L_NOSPACE) and n.value == len(f), (case.id, cap)
            assert out[:cap].tobytes() == f[:cap] and (out[cap:] == 0xA5).all(), (case.id, cap)


def test_arguments():
    L = capi.lib()
    px = np.zeros((4, 4, 3), np.uint8)
    out, res, modes = np.zeros(8192, np.uint8), np.zeros(16, np.uint32), np.zeros(4, np.uint8)
    n = C.c_size_t()
    E = capi.FFHIP_EINVAL

    def calls(src, flags=3, o=out.ctypes.data, cap=8192, ln=C.byref(n)):
        return (L.ffhip_vp8l_encode_picture(src, flags, o, cap, ln), L.ffhip_vp8l_encode_residual(src, flags, res.ctypes.data, modes.ctypes.data))

    good = ops.png_host_source(px)
    assert calls(C.byref(good)) == (0, 0)
    assert calls(None) == (E, E)
    assert calls(C.byref(good), ln=None)[0] == E and calls(C.byref(good), o=None)[0] == E
    assert calls(C.byref(good), flags=4) == (E, E) and calls(C.byref(good), flags=-1) == (E, E)
    assert L.ffhip_vp8l_encode_residual(C.byref(good), 3, None, modes.ctypes.data) == E
    assert L.ffhip_vp8l_encode_residual(C.byref(good), 3, res.ctypes.data, None) == E
    assert L.ffhip_vp8l_encode_residual(C.byref(good), 1, res.ctypes.data, None) == 0
    for field, value in (("width", 0), ("width", 16385), ("height", 0), ("height", 16385), ("channels", 0), ("channels", 5), ("reserved", 1),
                         ("pixels", None), ("row_stride", 1 << 30), ("pixel_stride", -(1 << 30))):
        bad = ops.png_host_source(px)
        setattr(bad, field, value)
        assert calls(C.byref(bad)) == (E, E), field
    assert ops.vp8l_encode_bound(0, 1) == 0 and ops.vp8l_encode_bound(1, 16385) == 0 and ops.vp8l_encode_bound(1, 1) > 0
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    it = capi.Vp8lEncodeItem()
    it.src, it.flags, it.d_out, it.cap = capi.png_source(16, 4, 4, 12, 3, (0, 1, 2)), 3, 16, 100
    for field, value in (("reserved", 1), ("flags", 4), ("d_out", None)):    # refused before any device is looked for
        bad = capi.Vp8lEncodeItem()
        bad.src, bad.flags, bad.d_out, bad.cap = it.src, it.flags, it.d_out, it.cap
        setattr(bad, field, value)
        assert L.ffhip_vp8l_encode_items(C.byref(bad), 1, lens, status, None) == E, field
    if L.ffhip_device_count() == 0:
        assert L.ffhip_vp8l_encode_items(C.byref(it), 1, lens, status, None) == capi.FFHIP_ENODEV


def test_the_bound():
    """4096 bytes, 2 a tile, 60 bits a pixel, 2 bytes; below 2^32 at the largest picture; full noise stays within it"""
    tile = 1 << spec.TILE_BITS
    for w, h in ((1, 1), (100, 64), (4097, 3), (16384, 16384)):
        tiles = -(-w // tile) * -(-h // tile)
        assert ops.vp8l_encode_bound(w, h) == 4096 + 2 * tiles + (w * h * 60 + 7) // 8 + 2
    assert ops.vp8l_encode_bound(16384, 16384) < 1 << 32
    noise = np.random.default_rng(8).integers(0, 256, (64, 300, 4), dtype=np.uint8)
    for flags in (0, 3):
        assert len(ops.vp8l_encode_picture(noise, flags)) <= ops.vp8l_encode_bound(300, 64)


def huffman_depth(counts):
    """the depth of an unrestricted Huffman tree over the counts"""
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def test_the_length_limit_binds_on_the_fibonacci_picture():
    case = next(c for c in CASES if c.id == "110x161x3-fibonacci-plain")
    px = case.samples.reshape(-1, 3)
    for d in (1, 110):                                                    # no three pixels in a row repeat at either distance: all literals
        same = (px[d:] == px[:-d]).all(1)
        assert not (same[2:] & same[1:-1] & same[:-2]).any(), d
    counts = np.bincount(px[:, 1], minlength=256)
    assert huffman_depth(counts) == 19
    lengths = ops.deflate_code_lengths(counts, 15)
    assert max(lengths) <= 15 and sum(2.0 ** -int(l) for l in lengths if l) == 1.0             # the limit binds: the halving rule ran; the code is complete
    assert np.array_equal(vp8l_spec.decode(host_file(case)), spec.to_bgra(case.samples))


def test_a_flat_picture_is_small():
    """sixteen chunks of one literal and one run each, every alphabet simple: PNG's file of the same picture has 1 483 bytes"""
    flat = np.full((256, 256, 4), 200, np.uint8)
    f = ops.vp8l_encode_picture(flat)
    assert len(f) <= 1024, len(f)
    assert np.array_equal(ops.vp8l_picture(f), spec.to_bgra(flat))


def corpus_pictures():
    Image = pytest.importorskip("PIL.Image")
    for name in CORPUS:
        im = Image.open(os.path.join(GOLDEN, name))
        im.load()
        a = np.asarray(im)
        yield name, np.ascontiguousarray(a if a.ndim == 3 else a[..., None])


def test_the_corpus_is_smaller_than_its_png_files():
    """the condition is on the total; the figures go to DESIGN.md 4.34"""
    webp = png = 0
    for name, px in corpus_pictures():
        f = ops.vp8l_encode_picture(px)
        p = ops.png_encode_picture(px)
        print(f"{name}: {px.shape[1]} x {px.shape[0]} x {px.shape[2]}: webp {len(f)}, png {len(p)}")
        if px.size < 200000:
            assert np.array_equal(ops.vp8l_picture(f), spec.to_bgra(px)), name
        webp += len(f)
        png += len(p)
    print(f"total: webp {webp}, png {png}, ratio {webp / png:.3f}")
    assert webp <= png


def test_the_host_encoder_under_the_sanitizers(tmp_path):
    """tests/tools/vp8l_enc_asan_main.c: pictures in heap buffers of exactly their size, into outputs of exactly cap, under
    -fsanitize=address,undefined.  A stand-alone program with the sanitizers' runtimes linked into it: nothing is preloaded or loaded into
    Python"""
    gcc = shutil.which("gcc") or "gcc"
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = str(tmp_path / "vp8l_enc_asan")
    subprocess.check_call([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "tools", "vp8l_enc_asan_main.c"),
                           os.path.join(csrc, "ffhip_vp8l_enc.c"), os.path.join(csrc, "ffhip_png_enc.c"), os.path.join(csrc, "ffhip_deflate.c"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().startswith("ok: ") and r.stdout.strip().endswith("pictures")
