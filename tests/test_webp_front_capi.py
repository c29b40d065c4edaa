"""The host front end for lossy WebP (ffhip_webp_probe / ffhip_webp_parse / ffhip_webp_parse_batch, ffhip_vp8_dequant_factors)
against what the reference's own WEBP_load did with every fixture of tests/golden/make_golden_webp.py.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from ffpic_amd import capi, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRONT = np.load(os.path.join(GOLDEN, "webp_front.npz"))
NAMES = [str(n) for n in FRONT["names"]]
# Files the reference cannot record (8 token partitions overflow its p[4] / bt[4]; a height that is not a multiple of 16 its BGRA
# buffer): no reference data, so host parser, kernels and oracle chain are held against each other on them.
UNPINNED = ["syn_parts8", "syn_h37", "pil_50x37_q30"]


def file_bytes(name):
    return open(os.path.join(GOLDEN, name + ".webp"), "rb").read()


def test_webp_manifest_intact():
    """the fixtures of make_golden_webp.py against their own manifest"""
    import hashlib
    lines = open(os.path.join(GOLDEN, "MANIFEST_webp.sha256")).read().split("\n")
    listed = {}
    for line in lines:
        if line.strip():
            digest, name = line.split()
            listed[name] = digest
            assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == digest, name
    want = set(n + ".webp" for n in NAMES + UNPINNED if n.startswith(("syn_", "pil_"))) | {"webp_front.npz", "file_1080p_q75.webp"}
    assert want == set(listed)
    # and no golden WebP file outside both manifests
    other = {line.split()[1] for line in open(os.path.join(GOLDEN, "MANIFEST.sha256")) if line.strip()}
    assert {f for f in os.listdir(GOLDEN) if f.endswith(".webp")} <= want | other


def oracle_residual(p):
    """levels -> the coefficients the predictor sees, by the oracle's residual stage with the DERIVED quantisers, through resmap"""
    n = len(p["modes"])
    res = np.zeros((n, 384), np.int16)
    for i in range(n):
        q = np.ascontiguousarray(p["quant"][p["mbinfo"][i, 26], :6])
        O.ffo().ffo_vp8_residual_mb(np.ascontiguousarray(p["levels"][i]).reshape(-1), np.ascontiguousarray(p["mbinfo"][i, :25]),
                                    int(p["mbinfo"][i, 25]), q, res[i])
    return res[p["resmap"]]


def oracle_bgra(p, residual):
    c, r = p["mbcols"], p["mbrows"]
    y, u, v = O.oracle_vp8_frame(c, r, p["modes"], residual)
    y, u, v = [np.ascontiguousarray(a).copy() for a in (y, u, v)]
    if p["filter_type"]:
        O.ffo().ffo_vp8_loopfilter_frame(c, r, p["filter_type"], np.ascontiguousarray(p["modes"]).reshape(-1), np.ascontiguousarray(p["filters"]).reshape(-1),
                                         y.reshape(-1), u.reshape(-1), v.reshape(-1))
    out = np.zeros((16 * r, 64 * c), np.uint8)
    O.ffo().ffo_yuv420_to_bgra32(out.reshape(-1), 64 * c, y.reshape(-1), u.reshape(-1), v.reshape(-1), 16 * c, 8 * c, r, c)
    return out


def check_modes(got, want):
    """y mode, uv mode and segment id of every record; the sixteen 4x4 modes of the B_PRED ones (a 16x16 record holds its y mode
    and then whatever malloc gave the reference, webp.c:1430, 1824)"""
    assert np.array_equal(got[:, [0, 1, 18]], want[:, [0, 1, 18]])
    b = want[:, 0] == 4
    assert np.array_equal(got[b, 2:18], want[b, 2:18])
    assert np.array_equal(got[~b, 2], want[~b, 0])


@pytest.mark.parametrize("name", NAMES)
def test_parse_equals_reference(name):
    data = file_bytes(name)
    w, h, pitch = [int(x) for x in FRONT[f"{name}_dims"]]
    assert ops.webp_probe(data)[:2] == (w, h)
    p = ops.webp_parse(data)
    assert (p["width"], p["height"]) == (w, h) and len(FRONT[f"{name}_modes"]) == p["mbcols"] * p["mbrows"]
    check_modes(p["modes"], FRONT[f"{name}_modes"])
    lf = FRONT[f"{name}_lf"]
    assert p["filter_type"] == (0 if lf[0] == 0 else 1 if lf[1] else 2)
    assert np.array_equal(p["filters"].reshape(-1), lf[3:27])
    assert p["nbr_partitions"] == FRONT[f"{name}_lf_header"][9]
    res = oracle_residual(p)
    assert np.array_equal(res, FRONT[f"{name}_residual"])
    bgra = oracle_bgra(p, res)
    ref = FRONT[f"{name}_bgra"]   # [height][the reference's pitch]
    rows, width_bytes = min(h, 16 * p["mbrows"]), min(4 * w, 64 * p["mbcols"])
    assert np.array_equal(bgra[:rows, :width_bytes], ref[:rows, :width_bytes])


def test_unpinned_files_parse_by_the_rule_of_the_others():
    """8 token partitions and a height of 37: what the host front end makes of them, checked where no reference is needed"""
    p8 = ops.webp_parse(file_bytes("syn_parts8"))
    assert p8["nbr_partitions"] == 8 and (p8["mbcols"], p8["mbrows"]) == (3, 10)
    # row y takes its tokens from partition y & 7: garbling partition k leaves the rows above row k alone and changes row k (the rows
    # below follow through the `top` contexts); cutting the last partition short must fail
    data = bytearray(file_bytes("syn_parts8"))
    tag = data[20] | data[21] << 8 | data[22] << 16
    sizes_at = 30 + (tag >> 5)
    sizes = [data[sizes_at + 3 * k] | data[sizes_at + 3 * k + 1] << 8 | data[sizes_at + 3 * k + 2] << 16 for k in range(7)]
    start = sizes_at + 21
    for k in (1, 5, 7):
        g = bytearray(data)
        off = start + sum(sizes[:k])
        for j in range(off + 1, off + 400):
            g[j] ^= 0x5a
        q = ops.webp_parse(bytes(g))
        rows = np.where((q["levels"] != p8["levels"]).reshape(10, -1).any(axis=1))[0]
        assert rows.min() == k, (k, rows)
        assert np.array_equal(q["modes"], p8["modes"])
    assert _status(bytes(data[:start + sum(sizes) + 20]))[1] == capi.FFHIP_EINVAL      # 20 bytes of the eighth partition
    for n in ("syn_h37", "pil_50x37_q30"):
        d = file_bytes(n)
        assert ops.webp_probe(d) == (52, 40, 4, 3)        # rounded up to 4; three macroblock rows
        p = ops.webp_parse(d)
        assert oracle_bgra(p, oracle_residual(p)).shape == (48, 256)


def test_cases_reach_what_they_are_for():
    p = {n: ops.webp_parse(file_bytes(n)) for n in ("syn_parts2", "syn_parts4", "syn_simple_filter", "syn_skips", "syn_cat6", "syn_seg_abs")}
    assert p["syn_parts2"]["nbr_partitions"] == 2 and p["syn_parts4"]["nbr_partitions"] == 4
    assert p["syn_simple_filter"]["filter_type"] == 1
    skipped = p["syn_skips"]["resmap"] != np.arange(len(p["syn_skips"]["resmap"]))
    assert skipped.sum() > 5 and (~skipped).sum() > 1
    assert skipped[4] and skipped[5]                           # across a row end (5 macroblocks a row)
    # a skipped macroblock in front of every coded one (unpinned in the reference): its own all-zero row
    import vp8_writer
    first = ops.webp_parse(vp8_writer.keyframe(width=48, height=32, seed=107, y_ac_qi=35, prob_skip=1))
    assert first["resmap"][0] == 0 and first["mbinfo"][0, :25].sum() == 0 and not first["levels"][0].any()
    assert np.abs(p["syn_cat6"]["levels"].astype(np.int32)).max() > 67 + 200   # cat6 with large extra bits (they wrap at 256)
    assert (p["syn_seg_abs"]["quant"][2, :2] == (157, 284)).all()   # index 127 ...
    assert (p["syn_seg_abs"]["quant"][1, :2] == (157, 284)).all()   # ... and -5 wraps to it


def test_dequant_factors_table():
    tin, tout = FRONT["dequant_in"], FRONT["dequant_out"]
    assert len(tin) >= 9
    for row, want in zip(tin, tout):
        got = ops.vp8_dequant_factors(int(row[0]), row[1:6], int(row[6]), int(row[7]), row[8:12])
        assert np.array_equal(got[:, :6], want[:, :6]), row
        assert not got[:, 6:].any()
    # without segmentation only segment 0 is derived
    q = ops.vp8_dequant_factors(50)
    assert q[0, 0] > 0 and not q[1:].any()
    assert capi.lib().ffhip_vp8_dequant_factors(None, q.ctypes.data) == capi.FFHIP_EINVAL


def test_parse_batch_threads():
    files = [file_bytes(n) for n in NAMES] + [b"RIFF\x00\x00\x00\x00WEBPjunk"]
    for nt in (1, 3, 16):
        outs, status = ops.webp_parse_batch(files, n_threads=nt)
        assert status[-1] == capi.FFHIP_EINVAL and not any(status[:-1]) and outs[-1] is None
        for n, o in zip(NAMES, outs):
            one = ops.webp_parse(file_bytes(n))
            for k in ("modes", "levels", "mbinfo", "resmap", "quant", "filters"):
                assert np.array_equal(o[k], one[k]), (n, k)


def _status(data):
    """probe and parse codes of one candidate file; the arrays are sized for the probe's answer, or for nothing"""
    L = capi.lib()
    buf = np.frombuffer(bytes(data) + b"", dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    v = [C.c_int() for _ in range(4)]
    rc = L.ffhip_webp_probe(buf.ctypes.data, len(data), *[C.byref(x) for x in v])
    n_mb = v[2].value * v[3].value if rc == 0 else 1
    if n_mb > 1 << 16:
        return rc, None
    p, keep = ops._webp_parsed(max(n_mb, 1))
    return rc, L.ffhip_webp_parse(buf.ctypes.data, len(data), C.byref(p))


@pytest.mark.parametrize("name", ["syn_parts2", "syn_parts8"])
def test_hostile_input_gets_a_code(name):
    base = file_bytes(name)
    good = ops.webp_parse(base)
    n_bad = 0
    for cut in range(len(base)):                       # every truncation length
        rc, prc = _status(base[:cut])
        assert prc is None or prc in (0, capi.FFHIP_EINVAL)
        n_bad += prc != 0
    assert n_bad > 100                                 # the frame header alone is longer than that
    rng = np.random.default_rng(5)
    for k in range(400):                               # bytes flipped in header and partitions
        b = bytearray(base)
        for pos in rng.integers(12, len(b), 3):
            b[pos] ^= 1 << int(rng.integers(0, 8))
        rc, prc = _status(bytes(b))
        assert prc is None or prc in (0, capi.FFHIP_EINVAL, capi.FFHIP_EWEBP_INTER_FRAME, capi.FFHIP_EWEBP_LOSSLESS, capi.FFHIP_EWEBP_ANIMATION)
    # partition sizes pointing outside the file: the 3-byte size of partition 0 stands behind the first partition
    tag = base[20] | base[21] << 8 | base[22] << 16
    sizes_at = 30 + (tag >> 5)
    b = bytearray(base)
    b[sizes_at:sizes_at + 3] = b"\xff\xff\xff"
    assert _status(bytes(b))[1] == capi.FFHIP_EINVAL
    b = bytearray(base)
    b[20:23] = bytes([(0x7ffff << 5 | 0x10) & 255, (0x7ffff << 5) >> 8 & 255, (0x7ffff << 5) >> 16 & 255])   # a first partition of 512 KiB
    assert _status(bytes(b))[1] == capi.FFHIP_EINVAL
    for w, h in ((0, 16), (16, 0), (16383, 16383), (16383, 1)):   # zero and 16 383-pixel dimensions
        b = bytearray(base)
        b[26:30] = bytes([w & 255, w >> 8, h & 255, h >> 8])
        rc, prc = _status(bytes(b))
        assert (rc == capi.FFHIP_EINVAL) == (w == 0 or h == 0)
        assert prc is None or prc == capi.FFHIP_EINVAL
    assert _status(b"")[0] == capi.FFHIP_EINVAL and _status(b"RIFF")[0] == capi.FFHIP_EINVAL
    # what the front end names instead of decoding
    inter = bytearray(base); inter[20] |= 1
    assert _status(bytes(inter)) == (capi.FFHIP_EWEBP_INTER_FRAME, capi.FFHIP_EWEBP_INTER_FRAME)
    assert _status(b"RIFF\x10\x00\x00\x00WEBPVP8L\x04\x00\x00\x00\x2f\x00\x00\x00")[0] == capi.FFHIP_EWEBP_LOSSLESS
    anim = base[:12] + b"VP8X\x0a\x00\x00\x00\x02\x00\x00\x00" + bytes(6) + base[12:]
    assert _status(anim)[0] == capi.FFHIP_EWEBP_ANIMATION
    assert _status(base[:12] + b"ANIM\x06\x00\x00\x00" + bytes(6) + base[12:])[0] == capi.FFHIP_EWEBP_ANIMATION
    assert np.array_equal(ops.webp_parse(base)["levels"], good["levels"])


def test_unknown_chunk_is_skipped_by_its_size_without_padding():
    base = file_bytes("syn_odd_size")
    odd = base[:12] + b"ICCP\x03\x00\x00\x00abc" + base[12:]     # an odd-sized chunk, NO padding byte: that is how the reference walks
    assert np.array_equal(ops.webp_parse(odd)["modes"], ops.webp_parse(base)["modes"])
    padded = base[:12] + b"ICCP\x03\x00\x00\x00abc\x00" + base[12:]
    assert _status(padded)[0] == capi.FFHIP_EINVAL
    # VP8X / ALPH only at the reference's struct sizes
    assert _status(base[:12] + b"VP8X\x0b\x00\x00\x00" + bytes(11) + base[12:])[0] == capi.FFHIP_EINVAL
    assert _status(base[:12] + b"ALPH\x02\x00\x00\x00ab" + base[12:])[0] == capi.FFHIP_EINVAL
    assert ops.webp_probe(base[:12] + b"ALPH\x01\x00\x00\x00a" + base[12:]) == ops.webp_probe(base)


def test_argument_checks_without_a_device():
    L = capi.lib()
    data = np.frombuffer(file_bytes("syn_odd_size"), dtype=np.uint8)
    ptrs, lens = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(data.size)
    outs, pitch, status = (C.c_void_p * 1)(0x1000), (C.c_int64 * 1)(192), (C.c_int * 1)()
    assert L.ffhip_webp_decode_files_device(None, lens, 1, 1, outs, pitch, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, None, 1, 1, outs, pitch, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, lens, 1, 1, None, pitch, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, lens, 1, 1, outs, None, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, lens, 1, 1, outs, pitch, None, None, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, lens, -1, 1, outs, pitch, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_decode_files_device(ptrs, lens, 0, 1, outs, pitch, None, status, None) == 0
    assert L.ffhip_webp_parse_device(ptrs, lens, 1, None, status, None) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_parse(data.ctypes.data, data.size, None) == capi.FFHIP_EINVAL
    p, keep = ops._webp_parsed(2)                       # too small for the file's 6 macroblocks
    assert L.ffhip_webp_parse(data.ctypes.data, data.size, C.byref(p)) == capi.FFHIP_EINVAL
    assert L.ffhip_webp_parse_batch(None, lens, 1, 1, None, status) == capi.FFHIP_EINVAL
    if L.ffhip_device_count() == 0:                     # good arguments, no device: ENODEV, and the per-file verdicts of the header pass
        assert L.ffhip_webp_decode_files_device(ptrs, lens, 1, 1, outs, pitch, None, status, None) == capi.FFHIP_ENODEV


SAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ffpic_hip.h"
int ffhip_vp8_filter_params(const ffhip_vp8_filter_header *h, uint8_t *filters, int *filter_type) { (void)h; memset(filters, 0, 24); *filter_type = 0; return 0; }
static int one(const uint8_t *f, size_t len)
{
    uint8_t *copy = malloc(len ? len : 1); /* exactly len bytes: one byte further is the sanitizer's */
    memcpy(copy, f, len);
    int w, h, c, r, rc = ffhip_webp_probe(copy, len, &w, &h, &c, &r);
    if (rc == 0 && (long)c * r <= 65536) {
        size_t n = (size_t)c * r;
        ffhip_webp_parsed p = {malloc(n * 20), malloc(n * 800), malloc(n * 32), malloc(n * 4), (int64_t)n, {0}};
        rc = ffhip_webp_parse(copy, len, &p);
        free(p.modes); free(p.levels); free(p.mbinfo); free(p.resmap);
    }
    free(copy);
    return rc;
}
int main(int argc, char **argv)
{
    FILE *fp = fopen(argv[1], "rb");
    static uint8_t buf[1 << 20];
    size_t len = fread(buf, 1, sizeof buf, fp);
    unsigned s = 12345; long bad = 0;
    for (size_t cut = 0; cut <= len; cut++) bad += one(buf, cut) != 0;
    for (int k = 0; k < 3000; k++) {
        static uint8_t m[1 << 20];
        memcpy(m, buf, len);
        for (int j = 0; j < 4; j++) { s = s * 1664525u + 1013904223u; m[(s >> 8) % len] ^= (uint8_t)(1u << (s >> 29)); }
        bad += one(m, len) != 0;
    }
    printf("ok %ld\n", bad);
    return argc > 2;
}
"""


@pytest.mark.parametrize("name", ["syn_odd_size", "syn_parts8", "pil_50x37_q30"])
def test_hostile_input_under_sanitizers(tmp_path, name):
    """the host C alone (CPU build), -fsanitize=address,undefined: every truncation of a small file and a few thousand bit flips"""
    src = tmp_path / "san_main.c"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "san"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = ["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I" + os.path.join(root, "include"),
           "-I" + capi.CSRC, str(src), os.path.join(capi.CSRC, "ffhip_webp.c"), "-lpthread", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0")
    out = subprocess.run([str(exe), os.path.join(GOLDEN, name + ".webp")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stderr[-2000:]
