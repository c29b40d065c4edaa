"""CPU: the progressive JPEG front end -- parse, scan list and host decoder (ffhip_jpeg_progressive.c) over the body it shares with the
kernel (ffhip_jpeg_prog_body.h).

The oracle is the baseline twin: a progressive file and a baseline file of the same quantised coefficients must give the same MCU-order
planes (padding blocks included), and ffhip_jpeg_entropy_decode is pinned on the reference already.  Files a PIL pair cannot reach come
from the writer of tests/jpeg_progressive.py, whose coefficients are known."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import jpeg_progressive as P
import progressive_cases as PC
from ffpic_amd import capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = capi.FFHIP_EINVAL


def _probe_any(data):
    L = capi.lib()
    g, w, h, pg = capi.JpegGeom(), C.c_int(), C.c_int(), C.c_int()
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    return L.ffhip_jpeg_probe_any(buf.ctypes.data, len(data), C.byref(g), C.byref(w), C.byref(h), C.byref(pg)), g, pg.value


def _decode_rc(data, k_max=63):
    """(code of probe or decode, planes) -- planes of the probed geometry, exact size"""
    rc, g, _ = _probe_any(data)
    if rc:
        return rc, None
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cy = np.full(g.y_blocks * 64, 77, np.int16)
    cu = np.full(g.c_blocks * 64, 77, np.int16)
    cv = np.full(g.c_blocks * 64, 77, np.int16)
    q = np.zeros((4, 64), np.uint16)
    rc = capi.lib().ffhip_jpeg_progressive_decode(buf.ctypes.data, buf.size, C.byref(g), cy.ctypes.data, cu.ctypes.data, cv.ctypes.data,
                                                  q.ctypes.data, k_max)
    return rc, (cy, cu, cv, q)


def _same_as_twin(prog, twin, k_max=63):
    g, cy, cu, cv, q = ops.jpeg_progressive_decode(prog, k_max)
    g2, by, bu, bv, bq = ops.jpeg_entropy_batch([twin])
    assert (g.mcu_cols, g.mcu_rows, g.ncomp, g.h, g.v, tuple(g.qt_id)) == (g2.mcu_cols, g2.mcu_rows, g2.ncomp, g2.h, g2.v, tuple(g2.qt_id))
    return g, (cy, cu, cv, q), (by, bu, bv, bq[0])


# ---- A: the shared body under the sanitizers ----
def test_shared_body_under_sanitizers(tmp_path):
    """ASan + UBSan build of the host decoder -- the per-block steps and the interval walk the kernel runs too -- as a stand-alone program:
    every truncation of one small progressive file (restart markers, ten scans) and 4000 seeded mutations of it, file and planes malloc'd at
    their exact size.  Every run ends in FFHIP_OK or FFHIP_EINVAL."""
    rng = np.random.default_rng(5)
    coef = P.random_coef(rng, 24, 16, 2, 2, 3)
    path = str(tmp_path / "small.jpg")
    open(path, "wb").write(P.encode_progressive(24, 16, 2, 2, coef, PC.QUANT[:2], P.pil_script(3), restart=2))
    exe = str(tmp_path / "fuzz_progressive")
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "tools", "fuzz_progressive.c"),
                           os.path.join(csrc, "ffhip_jpeg_progressive.c"), os.path.join(csrc, "ffhip_entropy.c"), os.path.join(csrc, "ffhip_jpeg_front.c"),
                           "-lpthread", "-o", exe])
    out = subprocess.run([exe, "4000", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "decoded" in out.stdout and "unexpected" not in out.stdout


# ---- B: PIL twins ----
def test_pil_twins_give_the_baseline_planes():
    pytest.importorskip("PIL.Image")
    longest = 0
    for tag, prog, twin in PC.pil_pairs():
        rc, g, pg = _probe_any(prog)
        assert rc == 0 and pg == 1, tag
        assert _probe_any(twin)[2] == 0, tag
        g, got, exp = _same_as_twin(prog, twin)
        assert np.array_equal(got[3], exp[3]), tag                       # quant
        assert np.array_equal(got[0], exp[0]), tag                       # whole planes, padding blocks included
        if g.ncomp == 3:
            assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), tag
        model = P.model_decode(prog)
        assert np.array_equal(model["coef"][0].reshape(-1), exp[0]), tag  # the model agrees: the writer's round trips below stand on it
        longest = max([longest] + [s["max_eobrun"] for s in model["scans"]])
    assert longest > 1                                                   # the set is not vacuous: some scan carries an EOBRUN


# ---- C: writer files ----
@pytest.mark.parametrize("k", range(11))
def test_writer_files_give_the_written_coefficients(k):
    case = PC.writer_cases()[k]
    g, cy, cu, cv, q = ops.jpeg_progressive_decode(case["file"])
    assert (g.ncomp, g.h, g.v) == (case["ncomp"], case["h"], case["v"])
    got = [cy, cu, cv]
    for c in range(case["ncomp"]):
        assert np.array_equal(got[c].reshape(-1, 64), case["planes"][c]), (case["tag"], c)
    assert np.array_equal(q[0], PC.QUANT[0])
    # the baseline twin of those planes decodes to them as well: the GPU tests compare pixels through it
    _, by, bu, bv, _ = ops.jpeg_entropy_batch([case["twin"]])
    assert np.array_equal(by, cy) and (cu is None or (np.array_equal(bu, cu) and np.array_equal(bv, cv)))


def test_writer_cases_reach_what_they_are_for():
    cases = {c["tag"]: c for c in PC.writer_cases()}
    big = P.model_decode(cases["grey_2048x1024_empty_band"]["file"])
    assert big["scans"][1]["max_eobrun"] == 32767                        # 32 768 empty blocks: the 14-bit class, and the run split behind it
    cut = P.model_decode(cases["restart_cuts_eobrun"]["file"])
    assert max(s["max_eobrun"] for s in cut["scans"]) > 1
    assert all(len(P.scan_units(40, 24, 2, 2, s["comps"])) % 7 for s in cut["scans"])  # the DRI divides no scan's unit count
    inc = cases["incomplete"]
    model = P.model_decode(inc["file"])
    g, cy, cu, cv, _ = ops.jpeg_progressive_decode(inc["file"])
    for c, got in enumerate((cy, cu, cv)):
        assert np.array_equal(got.reshape(-1, 64), model["coef"][c]), c
    assert not cv.reshape(-1, 64)[:, 1:].any() and cu.reshape(-1, 64)[:, 1:].any()   # a band never sent stays zero
    late = cases["late_ones"]["planes"]
    assert max(int(np.abs(p[:, 1:]).max()) for p in late) == 1
    # the ZRL case: its refinement scans hold ZRL symbols in blocks whose run passes non-zero history
    zrl = cases["zrl_in_refinement"]
    seen = []
    P.encode_progressive(16, 16, 1, 1, [zrl["planes"][0]], PC.QUANT[:1], zrl["script"], token_hook=lambda i, toks: seen.append((i, toks)))
    assert any(t == ("s", 0, 0xF0) for i, toks in seen if zrl["script"][i][3] for iv in toks for t in iv)


# ---- D: refusals ----
def _small(script=None, **kw):
    rng = np.random.default_rng(11)
    coef = P.random_coef(rng, 16, 16, 2, 2, 3)
    return P.encode_progressive(16, 16, 2, 2, coef, PC.QUANT[:2], script or P.pil_script(3), **kw)


def _patch_scan(scan, **fields):
    """a hook that rewrites fields of scan `scan`'s header: ss, se, ahal, or the whole header"""
    def hook(i, hdr, data):
        if i != scan:
            return hdr, data
        hdr = bytearray(fields.get("header", hdr))
        for name, off in (("ss", -3), ("se", -2), ("ahal", -1)):
            if name in fields:
                hdr[off] = fields[name]
        return bytes(hdr), data
    return hook


@functools.lru_cache(maxsize=None)
def _parse_time_refusals():
    good = _small()
    k = good.find(b"\xff\xc2")
    dht = good.find(b"\xff\xc4")
    second_dht = good.find(b"\xff\xc4", good.find(b"\xff\xda"))
    dqt = good[good.find(b"\xff\xdb"):good.find(b"\xff\xdb") + 69]
    many = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), i, i, 0, 0) for c in (0, 1, 2) for i in range(1, 64)]
    return {
        "arithmetic": good[:k + 1] + b"\xca" + good[k + 2:],
        "lossless": good[:k + 1] + b"\xc3" + good[k + 2:],
        "12-bit": good[:k + 4] + b"\x0c" + good[k + 5:],
        "AC scan of two components": _small(raw_scan_hook=_patch_scan(1, header=bytes([2, 1, 0, 2, 0, 1, 5, 2]))),
        "Ss = 0 with Se != 0": _small(raw_scan_hook=_patch_scan(0, se=5)),
        "Se < Ss": _small(raw_scan_hook=_patch_scan(1, ss=6, se=5)),
        "Se > 63": _small(raw_scan_hook=_patch_scan(2, se=64)),
        "first scan with Ah != 0": _small([((0, 1, 2), 0, 0, 1, 0)]),
        "Ah is not the previous Al": _small([((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 1, 0)]),
        "Al is not Ah - 1": _small([((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 2, 0)]),
        "a band sent twice": _small([((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 3, 9, 0, 0)]),
        "AC before DC": _small([((0,), 1, 63, 0, 0), ((0, 1, 2), 0, 0, 0, 0)]),
        "DQT behind the first SOS": good[:second_dht] + dqt + good[second_dht:],
        "more than 128 scans": _small(many),
        "table not yet defined": good[:dht + 4] + b"\x03" + good[dht + 5:],
        "missing EOI": _small(eoi=False),
    }


def test_the_refusal_files_are_what_they_say():
    """the pristine file of the refusal cases decodes, and 128 scans are not too many"""
    assert _decode_rc(_small())[0] == 0
    ok = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), i, i, 0, 0) for c in (0, 1, 2) for i in range(1, 64)][:capi.FFHIP_JPEG_MAX_SCANS - 1]
    assert _decode_rc(_small(ok))[0] == 0


@pytest.mark.parametrize("what", list(_parse_time_refusals()))
def test_refused_at_parse_time(what):
    rc, _, _ = _probe_any(_parse_time_refusals()[what])
    assert rc == EINVAL, what


def test_malformed_scans_are_refused_by_the_decode():
    good = _small()
    # cut in the middle of the third scan
    third = [i for i in range(len(good) - 1) if good[i] == 0xFF and good[i + 1] == 0xDA][2]
    nxt = good.find(b"\xff\xc4", third)
    assert _decode_rc(good[:(third + 10 + nxt) // 2])[0] == EINVAL
    # the same with an EOI put behind the cut: the parse accepts it, the scan runs dry
    rc_probe, _, _ = _probe_any(good[:third + 12] + b"\xff\xd9")
    assert rc_probe == 0 and _decode_rc(good[:third + 12] + b"\xff\xd9")[0] == EINVAL
    # an EOBRUN past the interval: four grey blocks with an empty AC band are one EOBRUN of 4; the same bytes under a SOF of two blocks
    coef = [np.zeros((4, 64), np.int16)]
    coef[0][:, 0] = (5, -3, 8, 1)
    f = bytearray(P.encode_progressive(16, 16, 1, 1, coef, PC.QUANT[:1], PC.GREY_EMPTY))
    assert _decode_rc(f)[0] == 0
    k = f.find(b"\xff\xc2")
    f[k + 5:k + 7] = (8).to_bytes(2, "big")                                # height 16 -> 8
    assert _probe_any(f)[0] == 0 and _decode_rc(f)[0] == EINVAL
    # a refinement symbol with s = 2: the last scan's table names (r, 1) symbols; one of them becomes (r, 2)
    f = bytearray(PC.writer_cases()[3]["file"])                              # ("late_ones": its last pass brings new coefficients)
    assert _decode_rc(f)[0] == 0
    dht = f.rfind(b"\xff\xc4")
    n = sum(f[dht + 5:dht + 21])
    hits = [i for i in range(dht + 21, dht + 21 + n) if f[i] & 15 == 1]
    assert hits
    for i in hits:
        f[i] += 1
    assert _probe_any(f)[0] == 0 and _decode_rc(f)[0] == EINVAL
    # a geometry other than the expected one, and arguments
    g = capi.jpeg_geom(3, 1)
    buf = np.frombuffer(good, np.uint8)
    cy = np.zeros(4 * 256, np.int16)
    q = np.zeros((4, 64), np.uint16)
    L = capi.lib()
    assert L.ffhip_jpeg_progressive_decode(buf.ctypes.data, buf.size, C.byref(g), cy.ctypes.data, cy.ctypes.data, cy.ctypes.data, q.ctypes.data, 63) == EINVAL
    assert L.ffhip_jpeg_progressive_decode(buf.ctypes.data, buf.size, None, cy.ctypes.data, cy.ctypes.data, cy.ctypes.data, q.ctypes.data, 64) == EINVAL
    assert L.ffhip_jpeg_progressive_decode(buf.ctypes.data, buf.size, None, cy.ctypes.data, None, None, q.ctypes.data, 63) == EINVAL


def test_a_header_cannot_ask_for_more_intervals_than_its_scan_has_bytes_for():
    """DRI = 1 under a SOF of 65 535 x 65 535 asks for half a billion restart intervals a scan; a scan of n intervals holds at least
    2 (n - 1) marker bytes, so the parse refuses the file before anything is sized by that figure"""
    f = bytearray(_small(restart=1))
    assert _decode_rc(bytes(f))[0] == 0
    k = f.find(b"\xff\xc2")
    f[k + 5:k + 9] = b"\xff\xff\xff\xff"
    assert _probe_any(f)[0] == EINVAL


# ---- E: k_max ----
def _skipped_by_rule(script, k_max):
    """scans with Ss above k_max, where k_max first grows to the Se of every kept refinement that reaches beyond it"""
    k, grew = k_max, True
    while grew:
        grew = False
        for _, ss, se, ah, _ in script:
            if ah and ss <= k < se:
                k, grew = se, True
    return sum(1 for _, ss, _, _, _ in script if ss > k)


def test_k_max_skips_whole_scans_and_keeps_the_leading_coefficients():
    pytest.importorskip("PIL.Image")
    low = [P.ZZ[:k + 1] for k in range(64)]
    pairs = {tag: (prog, twin) for tag, prog, twin in PC.pil_pairs()}
    cases = [(pairs["420_40x24"][0], pairs["420_40x24"][1], P.pil_script(3)), (pairs["grey_37x19"][0], pairs["grey_37x19"][1], P.pil_script(1))]
    spectral = PC.writer_cases()[0]
    cases.append((spectral["file"], spectral["twin"], spectral["script"]))
    for prog, twin, script in cases:
        assert [(s["comps"], s["ss"], s["se"], s["ah"], s["al"]) for s in P.model_decode(prog)["scans"]] == [tuple(s) for s in script]
        for k_max in (0, 4, 24, 63):
            g, got, exp = _same_as_twin(prog, twin, k_max)
            last = ops.progressive_last()
            assert last[2] == _skipped_by_rule(script, k_max) and last[1] + last[2] == len(script) and last[0] == 1 and last[4] == 0
            for c in range(g.ncomp):
                a, b = got[c].reshape(-1, 64), exp[c].reshape(-1, 64)
                assert np.array_equal(a[:, low[k_max]], b[:, low[k_max]]), (k_max, c)
                if k_max == 0:
                    assert not a[:, P.ZZ[1:]].any()
    # the spectral-selection script has bands that do not straddle: k_max = 4 drops the three 6..63 scans, k_max = 0 every AC scan
    assert _skipped_by_rule(spectral["script"], 4) == 3 and _skipped_by_rule(spectral["script"], 0) == 6
    assert _skipped_by_rule(P.pil_script(3), 0) == 8


# ---- F: default arguments ----
def test_flags_zero_is_the_old_call():
    """ffhip_jpeg_decode_files_mixed_device_ex with flags = 0 refuses a progressive file as ffhip_jpeg_decode_files_mixed_device does; with
    FFHIP_JPEG_ACCEPT_PROGRESSIVE the probe accepts it.  Seen through what the calls check before they touch a device: the outputs are
    NULL, so every file ends with FFHIP_EINVAL, but a file the probe took has its geometry in geom_out."""
    pytest.importorskip("PIL.Image")
    _, prog, twin = PC.pil_pairs()[0]
    L = capi.lib()
    bufs = [np.frombuffer(f, np.uint8) for f in (twin, prog)]
    ptrs = (C.c_void_p * 2)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * 2)(*[b.size for b in bufs])
    outs = (C.c_void_p * 2)(None, None)
    pitch = (C.c_int64 * 2)(0, 0)

    def call(fn, *mid):
        geoms, status = (capi.JpegGeom * 2)(), (C.c_int * 2)(5, 5)
        rc = fn(ptrs, lens, 2, 2, outs, pitch, *mid, geoms, status, None)
        return rc, list(status), [(g.mcu_cols, g.mcu_rows, g.h, g.v) for g in geoms]

    old = call(L.ffhip_jpeg_decode_files_mixed_device)
    assert call(L.ffhip_jpeg_decode_files_mixed_device_ex, None, 0) == old
    assert old[1][1] == EINVAL and old[2][1] == (0, 0, 0, 0) and old[2][0] == (3, 2, 2, 2)
    rc, status, geoms = call(L.ffhip_jpeg_decode_files_mixed_device_ex, None, capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE)
    assert geoms == [(3, 2, 2, 2), (3, 2, 2, 2)]
    den = (C.c_int * 2)(1, 3)
    assert call(L.ffhip_jpeg_decode_files_mixed_device_ex, den, 0)[0] == EINVAL      # a bad denominator
    assert call(L.ffhip_jpeg_decode_files_mixed_device_ex, None, 2)[0] == EINVAL     # an unknown flag
    # the device front end checks its arguments before it looks for a device
    st = (C.c_int * 1)()
    one = (C.c_void_p * 1)(bufs[1].ctypes.data)
    ln = (C.c_size_t * 1)(bufs[1].size)
    zero = capi.jpeg_geom(0, 4)
    assert L.ffhip_jpeg_progressive_batch_gpu(one, ln, 1, 1, C.byref(zero), 8, 8, 8, 8, 63, st, None) == EINVAL
    g = capi.jpeg_geom(3, 2)
    assert L.ffhip_jpeg_progressive_batch_gpu(one, ln, 1, 1, C.byref(g), 8, 8, 8, 8, 64, st, None) == EINVAL
    assert L.ffhip_jpeg_progressive_batch_gpu(one, ln, 1, 1, C.byref(g), 8, None, 8, 8, 63, st, None) == EINVAL
