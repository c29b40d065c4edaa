"""CPU: the JPEG entropy decoders against the ANSWER.  tests/jpeg_cases.py writes baseline files from known coefficients, under Huffman tables and
with symbols no encoder of photographs produces; every witness -- the Python fixture decoder, the host C decoder, the reference's whole-file decode --
must return exactly what was written.  These run before a GPU is involved: a mismatch in tests/test_jpeg_known_coefs_gpu.py can then only be a kernel's.
Also here: that the cases still reach the branches they are for (so that an edit cannot quietly make one trivial), that the writer's default output
is what the h4v1 / h1v4 golden files were made with, and the host staging pass on scans that are mostly FF 00 pairs."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_entropy
import jpeg_writer
import oracle_lib as O
from ffpic_amd import capi, ops, synth

ALL = list(JC.CASES)
RESTART = [n for n in ALL if JC.CASES[n][5]]


def _same_planes(case, cy, cu, cv, at=0):
    """the planes a decoder returned for picture `at` of a batch are the written ones"""
    for got, want in zip((cy, cu, cv), case.coef):
        if want is None:
            continue
        assert np.array_equal(got[at * want.size:(at + 1) * want.size], want), case.facts["name"]


def _lut(data, tc, th):
    L = capi.lib()
    L.ffhip_jpeg_lut_test.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ffhip_jpeg_lut_test.restype = C.c_int
    buf = np.frombuffer(data, np.uint8)
    lut = np.zeros(1536, np.uint16)
    assert L.ffhip_jpeg_lut_test(buf.ctypes.data, buf.size, tc * 4 + th, lut.ctypes.data) == 0
    return lut


# ---------------------------------------------------------------------------------------------------- 1. the writer
def test_writer_unchanged_by_default():
    """encode() without the new keyword arguments: the bytes of the writer before it had them (the SHA-256 was taken with that writer, not this one)"""
    rng = np.random.default_rng(20261018)
    q = synth.quant_tables()
    h = hashlib.sha256()
    for (w, hh, H, V, ncomp, restart) in ((45, 30, 2, 2, 3, 2), (17, 9, 1, 1, 1, 0), (70, 20, 4, 1, 3, 1), (24, 40, 1, 4, 3, 0), (33, 17, 2, 1, 3, 3)):
        mc, mr = -(-w // (8 * H)), -(-hh // (8 * V))
        coef = [synth._blocks(rng, mc * mr * H * V, q[0])]
        coef += [synth._blocks(rng, mc * mr, q[1]), synth._blocks(rng, mc * mr, q[1])] if ncomp == 3 else [None, None]
        h.update(jpeg_writer.encode(w, hh, H, V, coef, q, restart=restart))
    assert h.hexdigest() == "711f12cb28ee09eb5801bebb7ac45ecc4e708a5dd2dd26ae756802a6ccb8ced7"


@pytest.mark.parametrize("builder", ["deep_tables", "long_tables", "short_dc_tables", "ones_tables"])
def test_table_builders_give_valid_codes(builder):
    """Kraft sum below 1 (so no code is all ones), every symbol once, all twelve DC sizes and all 162 AC symbols of a baseline scan"""
    for (tc, th), (counts, syms) in getattr(jpeg_writer, builder)().items():
        assert len(counts) == 16 and sum(counts) == len(syms) == len(set(syms))
        assert jpeg_writer.kraft(counts) < 65536
        assert set(syms) == (set(jpeg_writer.AC_L[1]) if tc else set(range(12)))


# ---------------------------------------------------------------------------------------------------- 2. the cases reach what they are for
def test_deep_tables_overflow_the_lookup_groups_and_the_scan_uses_the_overflow():
    """deep tables: level one of the device look-up table (ffhip_jpeg_lut_test) has exactly 8 group entries (0x8000 | g), and the prefixes of the codes
    beyond them are 0 -- "take the canonical-code walk" --, not 0x5000 -- "no such code": build_lut knows the table is incomplete.  The large picture's
    scan holds a thousand symbols and more with such codes, EOB and ZRL among them."""
    case = JC.case("440_mixed_deep")
    f = case.facts
    total = 0
    for c in range(3):
        th = f["table_ids"][c][1]
        counts, syms = f["dht"][(1, th)]
        walk = JC.walk_symbols(counts, syms)
        assert len(set(walk.values())) >= 12 - JC.LUT_GROUPS and {0x00, 0xF0, 0x01, 0x11} <= set(walk)
        lut = _lut(case.data, 1, th)
        groups = [int(e) for e in lut[:512] if e & 0x8000]
        assert sorted(groups) == [0x8000 | g for g in range(8)]
        used = {sym: n for (tc, t, sym), n in f["stats"]["symbols"].items() if tc == 1 and t == th and sym in walk}
        assert used.get(0x00, 0) and used.get(0xF0, 0)
        for sym in used:
            assert lut[walk[sym]] == 0, hex(sym)
        if c < 2:       # (the two chroma components share their table: counted once)
            total += sum(used.values())
    assert total >= 1000
    long_prefixes = set()
    counts, syms = f["dht"][(1, 0)]
    for sym, (code, length) in jpeg_writer._codes(counts, syms).items():
        if length > 9:
            long_prefixes.add(code >> (length - 9))
    assert len(long_prefixes) >= 12
    # the DC tables of the family, and every other family's tables: complete, no zero left anywhere in the levels in use
    assert not (_lut(case.data, 0, 0)[:512] == 0).any()
    assert not (_lut(JC.case("444_3x2_dense_long_r5").data, 1, 0)[:512] == 0).any()


def test_dense_has_no_eob_and_blocks_longer_than_half_a_subsequence():
    st = JC.case("420_dense").facts["stats"]
    assert not any(sym == 0x00 for (tc, th, sym) in st["symbols"] if tc == 1)
    assert np.mean(st["block_bits"]) > 1024
    assert sum(st["block_bits"]) >= 40 * JC.SUB_BITS
    assert st["symbols"].get((0, 0, 11), 0) == 6 * 4 * 4     # DC size 11: every luma block (-1024 behind 0, then +-2047)
    assert st["symbols"].get((1, 0, 0x0A), 0) > 1000            # AC size 10 under Annex K's 16-bit code: half the coefficients and more


def test_sparse_has_a_subsequence_of_tiny_blocks_and_three_zrls_in_a_row():
    case = JC.case("444_sparse")
    st = case.facts["stats"]
    bits = np.array(st["block_bits"])
    best = run = 0
    for b in bits:
        run = run + int(b) if b < 8 else 0
        best = max(best, run)
    assert best >= JC.SUB_BITS
    assert 2 <= bits.min() <= 4
    assert st["zrl_in_a_row"] == 3
    assert bits.sum() >= 40 * JC.SUB_BITS
    used = {sym for (tc, th, sym) in st["symbols"] if tc == 1}
    assert {0xF1, 0xF2, 0xE1, 0xE2} & used and 0xF0 in used              # runs of 15 and (behind three ZRLs) 14
    y = case.coef[0].reshape(-1, 64)
    for k in JC.SPARSE_K:                                                 # every position, 63 among them: a block that ends by a run, not by an EOB
        assert (y[:, jpeg_entropy.ZZ[k]] != 0).any(), k


def test_ones_scans_are_dense_in_stuffed_bytes():
    for name in ("h4v1_ones", "h4v1_3x2_ones_r1", "422_1_ones"):
        data = JC.case(name).data
        sos = data.find(b"\xff\xda")
        scan = data[sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"):-2]
        assert scan.count(b"\xff\x00") * 16 >= len(scan), name


def test_some_file_has_dc_differences_of_plus_and_minus_2047():
    assert JC.case("420_dense").facts["stats"]["dc_diffs"] == (-2047, 2047)


def test_every_large_picture_has_forty_subsequences_and_restart_markers_wrap():
    for name in JC.LARGE:
        assert sum(JC.case(name).facts["stats"]["block_bits"]) >= 40 * JC.SUB_BITS, name
    assert {JC.CASES[n][0] for n in JC.LARGE} == set(JC.LAYOUTS)
    assert JC.case("h1v4_mixed_long_r1").data.count(b"\xff\xd0") >= 4 and b"\xff\xd7" in JC.case("grey_dense_deep_r5").data
    ids = {i for n in ALL for pair in JC.case(n).facts["table_ids"] for i in pair}
    assert ids == {0, 1, 2, 3}
    assert {JC.CASES[n][5] for n in ALL} >= {0, 1, 5} and any(JC.CASES[n][5] == JC.CASES[n][1] for n in RESTART)      # none, 1 MCU, 5 MCUs, an MCU row
    assert any(JC.CASES[n][6] for n in ALL)                                # a width that is no multiple of the MCU


# ---------------------------------------------------------------------------------------------------- 3. the witnesses
@pytest.mark.parametrize("name", ALL)
def test_python_decoder_returns_the_written_coefficients(name):
    case = JC.case(name)
    f = case.facts
    dec = jpeg_entropy.decode(case.data)
    assert (dec["mcu_cols"], dec["mcu_rows"], dec["ncomp"], dec["h"], dec["v"]) == (f["mcu_cols"], f["mcu_rows"], f["ncomp"], f["h"], f["v"])
    assert (dec["width"], dec["height"]) == (f["width"], f["height"])
    _same_planes(case, *dec["coef"])
    for t in set(dec["qt_id"][:f["ncomp"]]):
        assert np.array_equal(dec["quant"][t], case.quant[t])


@pytest.mark.parametrize("name", ALL)
def test_host_decoder_returns_the_written_coefficients(name):
    """ffhip_jpeg_entropy_batch: three pictures of the case's geometry with different content, on 1 and on 5 threads"""
    cases = [JC.case(name, seed) for seed in range(3)]
    for threads in (1, 5):
        g, cy, cu, cv, quant = ops.jpeg_entropy_batch([c.data for c in cases], n_threads=threads)
        for i, c in enumerate(cases):
            _same_planes(c, cy, cu, cv, at=i)
            for t in set(tuple(g.qt_id)[:g.ncomp]):
                assert np.array_equal(quant[i][t], c.quant[t])


@pytest.mark.parametrize("name", RESTART)
def test_host_decoder_over_threads_by_restart_interval(name):
    """ffhip_jpeg_entropy_decode_mt: one picture's restart intervals shared out over 1, 3 and 64 threads"""
    case = JC.case(name)
    L = capi.lib()
    g, _, _ = ops.jpeg_probe(case.data)
    buf = np.frombuffer(case.data, np.uint8)
    for th in (1, 3, 64):
        cy = np.full(g.y_blocks * 64, 77, np.int16)
        cu = np.full(max(g.c_blocks, 1) * 64, 77, np.int16)
        cv = np.full(max(g.c_blocks, 1) * 64, 77, np.int16)
        q = np.zeros((4, 64), np.uint16)
        assert L.ffhip_jpeg_entropy_decode_mt(buf.ctypes.data, buf.size, C.byref(g), cy.ctypes.data, cu.ctypes.data, cv.ctypes.data, q.ctypes.data, th) == 0
        _same_planes(case, cy, cu, cv)


@pytest.mark.parametrize("name", ["444_1_sparse_deep", "grey_1_mixed_deep", "420_3x2_mixed_deep23_r1", "444_3x2_dense_long_r5", "440_3x2_sparse_shared",
                                  "h4v1_3x2_ones_r1", "grey_3x2_dense_ids23_r5", "grey_dense_deep_r5"])
def test_device_lookup_table_decodes_the_case_scans(name, monkeypatch):
    """build_lut on the CPU: the fixture decoder with its symbol step replaced by a model of the kernels' -- level one of the library's two-level table
    (ffhip_jpeg_lut_test) by nine bits, a group by the next seven, the canonical code only where the entry is 0 -- returns the written coefficients, never
    meets "no such code", and takes the canonical code for the deep tables' symbols only"""
    case = JC.case(name)
    dht = case.facts["dht"]
    walked = []

    def build(counts, symbols):
        (tc, th), = [k for k, (c, s) in dht.items() if list(c) == list(counts) and list(s) == list(symbols)][:1]
        return _lut(case.data, tc, th), {(length, code): sym for sym, (code, length) in jpeg_writer._codes(counts, symbols).items()}

    def symbol(br, table):
        lut, canonical = table
        e, used = int(lut[br.bits(9)]), 9
        if e & 0x8000:
            e, used = int(lut[512 + ((e & 0xff) << 7) + br.bits(7)]), 16
        if e == 0:
            br.n += used
            code = 0
            for length in range(1, 17):
                code = (code << 1) | br.bit()
                if (length, code) in canonical:
                    assert length > 9
                    walked.append(canonical[(length, code)])
                    return canonical[(length, code)]
            raise AssertionError("no code")
        assert not e & 0x4000
        br.n += used - ((e >> 8) & 31)
        return e & 0xff
    monkeypatch.setattr(jpeg_entropy, "_build_huff", build)
    monkeypatch.setattr(jpeg_entropy, "_decode_sym", symbol)
    dec = jpeg_entropy.decode(case.data)
    _same_planes(case, *dec["coef"])
    assert bool(walked) == ("deep" in case.facts["tables"])


# The reference's whole-file loader on the case files.  Its loader stores every byte of a scan but the last (read_compressed_scan, format/jpg.c:604-633,
# writes the byte BEFORE the one it has just read; a stuffed FF 00 at the very end is the one ending it stores whole), and its bit reader then takes the
# end of the last data unit from memory nobody wrote: the last MCU comes out with pixels that change from process to process, or the reader runs past
# its buffer and exits (utils/bitstream.c:117) -- as it does, in the last MCU only, for two of the fixture files.  The case files (seed 0) therefore END
# in FF 00 (jpeg_cases._write: a last coefficient of 1023 at k = 63), the reference's decode of them is a function of the file, and the comparison
# leaves out nothing: no MCU, no case.  (It accepts table ids 2 and 3 in a baseline frame, and every table family.)
@pytest.mark.parametrize("name", ALL)
def test_reference_decodes_the_case_files_to_the_oracle_pixels_of_the_written_coefficients(name, tmp_path):
    """the reference's file decode == the oracle's reconstruction of the WRITTEN planes (O.check_ref: where the reference is built, element for element;
    elsewhere by the recorded digest).  The reference returns the picture's height and its width rounded up to 8."""
    case = JC.case(name)
    f = case.facts
    assert case.data[-4:] == b"\xff\x00\xff\xd9"
    g = O.make_geom(f["mcu_cols"], f["mcu_rows"], f["ncomp"], f["h"], f["v"])
    mine = O.oracle_jpeg_recon(g, case.coef[0], case.coef[1], case.coef[2], case.quant)[0][:f["height"], :(f["width"] + 7) // 8 * 8]

    def reference():
        sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
        import make_golden
        path = str(tmp_path / (name + ".jpg"))
        open(path, "wb").write(case.data)
        return make_golden.ref_decode_file(O.ref(), path)
    O.check_ref("known_coefs/" + name, np.ascontiguousarray(mine), reference)


# ---------------------------------------------------------------------------------------------------- 4. staging
@pytest.mark.parametrize("name", ["h4v1_ones", "h4v1_3x2_ones_r1", "422_1_ones"])
def test_stage_scan_on_scans_dense_in_stuffed_bytes(name):
    """ffhip_jpeg_stage_scan_raw_test: the unstuffed bytes of every interval, its own length, and the offsets -- every interval 4-byte aligned behind at
    least four zero bytes -- against a plain unstuffing of the same scan"""
    case = JC.case(name)
    data = case.data
    sos = data.find(b"\xff\xda")
    scan = data[sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"):]
    want, cur, i = [], bytearray(), 0
    while True:                                                           # FF 00 -> FF; RSTn ends an interval; EOI ends the scan
        if scan[i] != 0xFF:
            cur.append(scan[i]); i += 1
        elif scan[i + 1] == 0:
            cur.append(0xFF); i += 2
        else:
            want.append(bytes(cur)); cur = bytearray()
            if scan[i + 1] == 0xD9:
                break
            i += 2
    mcus = case.facts["mcu_cols"] * case.facts["mcu_rows"]
    n_seg = -(-mcus // case.facts["restart"]) if case.facts["restart"] else 1
    assert len(want) == n_seg
    L = capi.lib()
    L.ffhip_jpeg_stage_scan_raw_test.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.POINTER(C.c_size_t), C.c_void_p]
    L.ffhip_jpeg_stage_scan_raw_test.restype = C.c_int
    src = np.frombuffer(scan, np.uint8)
    dst = np.full(len(scan) + 8 * n_seg + 128, 0xA5, np.uint8)
    seg, raw, clean = np.zeros(n_seg + 1, np.uint32), np.zeros(n_seg + 1, np.uint32), C.c_size_t()
    assert L.ffhip_jpeg_stage_scan_raw_test(dst.ctypes.data, src.ctypes.data, src.size, seg.ctypes.data, n_seg, C.byref(clean), raw.ctypes.data) == n_seg
    off = 0
    for k, w in enumerate(want):
        assert seg[k] == off and raw[k] == len(w), k
        assert bytes(dst[off:off + len(w)]) == w, k
        nxt = off + ((len(w) + 3) & ~3) + 4
        assert not dst[off + len(w):nxt].any()
        off = nxt
    assert clean.value == off
