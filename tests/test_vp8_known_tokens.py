"""The VP8 front end against an answer key: key frames WRITTEN from known modes, segment ids, skip flags and levels (tests/vp8_cases.py,
tests/vp8_writer.keyframe_from), which every witness must return exactly -- the Python model of the parser, ffhip_webp_parse, the batch
call -- and which the reference's loader must turn into the pixels the oracle chain makes of the written arrays.  No GPU needed; the
two kernels read the same files in test_vp8_known_tokens_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import vp8_cases as VC
import vp8_writer as W
from ffpic_amd import capi, ops
from test_webp_front_capi import GOLDEN, check_modes, oracle_bgra, oracle_residual

sys.path.insert(0, GOLDEN)

ALL = list(VC.CASES)


def same_arrays(got, case, who):
    """modes by the rule of the fixtures' check (a 16x16 record: its y mode, then anything); the rest exactly"""
    check_modes(got["modes"], case.modes)
    assert np.array_equal(got["levels"], case.levels), f"{who}: levels"
    assert np.array_equal(got["mbinfo"][:, :27], case.mbinfo), f"{who}: token counts / has_y2 / segment"
    assert np.array_equal(got["resmap"], case.resmap), f"{who}: residual map"


def header_status(data):
    """ffhip_webp_read_header alone (the host pass in front of both front ends)"""
    buf = np.frombuffer(data, dtype=np.uint8)
    frame = np.zeros(8192, np.uint8)          # ffhip_webp_frame is some 1.3 KiB
    fn = capi.lib().ffhip_webp_read_header
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_void_p], C.c_int
    return fn(buf.ctypes.data, buf.size, frame.ctypes.data)


# ---------------------------------------------------------------------------------------------------- 1. the writer itself
def test_keyframe_still_writes_the_committed_fixtures():
    """keyframe() shares its header and container code with keyframe_from(): every syn_* fixture, written again, is the committed file"""
    import make_golden_webp as G
    cases = dict(G.synthetic_cases(), **G.unpinned_synthetic())
    assert len(cases) == 21
    for name, kw in cases.items():
        assert W.keyframe(**kw) == open(os.path.join(GOLDEN, name + ".webp"), "rb").read(), name


def test_reachable_slots_from_the_grammar():
    slots = VC.reachable_slots()
    assert len(slots) == VC.N_REACHABLE_SLOTS == 996
    assert not any(t == 0 and band == 0 for t, band, ctx, node in slots)                      # behind a Y2 block a Y block starts at position 1
    assert {(t, band) for t, band, ctx, node in slots if ctx == 0 and node == 0} == {(0, 1), (1, 0), (2, 0), (3, 0)}   # only at a first position


# ---------------------------------------------------------------------------------------------------- 2. what each case is for
def test_all_slots_visits_every_reachable_slot_with_both_bits():
    for seed in (0, 1, 2):
        f = VC.case("all_slots", seed).facts
        assert f["slots"] == {s + (b,) for s in VC.reachable_slots() for b in (0, 1)}
        assert len(f["slots"]) == 2 * 996
        probs = np.array(f["probs"])
        assert probs.min() >= 1 and len(set(f["probs"])) > 240                                # picking the wrong slot changes the probability


def test_token_ladder_puts_every_magnitude_at_every_position():
    c = VC.case("token_ladder")
    f = c.facts
    for t in range(4):
        for pos in VC.LADDER_POSITIONS:
            if t == 0 and pos == 0:
                continue
            for v in VC.LADDER:
                assert (t, pos, v) in f["positions"] and (t, pos, -v) in f["positions"], (t, pos, v)
    # cat6 wraps modulo 256: both values on record
    wrote, want = np.abs(f["written"]), np.abs(c.levels.astype(np.int64))
    assert (wrote == 67 + 256).any() and (want[wrote == 67 + 256] == 67).all()
    assert (wrote == 67 + 2047).any() and (want[wrote == 67 + 2047] == 67 + 255).all()
    assert (want[wrote == 67 + 255] == 67 + 255).all()
    assert c.mbinfo[47, 24] == 16 and c.mbinfo[46, 0] == 16 and (c.levels[46, 0] != 0).all()   # 16 non-zero tokens: no end of block read
    assert (c.mbinfo[48, :25] == 16).all() and not c.levels[48].any()                           # explicit zeros: count 16, nothing non-zero
    assert (c.mbinfo[45, :16] == 16).all() and not c.levels[45].any()
    for cat in ("cat3", "cat4", "cat5", "cat6"):
        assert f["tokens"][cat + "_extra_zeros"] > 0 and f["tokens"][cat + "_extra_ones"] > 0, cat
    assert all(f["tokens"][k] > 0 for k in ("EOB", "0", "1", "2", "3", "4", "cat1", "cat2"))


def test_extreme_probs_take_the_improbable_branch():
    f = VC.case("extreme_probs").facts
    probs = f["probs"]
    taken = {(probs[t * 264 + band * 33 + ctx * 11 + node], bit) for t, band, ctx, node, bit in f["slots"]}
    assert {(0, 0), (0, 1), (1, 0), (1, 1), (255, 0), (255, 1)} <= taken


def test_every_bmode_context_has_the_thousand_triples():
    for seed in (0, 1, 2):
        f = VC.case("every_bmode_context", seed).facts
        assert len(f["bmode_triples"]) == 1000
        assert f["bmode_kinds"] == {(side, kind) for side in ("above", "left") for kind in ("edge", "bpred", "i16_0", "i16_1", "i16_2", "i16_3")}


def test_y2_context_pattern():
    c = VC.case("y2_context")
    f, cols = c.facts, c.facts["mbcols"]
    for step in (1, cols):                                   # along row 0, down column 0
        for k, kind in enumerate(VC.Y2_PATTERN):
            mb = k * step
            assert f["skip"][mb] == kind.startswith("skipped") and (f["ymode"][mb] == 4) == kind.endswith("bpred")
            if kind == "A":
                assert c.mbinfo[mb, 24] > 0 and not c.mbinfo[mb, :16].any()      # Y2 flag set, every luma flag clear
            if kind == "C":
                between = VC.Y2_PATTERN[k - 1]
                assert f["y2_ctx"][mb] == (0 if between == "skipped_i16" else 1), (mb, between)
    used = {(ctx, node) for t, band, ctx, node, bit in f["slots"] if t == 1 and band == 0}
    assert {0, 1, 2} == {ctx for ctx, node in used}
    p = np.array(f["probs"][264:264 + 33]).reshape(3, 11)
    assert (np.abs(p[0, :3] - p[1, :3]) > 100).all()          # a wrong context derails the stream


def test_skip_cases():
    s = VC.case("skips")
    sk = s.facts["skip"]
    assert sk[0] and s.resmap[0] == 0 and not s.levels[0].any()          # nothing coded yet: its own, all-zero row
    assert sk[10:15].all() and sk[4] and sk[5] and (s.resmap[10:15] == 9).all()
    assert VC.case("skips_all").facts["skip"].all() and np.array_equal(VC.case("skips_all").resmap, np.arange(20))
    assert VC.case("skips_all").facts["part_bytes"][1] <= 12             # nothing but padding
    assert not VC.case("skips_coded_first").facts["skip"][0]


def test_segment_cases():
    for name in ("segments", "segments_off"):
        c = VC.case(name)
        assert set(c.modes[:, 18]) == {0, 1, 2, 3}
    assert VC.case("segments").facts["header"]["segmentation"]["probs"] == (120, 100, 160)
    assert VC.case("segments_off").facts["header"]["segmentation"] is None
    q = ops.webp_parse(VC.case("segments_off").data)["quant"]
    assert q[0].any() and not q[1:].any()                                # segmentation off: quantisers for segment 0 only


def test_geometry_and_partition_cases():
    want = {"geo_1x1": (1, 1, 1), "geo_1x9_p8": (1, 9, 8), "geo_9x1_p8": (9, 1, 8), "geo_3x10_p2": (3, 10, 2), "geo_3x10_p4": (3, 10, 4),
            "geo_3x10_p8": (3, 10, 8), "geo_50x37": (4, 3, 1)}
    for name, (cols, rows, nparts) in want.items():
        f = VC.case(name).facts
        assert (f["mbcols"], f["mbrows"], f["nparts"]) == (cols, rows, nparts)
        p = ops.webp_parse(VC.case(name).data)
        assert (p["mbcols"], p["mbrows"], p["nbr_partitions"]) == (cols, rows, nparts)
    assert ops.webp_probe(VC.case("geo_50x37").data) == (52, 40, 4, 3)
    assert all(b > 20 for b in VC.case("geo_1x9_p8").facts["part_bytes"][1:])        # row 8 wraps to partition 0; every partition is read
    assert all(f["mbcols"] <= 16 and f["mbrows"] <= 16 for f in (VC.case(n).facts for n in ALL))
    assert sum(VC.case(n).facts["nparts"] == 8 for n in VC.TIGHT) >= 1
    for name in VC.TIGHT:
        m = W.decode(VC.case(name).data)
        assert m["loaded"] == VC.case(name).facts["part_bytes"] and not m["err"]      # every partition ends on the last byte loaded
    assert VC.case("tight_9x1_p8").facts["part_bytes"][2:] == [0] * 7                  # nothing is loaded from a partition no row reads
    for name in ("unused_empty", "unused_empty_p4"):
        f = VC.case(name).facts
        assert f["part_bytes"][1] > 100 and not any(f["part_bytes"][2:]) and len(f["part_bytes"]) == 1 + f["nparts"]
    kinds = {VC.case(n).facts["short"] for n in VC.REFUSED}
    assert "p0" in kinds and 0 in kinds and {1, 3} <= kinds and 7 in kinds            # first partition, middle ones, last ones
    for name in VC.REFUSED:
        twin, whole = VC.case(name), VC.case(name.split("_short_")[0])
        assert len(twin.data) == len(whole.data) - 1
        assert sum(a - b for a, b in zip(whole.facts["part_bytes"], twin.facts["part_bytes"])) == 1


# ---------------------------------------------------------------------------------------------------- 3. the witnesses
@pytest.mark.parametrize("name", ALL)
def test_python_model(name):
    c = VC.case(name)
    m = W.decode(c.data)
    assert m["err"] == c.facts["refused"]
    if not c.facts["refused"]:
        same_arrays(m, c, "model")
        assert np.array_equal(m["skip"], c.facts["skip"])


@pytest.mark.parametrize("name", VC.ACCEPTED)
def test_host_parser_returns_what_was_written(name):
    same_arrays(ops.webp_parse(VC.case(name).data), VC.case(name), "ffhip_webp_parse")


@pytest.mark.parametrize("n_threads", [1, 5])
def test_host_batch_returns_what_was_written(n_threads):
    """every case and every one-byte-short twin in one call: the twins get FFHIP_EINVAL, their neighbours decode"""
    order = [ALL[i] for i in np.random.default_rng(3).permutation(len(ALL))]
    outs, status = ops.webp_parse_batch([VC.case(n).data for n in order], n_threads=n_threads)
    for n, o, st in zip(order, outs, status):
        if VC.case(n).facts["refused"]:
            assert st == capi.FFHIP_EINVAL and o is None, n
        else:
            assert st == 0, n
            same_arrays(o, VC.case(n), n)


@pytest.mark.parametrize("name", VC.REFUSED)
def test_one_byte_short_is_refused(name):
    c = VC.case(name)
    outs, status = ops.webp_parse_batch([c.data], n_threads=1)
    assert status == [capi.FFHIP_EINVAL] and outs == [None]
    # the frame header itself is whole in every twin: what runs dry is a macroblock header or a token
    assert header_status(c.data) == 0
    m = W.decode(c.data)
    assert m["err"] and not m["header_err"] and m["header_loaded"] < c.facts["part_bytes"][0]


# ---------------------------------------------------------------------------------------------------- 4. the reference
REF_OK = list(VC.REF_OK)


def test_the_reference_is_asked_about_every_case_it_can_take():
    assert set(REF_OK) == {n for n in ALL if VC.case(n).facts["ref_ok"]}
    for n in set(ALL) - set(REF_OK):
        f = VC.case(n).facts
        assert f["nparts"] == 8 or f["height"] % 16 or f["skip"][0] or f["refused"], n


@pytest.mark.parametrize("name", REF_OK)
def test_reference_decodes_the_case_files_to_the_oracle_pixels_of_the_written_arrays(name, tmp_path):
    """The reference's whole-file decode == the oracle chain (residual, prediction, loop filter, colour) run on the WRITTEN arrays
    (O.check_ref: element for element where the reference is built, by the recorded digest elsewhere).  This is the test that catches a
    typo in a constant table the writer shares with the library (the coefficient update and default probabilities and the 4x4 mode
    probabilities of ffhip_vp8_tables.h): writer and parser read the same header and would be wrong together, the reference would not.
    unused_empty_p4 is here too: the reference decodes a file whose unread token partitions have length zero."""
    c = VC.case(name)
    p = ops.webp_parse(c.data)                  # for the header only: sizes, quantisers, filter parameters
    info = np.zeros((len(c.mbinfo), 32), np.uint8)
    info[:, :27] = c.mbinfo
    written = dict(p, modes=c.modes.copy(), levels=c.levels.copy(), mbinfo=info, resmap=c.resmap.copy())
    rows, width_bytes = min(p["height"], 16 * p["mbrows"]), min(4 * p["width"], 64 * p["mbcols"])
    mine = np.ascontiguousarray(oracle_bgra(written, oracle_residual(written))[:rows, :width_bytes])

    def reference():
        import make_golden
        path = str(tmp_path / (name + ".webp"))
        open(path, "wb").write(c.data)
        d = make_golden.ref_decode_webp(path)
        assert [int(x) for x in d["dims"][:2]] == [p["width"], p["height"]]
        return np.ascontiguousarray(d["bgra"][:rows, :width_bytes])
    O.check_ref("vp8_known/" + name, mine, reference)
