"""CPU: the witness of the lossy WebP encoder's rule (tests/vp8_encode_spec.py) against the outside world.  For every
case of tests/vp8_encode_cases.py the file the witness writes with tests/vp8_writer.keyframe_from(valid=True) is opened by PIL (libwebp), and
PIL's pixels are those of the spec decoder tests/vp8_spec.py with rules=SPEC; with filter 0 the decoded planes ARE the witness's
reconstruction; and the forward transforms the rule states are inverses of RFC 6386's within 1."""
import io

import numpy as np
import pytest
from PIL import Image

import vp8_encode_spec as E
import vp8_spec as S
from vp8_encode_cases import CASES

DECODED = {}


def decoded(case):
    if case.id not in DECODED:
        DECODED[case.id] = S.decode(E.file(case.pixels, case.quality, case.filter), rules=S.SPEC)
    return DECODED[case.id]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_libwebp_decodes_the_witness_file_to_the_spec_pixels(case):
    data = E.file(case.pixels, case.quality, case.filter)
    im = Image.open(io.BytesIO(data))
    assert im.format == "WEBP" and im.size == (case.pixels.shape[1], case.pixels.shape[0])
    d = decoded(case)
    assert not d["refused"]
    assert np.array_equal(np.asarray(im.convert("RGB")), d["rgb"])


@pytest.mark.parametrize("case", [c for c in CASES if c.filter == 0], ids=[c.id for c in CASES if c.filter == 0])
def test_the_decoded_planes_are_the_reconstruction(case):
    d, m = decoded(case), E.encode_mbs(case.pixels, case.quality)
    assert d["filter_type"] == 0
    for k in "yuv":
        assert np.array_equal(d[k], m[k]), k
    assert np.array_equal(d["levels"], m["levels"]) and np.array_equal(d["skip"], m["skip"])
    assert np.array_equal(d["modes"][:, 0], m["ymode"]) and np.array_equal(d["modes"][:, 1], m["uvmode"])


def test_the_header_is_the_rule():
    for case in CASES:
        d, hd = decoded(case), E.header(case.pixels, case.quality, case.filter)
        rows = (case.pixels.shape[0] + 15) >> 4
        assert d["nbr_partitions"] == 1 << hd["log2_parts"] == max(p for p in (1, 2, 4, 8) if p <= min(8, rows)), case.id
        assert [int(v) for v in d["quant"][0]] == E.steps(E.quality_index(case.quality)), case.id
        assert d["filter_type"] == (2 if hd["level"] else 0), case.id
    assert [E.quality_index(q) for q in (0, 30, 75, 100)] == [127, 52, 26, 0] and len(E.QUALITY_QI) == 101
    assert E.auto_filter(26) == 8 and E.auto_filter(127) == 39


def test_the_cases_reach_what_they_are_for():
    by = {c.id: E.encode_mbs(c.pixels, c.quality) for c in CASES}
    assert by["flat-all-skipped"]["skip"].all() and not by["33x47"]["skip"].any()
    assert np.abs(by["checkerboard-noise-q100"]["levels"]).max() >= 67                      # cat6 tokens
    assert by["16x130-8-partitions"]["rows"] == 9 and by["48x24-2-partitions"]["rows"] == 2
    modes = set()
    for m in by.values():
        modes |= {("y", int(v)) for v in m["ymode"]} | {("uv", int(v)) for v in m["uvmode"]}
    assert modes == {(p, k) for p in ("y", "uv") for k in range(4)}


def test_forward_and_inverse_transforms_round_trip_within_one():
    rng = np.random.default_rng(5)
    R = S._Rules(S.SPEC)
    worst = 0
    for k in range(3000):
        d = rng.integers(-255, 256, 16) if k % 3 else rng.integers(-12, 13, 16)
        worst = max(worst, int(np.abs(np.array(S._idct(E.fdct(d), R)) - d).max()))
        x = rng.integers(-2040, 2041, 16)
        worst = max(worst, int(np.abs(np.array(S._iwht(E.fwht(x))) - x).max()))
    assert worst <= 1
