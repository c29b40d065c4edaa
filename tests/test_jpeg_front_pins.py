"""CPU: the JPEG host front ends -- ffhip_jpeg_probe, ffhip_jpeg_probe_any, ffhip_jpeg_exif_orientation, the two host decoders and the tables
handed to the device -- say of every file of tests/jpeg_front_cases.py what they said before they shared one marker walk, one frame record and one
table builder.  tests/golden/jpeg_front_pins.json holds the earlier commit's verdicts (tests/golden/make_jpeg_front_pins.py)."""
import functools
import json
import os

import jpeg_front_cases as FC
from ffpic_amd import capi

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_front_pins.json")


@functools.lru_cache(maxsize=None)
def _pins():
    """{tag: (digest, probe code, probe_any code, progressive flag)}"""
    return {row[0]: tuple(row[1:]) for row in json.load(open(PINS))["cases"]}


def test_the_pins_are_not_vacuous():
    """of the cases seeded from baseline files ffhip_jpeg_probe accepts a quarter at least and refuses a quarter at least; the same of the
    cases seeded from progressive files and the progressive leg of ffhip_jpeg_probe_any"""
    pins = _pins()
    base = [v for tag, v in pins.items() if tag.startswith("b.")]
    prog = [v for tag, v in pins.items() if tag.startswith("p.")]
    assert len(base) >= 1000 and len(prog) >= 400
    for n, accepted, refused in ((len(base), sum(v[1] == 0 for v in base), sum(v[1] != 0 for v in base)),
                                 (len(prog), sum(v[2] == 0 and v[3] == 1 for v in prog), sum(v[2] != 0 for v in prog))):
        assert 4 * accepted >= n and 4 * refused >= n, (n, accepted, refused)
    # the sixteen refusal files, as they are, are refused
    whole = [v for tag, v in pins.items() if tag.startswith("r.") and tag.count(".") == 1]
    assert len(whole) == 16 and all(v[2] == capi.FFHIP_EINVAL for v in whole)


def test_the_parsers_differ_where_the_design_says_they_do():
    """per difference of policy between the two parsers a baseline file and its progressive twin: ffhip_jpeg_probe's code for
    the one is not the code of ffhip_jpeg_probe_any's progressive leg for the other"""
    pins = _pins()
    for what, (b, p) in FC.TWINS.items():
        assert pins[b][3] == 0 and pins[p][1] == capi.FFHIP_EINVAL, what      # neither file is taken by the other parser
        assert pins[b][1] != pins[p][2], what
        assert {pins[b][1], pins[p][2]} == {0, capi.FFHIP_EINVAL}, what


def test_every_case_gives_its_pinned_verdict():
    pins = _pins()
    cases = FC.cases()
    assert [tag for tag, _ in cases] == list(pins)                  # no case left out, none added
    L = capi.lib()
    wrong = [tag for tag, data in cases if FC.verdict(L, data) != pins[tag]]
    assert not wrong, (len(wrong), wrong[:20])
