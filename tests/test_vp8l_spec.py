"""CPU: the lossless WebP rule held three ways.  The answer key (vp8l_writer.py: files from known pixels), the witness (vp8l_spec.py: the
rule in numpy and plain Python) and libwebp through PIL must agree on EVERY case of vp8l_cases.py; the witness equals PIL on files PIL's own
encoder writes; and the witness refuses exactly what PIL refuses among the damaged files.  Byte for byte, no case left out."""
import io
import os
import sys

import numpy as np
import pytest

import vp8l_cases
import vp8l_spec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_vp8l as golden  # noqa: E402

Image = pytest.importorskip("PIL.Image")
features = pytest.importorskip("PIL.features")
if not features.check("webp"):
    pytest.skip("PIL without WebP", allow_module_level=True)

CASE_IDS = [c.name for c in vp8l_cases.cases()]


def pil_bgra(data):
    im = Image.open(io.BytesIO(data))
    return im.mode, np.asarray(im.convert("RGBA"))[..., [2, 1, 0, 3]]


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_witness_and_pil_give_the_answer_key(k):
    c, want = vp8l_cases.cases()[k], vp8l_cases.expected()[k]
    got = vp8l_spec.decode(c.data)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    mode, pil = pil_bgra(c.data)
    assert mode == ("RGBA" if c.alpha else "RGB")                 # the VP8L bit decides, whatever a VP8X chunk says
    assert pil.shape == want.shape and np.array_equal(pil, want), np.argwhere(pil != want)[:4].tolist()
    p = vp8l_spec.parse(c.data)
    assert tuple(t["type"] for t in p["transforms"]) == c.types and p["cache_bits"] == c.cache_bits and p["meta"] == c.meta


def test_the_cases_cover_what_the_issue_lists():
    cs = vp8l_cases.cases()
    sizes = {(c.argb.shape[1], c.argb.shape[0]) for c in cs}
    assert {(1, 1), (1, 7), (7, 1), (5, 7), (4, 4), (33, 17), (65, 130), (130, 65)} <= sizes
    assert {c.cache_bits for c in cs} >= {0, 1, 4, 11} and any(c.meta for c in cs) and sum(c.host for c in cs) == 2
    assert {c.types for c in cs} >= {(), (2,), (2, 0), (2, 0, 1), (0, 1), (0,), (3,), (3, 0), (0, 3), (2, 3)}
    assert any(not c.alpha for c in cs) and any(c.orientation == 6 for c in cs)


def test_witness_equals_pil_on_the_encoders_files():
    stored = golden.load()
    fresh = golden.files()
    assert [n for n, _ in fresh] == [n for n, _, _ in stored]
    kinds = set()
    for (name, data), (_, kept, pixels) in zip(fresh, stored):
        _, pil = pil_bgra(data)                                   # PIL's DECODE, not the source: without `exact` colour under alpha 0 is rewritten
        assert np.array_equal(vp8l_spec.decode(data), pil), name
        assert np.array_equal(pil_bgra(kept)[1], pixels) and np.array_equal(vp8l_spec.decode(kept), pixels), name
        kinds.add(tuple(t["type"] for t in vp8l_spec.parse(data)["transforms"]))
    assert len(kinds) >= 5                                        # the encoder's transform orders, palette and none included


def test_witness_refuses_what_pil_refuses():
    for d in vp8l_cases.damaged_cases():
        try:
            Image.open(io.BytesIO(d.data)).convert("RGBA")
            pil_refuses = False
        except Exception:
            pil_refuses = True
        try:
            vp8l_spec.decode(d.data)
            code = 0
        except vp8l_spec.Animation:
            code = vp8l_cases.EANIMATION
        except vp8l_spec.Refused:
            code = vp8l_cases.EINVAL
        assert pil_refuses and code == d.code, d.name
