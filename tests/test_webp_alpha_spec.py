"""CPU: the alpha rule of lossy WebP files held three ways.  The answer key (webp_alpha_writer.py: files from known planes), the witness
(webp_alpha_spec.py: the rule in plain Python) and libwebp through PIL must agree on EVERY case of webp_alpha_cases.py; the witness equals
PIL on files PIL's own encoder writes; and among the damaged files and several hundred truncated and bit-flipped copies the witness refuses
exactly what PIL refuses -- and gives PIL's plane where both accept.  Byte for byte, no copy left out."""
import io
import os
import sys

import numpy as np
import pytest

import webp_alpha_cases as K
import webp_alpha_spec as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_webp_alpha as golden  # noqa: E402

Image = pytest.importorskip("PIL.Image")
features = pytest.importorskip("PIL.features")
if not features.check("webp"):
    pytest.skip("PIL without WebP", allow_module_level=True)

CASE_IDS = [c.name for c in K.cases()]


def pil_rgba(data):
    """PIL's RGBA [h][w][4], or None where it refuses the file"""
    try:
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
    except Exception:
        return None


def witness_plane(data):
    try:
        return S.plane(data)
    except S.Refused:
        return None


@pytest.mark.parametrize("k", range(len(CASE_IDS)), ids=CASE_IDS)
def test_witness_and_pil_give_the_answer_key(k):
    c = K.cases()[k]
    pil = pil_rgba(c.data)
    if c.plane is None:                                           # the file stays opaque
        assert S.find(c.data) is None
        assert (pil is None) == (c.name in K.PIL_REFUSES)         # the two named deviations
        assert pil is None or (pil[..., 3] == 255).all()
        return
    a = S.find(c.data)
    assert (a["compression"], a["filter"], a["pre"]) == (c.compression, c.filter, c.pre)
    got = S.plane(c.data)
    assert got.shape == c.plane.shape and np.array_equal(got, c.plane), np.argwhere(got != c.plane)[:4].tolist()
    assert pil is not None and np.array_equal(pil[..., 3], c.plane), np.argwhere(pil[..., 3] != c.plane)[:4].tolist()


def test_colour_is_the_carriers():
    """no premultiplication: PIL's RGB of a file with alpha is that of its VP8 chunk alone"""
    by = {c.name: c for c in K.cases()}
    for name, (w, h) in (("h65-w5-raw-f1", (5, 65)), ("predictor-f3", (20, 9))):
        assert np.array_equal(pil_rgba(by[name].data)[..., :3], pil_rgba(K.carrier(w, h))[..., :3]), name


def test_the_cases_cover_what_the_issue_lists():
    cs = [c for c in K.cases() if c.plane is not None]
    for f in range(4):
        assert {c.plane.shape[1] for c in cs if c.filter == f} >= set(K.WIDTHS), f
        assert {c.plane.shape[0] for c in cs if c.filter == f} >= set(K.HEIGHTS), f
        for comp in (0, 1):
            assert {c.plane.shape[1] for c in cs if c.filter == f and c.compression == comp} >= set(K.WIDTHS), (f, comp)
            assert {c.plane.shape[0] for c in cs if c.filter == f and c.compression == comp} >= set(K.HEIGHTS), (f, comp)
        assert {c.kind for c in cs if c.filter == f} >= {"", "plain", "predictor", "palette", "cache"}, f
    assert any(c.pre == 1 for c in cs) and sum(c.plane is None for c in K.cases()) >= 5
    assert any(len(dict(__import__("webp_alpha_writer").chunks_of(c.data))[b"ALPH"]) & 1 for c in cs)
    assert {d.name for d in K.damaged_cases()} >= {"raw-short", "payload-empty", "compression-2", "pre-processing-2", "reserved-bit-6",
                                                   "lossless-truncated", "lossless-over-subscribed"}


def test_witness_equals_pil_on_the_encoders_files():
    stored = golden.load()
    fresh = golden.files()
    assert [n for n, _ in fresh] == [n for n, _, _ in stored]
    kinds = set()
    for (name, data), (_, kept, pixels) in zip(fresh, stored):
        assert np.array_equal(S.plane(data), pil_rgba(data)[..., 3]), name
        assert np.array_equal(pil_rgba(kept)[..., [2, 1, 0, 3]], pixels) and np.array_equal(S.plane(kept), pixels[..., 3]), name
        a = S.find(kept)
        kinds.add((a["compression"], a["filter"], a["pre"]))
    assert kinds >= {(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 2, 0), (1, 3, 0)}


def test_witness_refuses_what_pil_refuses():
    for d in K.damaged_cases():
        assert pil_rgba(d.data) is None and witness_plane(d.data) is None, d.name
    f = K.lenient_end()                                           # ... and accepts the one kind of cut stream PIL accepts, with its plane
    assert np.array_equal(witness_plane(f), pil_rgba(f)[..., 3])


def mangled_sources():
    by = {c.name: c for c in K.cases()}
    names = ("w17-h3-raw-f2", "w5-h3-lossless-f1", "predictor-f1", "palette-f0", "palette-f2", "cache-f3", "palette-one-symbol-codes")
    stored = {n: d for n, d, _ in golden.load()}
    kept = ("mask-3x5-m0-a100", "mask-17x9-m4-a100", "grad-17x9-m0-a100", "soft-50x37-m4-a100", "noise-3x5-m4-a50", "soft-17x9-m6-a0")
    return [(n, by[n].data) for n in names] + [(n, stored[n]) for n in kept]


def test_truncated_and_bit_flipped_copies():
    copies = K.mangled(mangled_sources())
    assert len(copies) >= 300
    accepted = 0
    for name, data in copies:
        pil, wit = pil_rgba(data), witness_plane(data)
        assert (pil is None) == (wit is None), (name, "PIL refuses" if pil is None else "PIL accepts")
        if pil is not None:
            accepted += 1
            assert np.array_equal(pil[..., 3], wit), name
    assert 20 <= accepted < len(copies) - 20                      # both verdicts are well represented
