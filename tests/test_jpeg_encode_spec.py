"""CPU: the encoder's witness (tests/jpeg_encode_spec.py) against PIL's own encoder (libjpeg-turbo), byte for byte, on every case of
tests/jpeg_encode_cases.py; and against this repository's entropy decoder, coefficient for coefficient.  The library is not in this
module: test_jpeg_encode_capi.py and test_jpeg_encode_gpu.py hold it to the witness."""
import inspect
import io

import numpy as np
import pytest

import jpeg_encode_spec as spec
import jpeg_entropy
from jpeg_encode_cases import CASES

SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pil_bytes(case):
    Image = pytest.importorskip("PIL.Image")
    from PIL import JpegImagePlugin
    if "restart_marker_blocks" not in inspect.getsource(JpegImagePlugin):
        pytest.skip("this PIL has no restart_marker_blocks")
    px = case.pixels
    im = Image.fromarray(px, "L" if px.ndim == 2 else "RGB")
    buf = io.BytesIO()
    kw = dict(quality=case.quality, restart_marker_blocks=case.restart)
    if px.ndim == 3:
        kw["subsampling"] = SUBSAMPLING[case.layout]
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_witness_file_is_pils(case):
    want = pil_bytes(case)
    got = case.key[2]
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, next(i for i in range(len(got)) if got[i] != want[i])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_witness_file_decodes_to_its_coefficients(case):
    coef, quant, data = case.key
    d = jpeg_entropy.decode(data)
    h, v, ncomp = spec.LAYOUTS[case.layout]
    assert (d["width"], d["height"], d["h"], d["v"], d["ncomp"]) == (case.width, case.height, h, v, ncomp)
    for c in range(ncomp):
        assert np.array_equal(d["coef"][c], coef[c]), c
        assert np.array_equal(d["quant"][d["qt_id"][c]], quant[min(c, 1)])


def test_tables_at_the_ends_of_the_quality_scale():
    assert (spec.tables(100)[:2] == 1).all()
    assert spec.tables(1)[0].max() == 255 and spec.tables(0)[0].tolist() == spec.tables(1)[0].tolist()
    assert spec.tables(50)[0].tolist() == spec.STD_LUMA.tolist() and spec.tables(50)[1].tolist() == spec.STD_CHROMA.tolist()


def test_the_large_cases_are_what_the_issue_says():
    """noise at 100x75, 4:4:4, quality 100: larger than its pixels, some two hundred stuffed bytes"""
    case = next(c for c in CASES if c.id == "100x75-4:4:4-q100-r0-noise")
    data = case.key[2]
    scan = data[data.index(b"\xff\xda"):]
    assert len(data) > 100 * 75 * 3 and 100 < scan.count(b"\xff\x00") < 400, (len(data), scan.count(b"\xff\x00"))
