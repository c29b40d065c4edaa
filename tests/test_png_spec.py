"""CPU: the PNG witness (png_spec.py) itself, and the library's host decoder (ops.png_picture) beside it on the same expectations.  Against the writer's answer key on every case; against PIL on exactly the kinds PIL can
witness -- colour types 2, 4 and 6 at 8 and 16 bits, grey at 1/2/4/8 without tRNS, grey 8 and RGB 8 with tRNS, palette at every depth with
tRNS, Adam7 --; and against hand-computed pixels on the kinds it cannot: grey 16 (PIL gives I;16 and clips it), grey below 8 bits with tRNS
and RGB 16 with tRNS (PIL ignores the chunk)."""
import io

import numpy as np
import pytest

import png_cases
import png_spec
import png_writer as W
from ffpic_amd import ops


def pil_can_witness(c):
    if c.ctype == 0:
        return c.depth <= 8 and (c.trns is None or c.depth == 8)
    if c.ctype == 2:
        return c.trns is None or c.depth == 8
    return True


@pytest.mark.parametrize("k", range(len(png_cases.cases())), ids=[c.name for c in png_cases.cases()])
def test_witness_gives_the_answer_key(k):
    c = png_cases.cases()[k]
    key = W.expected_bgra(c.samples, c.ctype, c.depth, c.palette, c.trns)
    assert np.array_equal(png_cases.expected()[k], key)
    assert np.array_equal(ops.png_picture(c.data), key)


def test_witness_against_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    s = png_cases.random_samples(rng, 5, 9, 0, 8)
    s[::2, ::2, 0] = 77
    extra = [png_cases.Case("trns_grey8", W.write(s, 0, 8, filters=[4, 3, 1], trns=b"\x00\x4d"), s, 0, 8, False, None, b"\x00\x4d")]
    seen = 0
    for c in png_cases.cases() + extra:
        if not pil_can_witness(c):
            continue
        rgba = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGBA"))
        assert np.array_equal(png_spec.decode(c.data), rgba[..., [2, 1, 0, 3]]), c.name
        assert np.array_equal(ops.png_picture(c.data), rgba[..., [2, 1, 0, 3]]), c.name
        seen += 1
    assert seen >= 40 and any(c.interlace for c in png_cases.cases())


def bgra(*pixels):
    return np.array(pixels, np.uint8).reshape(1, -1, 4)


def both(data):
    """the witness's picture, which the library's host decoder has to give too"""
    got = png_spec.decode(data)
    assert np.array_equal(ops.png_picture(data), got)
    return got


def test_grey_16_is_its_high_byte():
    s = np.array([[[0x1234], [0xffee], [0x00ff], [0x0100]]])
    got = both(W.write(s, 0, 16, filters=1))
    assert np.array_equal(got, bgra((0x12, 0x12, 0x12, 255), (0xff, 0xff, 0xff, 255), (0, 0, 0, 255), (1, 1, 1, 255)))


def test_trns_on_grey_below_8_bits_is_compared_before_scaling():
    s = np.array([[[0], [1], [2], [3]]])
    got = both(W.write(s, 0, 2, trns=b"\x00\x02"))
    assert np.array_equal(got, bgra((0, 0, 0, 255), (85, 85, 85, 255), (170, 170, 170, 0), (255, 255, 255, 255)))
    got = both(W.write(s[:, :2], 0, 1, trns=b"\x00\x00"))
    assert np.array_equal(got, bgra((0, 0, 0, 0), (255, 255, 255, 255)))
    s = np.array([[[15], [14], [0]]])
    got = both(W.write(s, 0, 4, trns=b"\x00\x0f"))
    assert np.array_equal(got, bgra((255, 255, 255, 0), (238, 238, 238, 255), (0, 0, 0, 255)))


def test_trns_at_16_bits_is_compared_before_stripping():
    s = np.array([[[0x1234], [0x1235], [0x1334]]])
    got = both(W.write(s, 0, 16, trns=b"\x12\x34"))
    assert np.array_equal(got, bgra((0x12, 0x12, 0x12, 0), (0x12, 0x12, 0x12, 255), (0x13, 0x13, 0x13, 255)))
    s = np.array([[[0x0102, 0x0304, 0x0506], [0x0102, 0x0304, 0x0507], [0x0102, 0x0304, 0x0606]]])
    got = both(W.write(s, 2, 16, filters=4, trns=b"\x01\x02\x03\x04\x05\x06"))
    assert np.array_equal(got, bgra((5, 3, 1, 0), (5, 3, 1, 255), (6, 3, 1, 255)))


def test_adam7_1x1_has_pass_1_only():
    lay = png_spec.layout(png_cases.cases()[[c.name for c in png_cases.cases()].index("adam7_1x1")].data)
    assert lay["n_passes"] == 1 and lay["pass_rows"] == [1, 0, 0, 0, 0, 0, 0] and lay["filtered_bytes"] == 5
    info = ops.png_probe(png_cases.cases()[[c.name for c in png_cases.cases()].index("adam7_1x1")].data)
    assert info.n_passes == 1 and list(info.pass_rows) == [1, 0, 0, 0, 0, 0, 0] and info.filtered_bytes == 5


def test_witness_refuses_what_the_rule_refuses():
    from ffpic_amd import capi
    for name, data in png_cases.damaged():
        with pytest.raises(png_spec.Refused):
            png_spec.decode(data)
        with pytest.raises(capi.FfhipError):
            ops.png_picture(data)
