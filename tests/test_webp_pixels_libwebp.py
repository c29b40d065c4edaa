"""pixels='libwebp' without a GPU: the host front end under the rule (ffhip_webp_parse_ex, ffhip_webp_probe_ex) and the two bodies the
kernels compile (ffhip_vp8_libwebp_residual_mb, ffhip_webp_libwebp_color) against the witness, tests/vp8_spec.py with rules=SPEC, on the
81 corpus files, the files of webp_libwebp_more.npz and crafted inputs.  No tolerance anywhere."""
import numpy as np
import pytest

import vp8_spec as S
from ffpic_amd import capi, ops, tensors
from webp_pixels_cases import CORPUS, NAMES, data_of, pil_rgb, witness

SPEC = S._Rules(S.SPEC)


def assert_parse_is_witness(p, w, what):
    for key in ("width", "height", "mbcols", "mbrows", "nbr_partitions", "filter_type"):
        assert p[key] == w[key], (what, key, p[key], w[key])
    assert np.array_equal(p["modes"], w["modes"]), (what, "modes")
    assert np.array_equal(p["levels"], w["levels"]), (what, "levels")
    assert np.array_equal(p["mbinfo"][:, :25], w["counts"]), (what, "token counts")
    assert np.array_equal(p["mbinfo"][:, 25], w["modes"][:, 0] != 4), (what, "has_y2")
    assert np.array_equal(p["mbinfo"][:, 26], w["modes"][:, 18]), (what, "segment ids")
    assert np.array_equal(p["resmap"], np.arange(len(w["modes"]))), (what, "the residual map is the identity")
    assert np.array_equal(p["quant"][:, :6], w["quant"]) and not p["quant"][:, 6:].any(), (what, "quantisers", p["quant"], w["quant"])
    assert np.array_equal(p["filters"], w["filters"]), (what, "filter parameters")


def test_the_witness_gives_pils_pictures():
    """the oracle of everything below: SPEC is PIL's RGB on every file, the new ones included"""
    for name in NAMES:
        assert np.array_equal(witness(name)["rgb"], pil_rgb(name)), name


def test_parse_ex_returns_the_witness_arrays_and_refuses_no_file():
    for name in NAMES:
        w = witness(name)
        assert not w["refused"], name
        assert_parse_is_witness(ops.webp_parse(data_of(name), pixels="libwebp"), w, name)
        # the skip flags: a skipped macroblock has no tokens and zero levels
        p = ops.webp_parse(data_of(name), pixels="libwebp")
        sk = w["skip"].astype(bool)
        assert not p["levels"][sk].any() and not p["mbinfo"][sk][:, :25].any(), name


@pytest.mark.parametrize("name", ["pil_noise_16x16_q100_m4", "wr_seg_delta", "wr_parts2", "wm_size_17x17"])
def test_every_truncation_gets_the_witness_verdict(name):
    data = data_of(name)
    for n in range(len(data)):
        cut = data[:n]
        try:
            w = S.decode(cut, S.SPEC, pixels=False)
        except S.Refused:
            w = None
        try:
            p = ops.webp_parse(cut, pixels="libwebp") if n else None
        except capi.FfhipError:
            p = None
        if w is None or w["refused"]:
            assert p is None, (name, n, "the witness refuses this truncation")
        else:
            assert p is not None, (name, n, "the witness decodes this truncation")
            assert_parse_is_witness(p, w, (name, n))


def test_probe_ex_gives_the_frame_tags_sizes():
    data = data_of("pil_noise_50x37_q30_m4")
    assert ops.webp_probe(data, pixels="libwebp") == (50, 37, 4, 3)
    assert ops.webp_probe(data) == (52, 40, 4, 3)               # the default rule rounds up to 4
    for name in NAMES:
        w = witness(name)
        assert ops.webp_probe(data_of(name), pixels="libwebp") == (w["width"], w["height"], w["mbcols"], w["mbrows"]), name


def want_residual(levels, counts, has_y2, q):
    res, nz = S._residual(levels, counts, has_y2, q, SPEC)
    # the entry's residual is int16 and saturates; the add-and-clip to 8 bits behind it cannot tell (ffhip_vp8_libwebp_body.h)
    return np.clip(res, -32768, 32767), bool(nz)


def check_residual(levels, has_y2, q, what):
    got, nz = ops.vp8_libwebp_residual_mb(levels, has_y2, q)
    want, wnz = want_residual(levels, np.full(25, 16), has_y2, q)
    assert np.array_equal(got, want) and nz == wnz, (what, np.argwhere(got != want)[:4], nz, wnz)


def test_residual_mb_is_the_witness_on_every_macroblock():
    for name in NAMES:
        w = witness(name)
        for mb in range(len(w["modes"])):
            check_residual(w["levels"][mb], w["modes"][mb, 0] != 4, w["quant"][w["modes"][mb, 18]], (name, mb))


def test_residual_mb_crafted():
    q = np.array([8, 10, 16, 20, 8, 10], np.uint16)
    z = np.zeros((25, 16), np.int16)
    # first-pass sums at +-32767 and +-32768: c[0] + c[8] with no odd terms is t[0] itself
    for a, b in ((32767, 0), (16384, 16383), (16384, 16384), (-16384, -16384), (-16384, -16383), (32767, 32767), (-32768, -32768), (32767, -32768)):
        lv = z.copy()
        lv[17, 0], lv[17, 8] = a, b
        check_residual(lv, True, np.array([1, 1, 1, 1, 1, 1], np.uint16), ("pass 1", a, b))
        lv = z.copy()
        lv[3, 1], lv[3, 9], lv[3, 4], lv[3, 12] = a, b, a, b
        check_residual(lv, False, np.array([1, 1, 1, 1, 1, 1], np.uint16), ("pass 1, B_PRED luma", a, b))
    # the wrapping product: 512 x 128 = 65536 is 0, 256 x 128 is -32768
    lv = z.copy()
    lv[5, 3] = 512
    got, nz = ops.vp8_libwebp_residual_mb(lv, False, np.array([8, 128, 16, 20, 8, 10], np.uint16))
    assert not got.any() and not nz
    check_residual(lv, False, np.array([8, 128, 16, 20, 8, 10], np.uint16), "wrap to 0")
    lv[5, 3] = 256
    check_residual(lv, False, np.array([8, 128, 16, 20, 8, 10], np.uint16), "wrap to -32768")
    # Y2 DCs that cancel to zero: the Y2 block has coefficients, every luma DC it gives is 0 (a DC of 1 x 2 rounds to 0: (2 + 3) >> 3)
    lv = z.copy()
    lv[24, 0] = 1
    got, nz = ops.vp8_libwebp_residual_mb(lv, True, np.array([8, 10, 2, 20, 8, 10], np.uint16))
    assert not got.any() and not nz
    check_residual(lv, True, np.array([8, 10, 2, 20, 8, 10], np.uint16), "Y2 cancels")
    lv[24, 0], lv[24, 1] = 40, -3
    check_residual(lv, True, q, "Y2 with a wrapping-free DC pattern")
    lv[24, 0] = 32767
    check_residual(lv, True, np.array([8, 10, 314, 439, 8, 10], np.uint16), "Y2 DC wraps")
    # a lone AC with zero DC goes through the IDCT: the residual is not the coefficient itself
    lv = z.copy()
    lv[2, 1] = 7
    got, nz = ops.vp8_libwebp_residual_mb(lv, False, q)
    assert nz and got[2, 1] != 70 and np.array_equal(got[2], S._idct([0, 70] + [0] * 14, SPEC))
    check_residual(lv, False, q, "lone AC")
    rng = np.random.default_rng(5)
    for k in range(200):
        lv = (rng.integers(-2048, 2048, (25, 16)) * (rng.random((25, 16)) < 0.3)).astype(np.int16)
        has_y2 = bool(k & 1)
        if has_y2:
            lv[:16, 0] = 0
        check_residual(lv, has_y2, rng.integers(4, 315, 6).astype(np.uint16), ("random", k))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (17, 5), (64, 2), (65, 3)])
def test_color_is_to_rgb_on_random_planes(w, h):
    rng = np.random.default_rng(100 * w + h)
    for _ in range(4):
        y, u, v = rng.integers(0, 256, (h, w)), rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2)), rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2))
        got = ops.webp_libwebp_color(y, u, v, pitch=4 * w + 16)
        assert np.array_equal(got[:, :, 2::-1], S.to_rgb(y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8))) and (got[:, :, 3] == 255).all()


def test_color_is_to_rgb_on_every_files_planes():
    for name in NAMES:
        w = witness(name)
        hh, ww = w["rgb"].shape[:2]
        got = ops.webp_libwebp_color(w["y"][:hh, :ww], w["u"][:(hh + 1) // 2, :(ww + 1) // 2], w["v"][:(hh + 1) // 2, :(ww + 1) // 2])
        assert np.array_equal(got[:, :, 2::-1], pil_rgb(name)) and (got[:, :, 3] == 255).all(), name


def test_every_decode_side_rule_is_asked_for_by_some_file():
    """the corpus reaches every rule the pixel rule changes: each flag but the one no single libwebp picture exists for"""
    asked = set()
    for name in CORPUS:
        asked |= witness(name)["asked"]
    assert set(S.FLAGS) - asked <= {"idct_pass1_int16", "reference_colour"}, set(S.FLAGS) - asked


def test_value_errors():
    data = data_of(CORPUS[0])
    for call in (lambda p: ops.webp_probe(data, pixels=p), lambda p: ops.webp_parse(data, pixels=p), lambda p: ops.webp_parse_device([data], pixels=p),
                 lambda p: ops.webp_decode_files_device([data], pixels=p), lambda p: tensors.decode_webp_to_tensors([data], pixels=p),
                 lambda p: tensors.webp_entry_point(p)):
        for bad in ("libjpeg", "", None, "LIBWEBP"):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        ops.webp_decode_files_device([data], planes=True)       # the default rule's file call writes no planes
    with pytest.raises(ValueError):
        ops.webp_libwebp_color(np.zeros((4, 4)), np.zeros((2, 2)), np.zeros((2, 3)))


def test_the_ninth_entry_stands_beside_the_table():
    assert tensors.webp_entry_point("libwebp") == "ffhip_webp_decode_files_tensor_ex" not in tensors._ENTRY_TAILS
    assert len(tensors._ENTRY_TAILS) == 8 and tensors._WEBP_EX_TAIL == ("resize", "orient", "flags")
    for oriented in (False, True):
        for targets in (False, True):
            assert tensors.webp_entry_point("reference", oriented, targets) == tensors.entry_point("webp", oriented, 1, targets)
    assert "ffhip_webp_decode_files_tensor_ex" in capi.EXPORTS
