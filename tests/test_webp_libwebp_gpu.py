"""The device side of the WebP path against tests/vp8_spec.py under its REFERENCE rules, on the corpus of
tests/golden/webp_libwebp.npz (files libwebp decodes; tests/test_webp_libwebp.py holds the witness to libwebp and to the tree's CPU
side).  The two bool-decoder kernels, the file call and the planes of ffhip_vp8_decode_frames each get a witness here that shares no
code with them.  Reads the npz only; a file the REFERENCE rules refuse must get a status, every other one 0."""
import functools

import numpy as np
import pytest

import vp8_spec as S
from ffpic_amd import capi, ops
from test_webp_libwebp import CNAMES, data_of, planes_to_bgra, refused_by_witness, witness

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    for n in ("FFHIP_WEBP_GPU_ENTROPY", "FFHIP_WEBP_PACK"):
        capi.setenv(n, None)


@functools.lru_cache(maxsize=None)
def want_bgra(name):
    return planes_to_bgra(witness(name, S.REFERENCE))


def first_macroblock(a, b, size, cols):
    at = np.argwhere(a != b)[0]
    return f"macroblock {int(at[0]) // size * cols + int(at[1]) // size} (row {at[0]}, column {at[1]})"


@pytest.mark.parametrize("pack", [None, 5])
def test_kernels_a_and_b_against_the_witness(pack):
    """one call for the whole corpus; pack = 5: five frames to a wave, divergent"""
    capi.setenv("FFHIP_WEBP_PACK", pack)
    dev, status = ops.webp_parse_device([data_of(n) for n in CNAMES])
    assert 4 * status.count(0) >= 3 * len(CNAMES)      # the comparison below is about most of the corpus
    for n, d, st in zip(CNAMES, dev, status):
        assert (st != 0) == refused_by_witness(n), n
        if st:
            assert st == capi.FFHIP_EINVAL and d is None
            continue
        o = witness(n, S.REFERENCE)
        for k in ("width", "height", "mbcols", "mbrows", "nbr_partitions", "filter_type"):
            assert d[k] == o[k], (n, k)
        assert np.array_equal(d["modes"], o["modes"]), (n, "kernel A: mode records")
        assert np.array_equal(d["resmap"], o["resmap"]), (n, "kernel A: residual map")
        assert np.array_equal(d["mbinfo"][:, :25], o["counts"]), (n, "kernel B: token counts")
        assert np.array_equal(d["mbinfo"][:, 25], o["modes"][:, 0] != 4) and np.array_equal(d["mbinfo"][:, 26], o["modes"][:, 18]), n
        assert np.array_equal(d["levels"], o["levels"]), (n, "kernel B: levels")
        assert np.array_equal(d["quant"][:, :6], o["quant"]), (n, "quantisers")
        assert np.array_equal(d["filters"], o["filters"]), (n, "filter parameters")


@pytest.mark.parametrize("crop", [True, False])
@pytest.mark.parametrize("entropy", [1, 0])
def test_the_file_call_against_the_witness(entropy, crop):
    """one mixed call, permuted with a fixed seed: the kernels (1) and the host threads (0) in front of the same pixel stages"""
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
    order = [CNAMES[i] for i in np.random.default_rng(19).permutation(len(CNAMES))]
    infos, images, _, status = ops.webp_decode_files_device([data_of(n) for n in order], strict=False, crop=crop)
    assert 4 * list(status).count(0) >= 3 * len(order)
    for n, img, st in zip(order, images, status):
        assert (st != 0) == refused_by_witness(n), n
        if st:
            assert img is None
            continue
        o, want = witness(n, S.REFERENCE), want_bgra(n)
        if crop:
            want = want[:o["height"], :o["width"]]
        assert img.shape == want.shape, n
        assert np.array_equal(img, want), (n, "first at row, column, channel", np.argwhere(img != want)[0].tolist())


def test_the_planes_against_the_witness():
    """the writer-made border files (every 16x16, chroma and 4x4 predictor on the top row, the left column and the right-most column):
    host parser, residual kernel, then ffhip_vp8_decode_frames' d_y / d_u / d_v in one call.  A failure names plane and macroblock."""
    names = [n for n in CNAMES if n.startswith("wr_border_")]
    assert len(names) == 15
    parsed = [ops.webp_parse(data_of(n)) for n in names]
    p0 = parsed[0]
    c, r = p0["mbcols"], p0["mbrows"]
    assert all((p["mbcols"], p["mbrows"], p["filter_type"]) == (c, r, 0) and np.array_equal(p["quant"], p0["quant"]) for p in parsed)
    assert all(np.array_equal(p["resmap"], np.arange(c * r)) for p in parsed)
    residual = ops.vp8_residual_batch(np.concatenate([p["levels"] for p in parsed]), np.concatenate([p["mbinfo"] for p in parsed]), p0["quant"])
    modes = np.stack([p["modes"] for p in parsed])
    bgra, planes = ops.vp8_decode_frames(c, r, modes, residual.reshape(len(names), c * r, 384), 0, None, planes=True)
    seen = set()
    for i, n in enumerate(names):
        o = witness(n, S.REFERENCE)
        for k, plane, size in zip("yuv", planes, (16, 8, 8)):
            assert np.array_equal(plane[i], o[k]), (n, k, first_macroblock(plane[i], o[k], size, c))
        assert np.array_equal(bgra[i].reshape(16 * r, 16 * c, 4), want_bgra(n)), n
        for mb in range(c * r):
            if mb < c or mb % c in (0, c - 1):
                m = o["modes"][mb]
                seen |= {("y", int(m[0])), ("uv", int(m[1]))} | ({("b", int(v)) for v in m[2:18]} if m[0] == 4 else set())
    assert seen >= {("y", m) for m in range(5)} | {("uv", m) for m in range(4)} | {("b", m) for m in range(10)}
