"""CPU: the host-side parts of test_limits_gpu.py -- its answer keys against the rules they restate, and that they hold what each case is
there for -- and the limits of the argument checks that the GPU cases run at."""
import itertools

import numpy as np
import pytest

import limits as M
from ffpic_amd import capi
from limits import AA, BIL, F16, F32
from test_resize_capi import SIDES
from test_resize_gpu import axis_matrix, resize_rule


@pytest.mark.parametrize("filt", [BIL, AA])
def test_the_sparse_resize_rule_equals_axis_matrix(filt):
    """every output index of every pair of sides both can do: the run's place and every weight"""
    sides = [s for s in SIDES if s <= 1080]
    assert len(sides) == len(SIDES) - 1
    for n_in, n_out in itertools.product(sides, sides):
        W = axis_matrix(n_in, n_out, filt)
        dense = np.zeros_like(W)
        for o, (first, q) in enumerate(M.axis_runs(n_in, n_out, filt)):
            dense[o, first:first + len(q)] = q
        assert np.array_equal(dense, W), (n_in, n_out, filt)


@pytest.mark.parametrize("filt", [BIL, AA])
def test_the_sparse_resize_equals_resize_rule(filt):
    rng = np.random.default_rng(31 + filt)
    for h, w, oh, ow in ((17, 65, 5, 7), (3, 224, 7, 1), (1080, 2, 1, 3), (1, 1, 16, 5), (9, 13, 9, 13)):
        v = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert np.array_equal(M.resize_sparse(v, oh, ow, filt), resize_rule(v, oh, ow, filt)), (h, w, oh, ow)


def test_the_side_cases_reach_what_they_are_there_for():
    for filt in (BIL, AA):
        first, q = M.axis_taps(16384, 16384, filt, 16383)
        assert first == 16383 and list(q) == [4096]
        assert M.axis_taps(16383, 16384, filt, 16383)[0] + len(M.axis_taps(16383, 16384, filt, 16383)[1]) == 16383
        first, q = M.axis_taps(16384, 16383, filt, 16382)
        assert first + len(q) == 16384                                         # the last output's run ends at sample 16383
    first, q = M.axis_taps(16384, 1, AA, 0)
    assert (first, len(q)) == (0, 16384)                                       # four LDS chunks of exactly 4096
    assert len(M.axis_taps(16384, 1, BIL, 0)[1]) == 2


def jpeg_item_code(layout, mcu_cols, mcu_rows, pitch=None):
    """ffhip_jpeg_recon_items' word on one item at made-up addresses: nothing is dereferenced before the device check"""
    ncomp, h, v, _ = M.JPEG_CLASSES[layout]
    it = capi.JpegItem()
    it.geom = capi.jpeg_geom(mcu_cols, mcu_rows, ncomp, h, v)
    it.d_coef_y, it.d_quant, it.d_bgra = 1 << 20, 3 << 20, 4 << 20
    it.d_coef_u, it.d_coef_v = (2 << 20, 2 << 20) if ncomp == 3 else (None, None)
    it.pitch = mcu_cols * 8 * h * 4 if pitch is None else pitch
    return capi.lib().ffhip_jpeg_recon_items((capi.JpegItem * 1)(it), 1, None)


@pytest.mark.parametrize("layout", list(M.JPEG_CLASSES))
def test_the_jpeg_limits_are_where_the_header_and_the_gpu_cases_have_them(layout):
    """One past each limit is FFHIP_EINVAL on any machine.  Without a device the limit itself reaches the device check, and the largest
    mcu_cols the check takes, found by bisection, is 4096 x the class's MCUs per unit"""
    ncomp, h, v, mcus = M.JPEG_CLASSES[layout]
    cols = M.jpeg_max_cols(layout)
    rows = M.JPEG_UNITS_PER_PICTURE // M.JPEG_UNITS_PER_ROW
    assert cols == 4096 * mcus and cols * 8 * h * 4 <= M.JPEG_MAX_PITCH
    assert jpeg_item_code(layout, cols + 1, 1) == capi.FFHIP_EINVAL
    assert jpeg_item_code(layout, cols, rows + 1) == capi.FFHIP_EINVAL
    assert jpeg_item_code(layout, 2, 2, M.JPEG_MAX_PITCH + 16) == capi.FFHIP_EINVAL
    if capi.lib().ffhip_device_count() > 0:
        return                                                  # with a device the admitted items run: test_limits_gpu.py
    lo, hi = 1, 1 << 20                                         # lo is taken, hi refused
    assert jpeg_item_code(layout, lo, 2) == capi.FFHIP_ENODEV and jpeg_item_code(layout, hi, 2) == capi.FFHIP_EINVAL
    while hi - lo > 1:
        mid = (lo + hi) // 2
        code = jpeg_item_code(layout, mid, 2)
        assert code in (capi.FFHIP_ENODEV, capi.FFHIP_EINVAL)
        lo, hi = (mid, hi) if code == capi.FFHIP_ENODEV else (lo, mid)
    assert lo == cols
    assert jpeg_item_code(layout, cols, rows) == capi.FFHIP_ENODEV
    assert jpeg_item_code(layout, 2, 2, M.JPEG_MAX_PITCH) == capi.FFHIP_ENODEV


@pytest.mark.parametrize("dtype,planar", [(F32, 1), (F32, 0), (F16, 1), (F16, 0)])
def test_the_float_keys_hold_inf_subnormals_and_signed_zeros(dtype, planar):
    pic = M.byte_ramps()
    for scale, bias, what in M.FLOAT_EDGES:
        key = M.float_key(pic, dtype, planar, 0, scale, bias)
        assert key.shape == ((3, 2, 256) if planar else (2, 256, 3))
        assert M.float_key_holds(key, what), (scale, bias, what)
    if dtype == F16:
        red = M.float_key(pic, F16, 1, 0, 300.0, 0.0)[0, 0]                     # channel R of row 0: the bytes (k + 74) % 256
        byte = (np.arange(256) + 74) % 256
        assert np.array_equal(np.isposinf(red), byte >= 219)                  # 219 x 300 = 65700 > 65520
        tie = M.float_key(pic, F16, 1, 0, 2.0 ** -25, 0.0)[0, 0].view(np.uint16)
        assert [int(tie[(b - 74) % 256]) for b in (0, 1, 2, 3, 4, 5)] == [0, 0, 1, 2, 2, 2]      # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    else:
        sub = M.float_key(pic, F32, 1, 0, 1e-40, 0.0)[0, 0].view(np.uint32)
        assert int(sub[(1 - 74) % 256]) == int(np.float32(1e-40).view(np.uint32)) < 1 << 23
        both = M.float_key(pic, F32, 1, 0, 1e-38, -1e-38)[0, 0].view(np.uint32)
        assert int(both[(1 - 74) % 256]) & 0x7fffffff < 1 << 23                # 1e-38 - 1e-38: a subnormal difference or zero
