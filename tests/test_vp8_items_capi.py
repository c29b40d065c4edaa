"""CPU: the argument checks of ffhip_vp8_decode_items (key frames of mixed sizes, quantisers and loop filters in one call).
Every refusal is FFHIP_EINVAL whether or not a device is present; good arguments reach the device check (FFHIP_ENODEV here)."""
import ctypes as C

import numpy as np
import pytest

from ffpic_amd import capi, synth

A = 1 << 20     # fake, 16-byte-aligned "device" addresses: nothing is dereferenced before the device check


@pytest.fixture(scope="module")
def L():
    return capi.lib()


@pytest.fixture
def no_gpu(L):
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present; covered by the -m gpu tests")
    return L


_keep = []      # host mode copies the items point at


def item(c=5, r=3, levels=True, residual=None, modes=A, bgra=A + (1 << 16), pitch=None, ft=2, resmap=None, h_modes=True,
         mbinfo=A + 8192, lv=A + 4096):
    it = capi.Vp8Item()
    it.mbcols, it.mbrows = c, r
    if h_modes is True:
        m = synth.vp8_modes(c, r, seed=c * 7 + r)
        _keep.append(m)
        it.h_modes = m.ctypes.data
    elif h_modes is not None:
        _keep.append(h_modes)
        it.h_modes = h_modes.ctypes.data
    it.d_modes = modes
    if levels:
        it.d_levels, it.d_mbinfo = lv, mbinfo
    it.d_residual = residual
    it.d_resmap = resmap
    it.filter_type = ft
    it.d_bgra = bgra
    it.pitch = 64 * c if pitch is None else pitch
    return it


def call(L, items, n=None):
    arr = (capi.Vp8Item * max(len(items), 1))(*items)
    return L.ffhip_vp8_decode_items(arr, len(items) if n is None else n, None)


GOOD = [dict(), dict(levels=False, residual=A + 4096), dict(ft=0), dict(ft=1), dict(c=1, r=1), dict(c=240, r=2), dict(c=2, r=68),
        dict(resmap=A + 12288), dict(h_modes=None), dict(pitch=64 * 5 + 1024), dict(c=120, r=68)]


@pytest.mark.parametrize("kw", GOOD)
def test_valid_items_reach_the_device_check(no_gpu, kw):
    assert call(no_gpu, [item(**kw)]) == capi.FFHIP_ENODEV


def test_mixed_items_reach_the_device_check(no_gpu):
    assert call(no_gpu, [item(**kw) for kw in GOOD]) == capi.FFHIP_ENODEV


def test_empty_call_is_a_no_op(L):
    assert call(L, [], n=0) == 0
    assert L.ffhip_vp8_decode_items(None, 0, None) == 0


def _bad_modes():
    m = synth.vp8_modes(5, 3, seed=1)
    m[7, 0] = 4
    m[7, 9] = 10            # a B_PRED sub-block mode above 9
    return m


BAD = {
    "both residual forms": dict(residual=A + 4096),
    "neither residual form": dict(levels=False),
    "levels without mbinfo": dict(mbinfo=None),
    "filter type 3": dict(ft=3),
    "filter type -1": dict(ft=-1),
    "levels misaligned": dict(lv=A + 4104),
    "mbinfo misaligned": dict(mbinfo=A + 8194),
    "residual misaligned": dict(levels=False, residual=A + 4098),
    "modes misaligned": dict(modes=A + 2),
    "modes NULL": dict(modes=None),
    "resmap misaligned": dict(resmap=A + 12290),
    "output misaligned": dict(bgra=A + (1 << 16) + 8),
    "output NULL": dict(bgra=None),
    "pitch below 64 x mbcols": dict(pitch=64 * 5 - 16),
    "pitch not a multiple of 16": dict(pitch=64 * 5 + 4),
    "pitch x 16 x mbrows reaches 2^31": dict(pitch=1 << 23, r=16, h_modes=None),
    "pitch near 2^59 (the product with 16 x mbrows wraps)": dict(pitch=(1 << 59) + 16, r=32, h_modes=None),
    "pitch above 2^31": dict(pitch=1 << 32, r=1, h_modes=None),
    "zero columns": dict(c=0, h_modes=None),
    "zero rows": dict(r=0, h_modes=None),
    "2^23 macroblocks in one frame": dict(c=2048, r=4096, pitch=2048 * 64, h_modes=None),
    "host mode record out of range": dict(h_modes=_bad_modes()),
}


@pytest.mark.parametrize("why", list(BAD))
def test_refusals(L, why):
    assert call(L, [item(**BAD[why])]) == capi.FFHIP_EINVAL, why
    # one bad item refuses the whole call, wherever it stands
    assert call(L, [item(), item(ft=0, levels=False, residual=A), item(**BAD[why])]) == capi.FFHIP_EINVAL, why


def test_host_mode_byte_checks(L):
    for rec, val in ((0, 5), (1, 4)):          # y mode above 4, uv mode above 3
        m = synth.vp8_modes(5, 3, seed=2)
        m[3, rec] = val
        assert call(L, [item(h_modes=m)]) == capi.FFHIP_EINVAL


def test_total_macroblocks_over_the_limit(L):
    # 1 024 items of 2^20 macroblocks are 2^30 in all: refused before anything else happens
    big = [item(c=1024, r=1024, pitch=1024 * 64, h_modes=None) for _ in range(1024)]
    assert call(L, big) == capi.FFHIP_EINVAL


def test_negative_count(L):
    assert call(L, [item()], n=-1) == capi.FFHIP_EINVAL
    assert L.ffhip_vp8_decode_items(None, 1, None) == capi.FFHIP_EINVAL


def test_struct_layout_matches_the_header():
    assert C.sizeof(capi.Vp8Item) == 168
    assert capi.Vp8Item.quant.offset == 40 and capi.Vp8Item.filters.offset == 124 and capi.Vp8Item.pitch.offset == 160
    np.testing.assert_equal(capi.Vp8Item.filter_type.offset, 120)
