"""GPU: ffhip_hevc_residual_batch and ffhip_hevc_intra_recon against the spec witness (tests/hevc_spec.py), with no oracle in the
loop.  Everything is exact: the device equals the witness under REFERENCE everywhere, and under SPEC wherever no named
deviation is touched (tests/test_hevc_spec.py holds the witness itself)."""
import numpy as np
import pytest

import hevc_cases as HC
import hevc_spec as S
from ffpic_amd import capi, ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("n", (4, 8, 16, 32))
def test_residual_batch_is_the_witness(n, bd):
    """one call: every single-coefficient block at 1, -1 and the largest in-range level, Laplace levels over qP 0 .. 51, flat
    scaling and lists, every flag"""
    lv, info, sc = HC.residual_batch(n, bd)
    assert {int(f) for f in info[:, 1]} == ({0, 1, 2, 4, 2 | 8, 4 | 8} if n == 4 else {0, 2, 4}) and set(range(52)) <= {int(q) for q in info[:, 0]}
    got = ops.hevc_residual_batch(n, lv, info, bitdepth=bd, scaling=sc).astype(np.int64)
    ref = S.residual(lv, info, n, bd, 0, sc, S.REFERENCE)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert not bad.size, "TU %d of %d (qP %d, flags %d, list %d): not the witness under REFERENCE" % (bad[0], len(lv), *info[bad[0], :3])
    spec = S.residual(lv, info, n, bd, 0, sc, S.SPEC)
    same = (got == spec).all(axis=1)
    touched = HC.residual_touched(info, n)
    keep = HC.residual_conformant(lv, info, n, bd, sc) & ~touched
    assert keep.mean() >= 0.6                                    # (the 4x4 batch holds every single-coefficient block through the DST too)
    bad = np.nonzero(keep & ~same)[0]
    assert not bad.size, "TU %d (qP %d, flags %d, list %d): conformant and untouched, yet not the standard's residual" % (bad[0], *info[bad[0], :3])
    # where a named rule says the residual differs it does: a transform-skipped block with a coefficient, most DST blocks
    conf = HC.residual_conformant(lv, info, n, bd, sc)
    ts = touched & ((info[:, 1] & 2) != 0) & conf & (np.abs(got).max(axis=1) > 0)
    assert ts.sum() >= 5 and not same[ts].any(), np.nonzero(ts & same)[0][:4]
    if n == 4:
        dst = touched & ((info[:, 1] & 2) == 0) & (np.abs(lv).max(axis=1) > 1)
        assert dst.sum() > 20 and (~same[dst]).mean() > 0.5


def _check_planes(tus, got, ref, what):
    bad = np.nonzero(HC.tu_differs(tus, got, ref))[0]
    assert not bad.size, "%s: %s" % (what, HC.describe(tus, bad[0]))
    for g, r in zip(got, ref):                                   # and nothing outside the TUs
        assert g is None or np.array_equal(g, r), what


def _cells(n, bd, pattern):
    tus, res, w, h, under_test = HC.intra_cells(n, bd, pattern)
    t = tus[under_test]
    assert len(t) == 70 and set(t["pred_mode"].tolist()) == set(range(35)) and len(tus) == 420
    got = ops.hevc_intra_recon(tus, res, w, h, False, bd, bd)
    what = f"{n}x{n}, {bd} bits, {pattern}"
    _check_planes(tus, got[:1], S.intra(tus, res, w, h, False, bd, bd, 2, S.REFERENCE)[:1], what + ", REFERENCE")
    assert not HC.intra_touched(tus).any()                       # no cell holds rdpcm or cross-component prediction: SPEC is the same picture
    _check_planes(tus, got[:1], S.intra(tus, res, w, h, False, bd, bd, 2, S.SPEC)[:1], what + ", SPEC")


@pytest.mark.parametrize("pattern", HC.PATTERNS)
@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("n", (4, 8, 16, 32))
def test_intra_cells_are_the_witness(n, bd, pattern):
    """per size one picture of 70 cells -- 35 modes, with and without TU_FILTER | TU_STRONG -- and one call per availability pattern"""
    _cells(n, bd, pattern)


@pytest.mark.parametrize("pattern", ("everything", "no above-right"))
@pytest.mark.parametrize("n", (4, 8, 16, 32))
def test_intra_cells_are_the_witness_levels_form(n, pattern, monkeypatch):
    monkeypatch.setenv("FFHIP_HEVC_INTRA_MODE", "levels"); capi.reload_env()
    _cells(n, 8 if n != 16 else 10, pattern)


@pytest.mark.parametrize("name", list(HC.WHOLE_LISTS))
def test_whole_lists_with_the_real_chain(name):
    """levels -> ffhip_hevc_residual_batch -> ffhip_hevc_intra_recon against levels -> witness residual -> witness intra.
    Under REFERENCE every TU agrees.  Under SPEC the witness takes each TU's neighbours from the device's picture, so that every
    TU no named rule touches -- no DST or transform-skip residual, no horizontal rdpcm, no cross-component prediction -- must agree
    on its own"""
    bd = 8
    tus, w, h, csub, by_size = HC.whole_list(name, bd)
    dev_blocks, ref_blocks, spec_blocks = {}, {}, {}
    direct = HC.intra_touched(tus)
    for n, (idx, lv, info) in by_size.items():
        dev_blocks[n] = ops.hevc_residual_batch(n, lv, info, bitdepth=bd).astype(np.int64)
        ref_blocks[n] = S.residual(lv, info, n, bd, 0, None, S.REFERENCE)
        spec_blocks[n] = S.residual(lv, info, n, bd, 0, None, S.SPEC)
        bad = np.nonzero((dev_blocks[n] != ref_blocks[n]).any(axis=1))[0]
        assert not bad.size, "residual of " + HC.describe(tus, idx[bad[0]])
        assert HC.residual_conformant(lv, info, n, bd).all(), n
        differs = (spec_blocks[n] != ref_blocks[n]).any(axis=1)
        assert not (differs & ~HC.residual_touched(info, n)).any()
        direct[idx[differs]] = True
    flat = HC.scatter_residual(tus, by_size, dev_blocks)
    assert np.abs(flat).max() <= 32767
    got = ops.hevc_intra_recon(tus, flat.astype(np.int16), w, h, True, bd, bd, csub=csub)
    _check_planes(tus, got, S.intra(tus, HC.scatter_residual(tus, by_size, ref_blocks), w, h, True, bd, bd, csub, S.REFERENCE), name + ", REFERENCE")
    spec = S.intra(tus, HC.scatter_residual(tus, by_size, spec_blocks), w, h, True, bd, bd, csub, S.SPEC, forced=got)
    assert (~direct).sum() > len(tus) // 3
    bad = np.nonzero(HC.tu_differs(tus, got, spec) & ~direct)[0]
    assert not bad.size, "%s, SPEC: %s" % (name, HC.describe(tus, bad[0]))
    assert (HC.tu_differs(tus, got, spec) & direct).any()        # and the named rules do move this picture
