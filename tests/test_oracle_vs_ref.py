"""CPU: the oracle against the reference itself (oracle/_ref/libffpic_ref.so, compiled by oracle/Makefile from the
reference sources) on seeded random inputs -- wider than the other goldens.  Where the compiled reference cannot be had,
the SHA-256 digests of its outputs for these same inputs (and the reference outputs the oracle takes as inputs) come
from tests/golden/ref_outputs.npz (oracle_lib.check_ref / ref_inputs)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from ffpic_amd import synth


def test_idct8x8_and_dequant_random(ffo):
    rng = np.random.default_rng(11)
    blocks = np.concatenate([synth.adversarial_blocks(rng, 2048), synth._blocks(rng, 2048, synth.quant_tables()[0])])
    q = rng.integers(1, 65536, size=64).astype(np.uint16)

    def run(idct_fn, dequant_fn, qtab):
        idct, deq = blocks.copy(), np.zeros_like(blocks)
        for i in range(len(blocks)):
            idct_fn(idct[i])
            dequant_fn(deq[i], blocks[i].copy(), qtab.copy(), 63)
        return idct, deq
    O.check_ref("idct8x8_and_dequant_random", run(ffo.ffo_idct_8x8_16, ffo.ffo_jpeg_dequant, q),
                lambda: run(O.ref().ref_idct_8x8_16, O.ref().ref_jpeg_dequant, q))


def test_vp8_random(ffo):
    rng = np.random.default_rng(12)
    blocks = rng.integers(-32768, 32768, size=(4096, 16)).astype(np.int16)

    def run(idct_fn, iwht_fn):
        idct, wht = blocks.copy(), np.zeros((len(blocks), 256), np.int16)
        for i in range(len(blocks)):
            idct_fn(idct[i])
            iwht_fn(blocks[i].copy(), wht[i])
        return idct, wht
    O.check_ref("vp8_random", run(ffo.ffo_vp8_idct_4x4, ffo.ffo_vp8_iwht_long), lambda: run(O.ref().ref_vp8_idct_4x4, O.ref().ref_vp8_iwht_long))


@pytest.mark.parametrize("regime", ["random", "sparse", "dense"])
def test_vp8_residual_block_driven(ffo, regime):
    """ffo_vp8_residual_mb against vp8_decode_residual_block itself (webp.c:1125-1199) on synthetic streams: the levels,
    non-zero flags and quantisers the reference decoded are the oracle's inputs, the residual it wrote the expected output"""
    key = f"vp8_residual_block_driven_{regime}"
    lv, info, q = O.ref_inputs(key, lambda: O.ref_vp8_driven(400, seed=77, regime=regime)[:3])
    out = np.zeros((lv.shape[0], 384), np.int16)
    for i in range(lv.shape[0]):
        ffo.ffo_vp8_residual_mb(np.ascontiguousarray(lv[i]).reshape(-1), info[i], int(info[i, 25]),
                                np.ascontiguousarray(q[info[i, 26], :6]), out[i])
    O.check_ref(key, out, lambda: O.ref_vp8_driven(400, seed=77, regime=regime)[3])


def test_hevc_random(ffo):
    rng = np.random.default_rng(13)
    blocks = rng.integers(-32768, 32768, size=(1024, 16)).astype(np.int16)
    forms = ((8, 0), (10, 0), (12, 1))

    def run_dst(fn):
        out = np.zeros((len(blocks), len(forms), 16), np.int16)
        for i, b in enumerate(blocks):
            for j, (bd, epp) in enumerate(forms):
                fn(b.copy(), out[i, j], bd, epp)
        return out
    O.check_ref("hevc_random_dst4", run_dst(ffo.ffo_hevc_idct_4x4_dst), lambda: run_dst(lambda b, o, bd, epp: O.ref().idct_4x4_hevc(b, o, bd, bool(epp))))
    for n in (4, 8, 16, 32):
        cases = []
        for _ in range(24):
            lv = rng.integers(-32768, 32768, size=n * n).astype(np.int16) if rng.random() < 0.3 else \
                np.rint(rng.laplace(0, 8, size=n * n)).astype(np.int16)
            cases.append((lv, int(rng.integers(0, 52)), int(rng.choice([8, 10]))))

        def run(scale_fn, transform_fn):
            scaled, res = np.zeros((len(cases), n * n), np.int16), np.zeros((len(cases), n * n), np.int16)
            for k, (lv, qp, bd) in enumerate(cases):
                scale_fn(lv.copy(), scaled[k], n, qp, bd)
                transform_fn(scaled[k].copy(), res[k], n, 0, bd, 0)
            return scaled, res
        O.check_ref(f"hevc_random_scale_transform_{n}",
                    run(lambda lv, d, n, qp, bd: ffo.ffo_hevc_scale(lv, d, n, qp, bd, 0, None), ffo.ffo_hevc_transform),
                    lambda: run(lambda lv, d, n, qp, bd: O.ref().ref_hevc_scale(lv, d, n, qp, bd, 0, None, 0), O.ref().ref_hevc_transform))


def test_hevc_scale_and_transform_every_branch(ffo):
    """ffo_hevc_residual_tu against the reference's scale_and_transform (hevc.c:4172-4251) called as a whole: random
    bypass / transform-skip / rotation flags, scaling lists, bit depths, extended precision, luma and chroma (the qP
    the reference derives in 8.6.1 is handed to the restatement)"""
    rng = np.random.default_rng(0xA12)
    seen = set()
    for n in (4, 8, 16, 32):
        cases = []
        for _ in range(150 if n < 32 else 60):
            lv = rng.integers(-32768, 32768, size=n * n).astype(np.int16) if rng.random() < 0.3 else \
                np.rint(rng.laplace(0, 8, size=n * n)).astype(np.int16)
            bd, epp = int(rng.choice([8, 10, 12])), int(rng.random() < 0.2)
            qp = int(rng.integers(0, 52 + 6 * (bd - 8)))
            cidx, cat = int(rng.integers(0, 3)), int(rng.choice([1, 3]))
            bypass, ts, rot = int(rng.random() < 0.25), int(rng.random() < 0.4), int(rng.random() < 0.5)
            sf = rng.integers(1, 256, size=n * n).astype(np.uint8) if rng.random() < 0.5 else None
            cases.append((lv, bd, epp, qp, cidx, cat, bypass, ts, rot, sf))

        def sfp(sf):
            return None if sf is None else sf.ctypes.data_as(C.c_void_p)

        def ref():
            R = O.ref()
            res, qps = np.zeros((len(cases), n * n), np.int16), np.zeros(len(cases), np.int32)
            for k, (lv, bd, epp, qp, cidx, cat, bypass, ts, rot, sf) in enumerate(cases):
                qps[k] = R.ref_hevc_scale_and_transform(lv.copy(), res[k], n, cidx, qp, bd, epp, bypass, ts, rot, cat, sfp(sf))
            return qps, res
        key = f"hevc_scale_and_transform_every_branch_{n}"
        exp_qp = O.ref_inputs(key + "_qp", lambda: ref()[0])
        got = np.zeros((len(cases), n * n), np.int16)
        for k, (lv, bd, epp, qp, cidx, cat, bypass, ts, rot, sf) in enumerate(cases):
            qP = int(exp_qp[k])
            if cidx == 0:
                assert qP == qp
            flags = (1 if n == 4 and cidx == 0 else 0) | (2 if ts else 0) | (4 if bypass else 0) | (8 if rot and n == 4 else 0)
            ffo.ffo_hevc_residual_tu(lv.copy(), got[k], n, qP, flags, bd, epp, sfp(sf))
            seen.add((bypass, ts, bool(rot and n == 4), sf is not None and n > 4))
        O.check_ref(key, got, lambda: ref()[1])
    assert len(seen) == 12          # rotation exists at 4x4 only, the dropped scaling list above 4x4 only


@pytest.mark.parametrize("nc,h,v", [(3, 2, 2), (3, 1, 1), (3, 2, 1), (3, 1, 2), (1, 1, 1), (3, 4, 1), (3, 1, 4), (3, 3, 1),
                                    (3, 1, 3), (1, 2, 2), (1, 4, 1)])
def test_jpeg_grid_random(nc, h, v):
    q = synth.quant_tables(60)
    g = O.make_geom(9, 5, nc, h, v)
    cy, cu, cv = synth.coef_batch(1, 9, 5, nc, h, v, quant=q, first=100)
    O.check_ref(f"jpeg_grid_random_{nc}{h}{v}", O.oracle_jpeg_recon(g, cy, cu, cv, q)[0], lambda: O.ref_jpeg_recon(g, cy, cu, cv, q))


@pytest.mark.parametrize("seed,bd,bdc,c444", [(21, 8, 8, False), (22, 10, 10, False), (23, 8, 8, True), (24, 12, 9, True)])
def test_hevc_intra_random_tu_lists(seed, bd, bdc, c444):
    """TU lists (not the committed ones) through the reference's own neighbour processing,
    predictors, rdpcm, cross-component prediction and construct_pic vs the restatement"""
    w, h = 128, 128
    tus, res = synth.hevc_intra_tus(w, h, seed, adversarial_masks=True, ccp=c444, chroma_444=c444)
    res = res.copy()
    res[::41] = 32767
    res[5::43] = -32768
    csub = 1 if c444 else 2
    O.check_ref(f"hevc_intra_random_tu_lists_{seed}", O.oracle_hevc_intra(tus, res, w, h, True, bd, bdc, csub=csub),
                lambda: O.ref_hevc_intra(tus, res, w, h, True, bd, bdc, csub=csub))


def test_vp8_filter_params_sweep():
    """f3: ffhip_vp8_filter_params (host C in the product) against the reference's calculate_filter_control_parameter
    (webp.c:1756-1803) over every level x sharpness x filter type, with and without segmentation (both feature modes)
    and loop-filter deltas, for 1, 2 and 4 partitions (the reference derives triples per PARTITION index, webp.c:1905-1915)"""
    from ffpic_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(3)
    cases = [(ft, lvl, sh, 0, 0, (0, 0, 0, 0), 0, 0, 0, 4) for ft in (0, 1) for lvl in range(64) for sh in range(8)]
    for _ in range(3000):
        cases.append((int(rng.integers(0, 2)), int(rng.integers(0, 64)), int(rng.integers(0, 8)), int(rng.integers(0, 2)), int(rng.integers(0, 2)),
                      tuple(int(x) for x in rng.integers(-63, 64, size=4)), int(rng.integers(0, 2)), int(rng.integers(-63, 64)),
                      int(rng.integers(-63, 64)), int(rng.choice([1, 2, 4]))))

    def ref():
        R = O.ref()
        out = np.zeros((len(cases), 24), np.int32)
        for k, (ft, lvl, sh, seg, fmode, lfu, adj, d0, d1, parts) in enumerate(cases):
            R.ref_webp_filter_params(np.array([ft, lvl, sh, seg, fmode, *lfu, adj, d0, d1, parts], np.int32), out[k])
        return out
    seen_types = set()
    got_all = np.zeros((len(cases), 24), np.int32)
    for k, (ft, lvl, sh, seg, fmode, lfu, adj, d0, d1, parts) in enumerate(cases):
        h = capi.Vp8FilterHeader(ft, lvl, sh, seg, fmode, (C.c_int8 * 4)(*lfu), adj, d0, d1, parts)
        got = np.zeros(24, np.uint8)
        ftype = C.c_int(-1)
        assert L.ffhip_vp8_filter_params(C.byref(h), got.ctypes.data, C.byref(ftype)) == 0
        got_all[k] = got
        assert ftype.value == (0 if lvl == 0 else (1 if ft else 2))
        seen_types.add(ftype.value)
    O.check_ref("vp8_filter_params_sweep", got_all, ref)
    assert seen_types == {0, 1, 2}
    bad = capi.Vp8FilterHeader(0, 64, 0, 0, 0, (C.c_int8 * 4)(), 0, 0, 0, 1)
    assert L.ffhip_vp8_filter_params(C.byref(bad), got.ctypes.data, C.byref(ftype)) == capi.FFHIP_EINVAL
    bad = capi.Vp8FilterHeader(0, 10, 0, 0, 0, (C.c_int8 * 4)(), 0, 0, 0, 3)
    assert L.ffhip_vp8_filter_params(C.byref(bad), got.ctypes.data, C.byref(ftype)) == capi.FFHIP_EINVAL
