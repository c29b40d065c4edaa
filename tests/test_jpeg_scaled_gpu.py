"""GPU: reduced-size JPEG decode.  ffhip_jpeg_recon_items_scaled byte for byte against the rule written in numpy (tests/jpeg_scaled_rule.py)
with every byte around the pictures checked untouched; denominator 1 against ffhip_jpeg_recon_items; files written from known coefficients
through ffhip_jpeg_decode_files_mixed_device_scaled, behind the device entropy decoder and behind the host threads; the torch layer's
reduce= against numpy rule -> crop or resize -> the tensor stage's formula.  No tolerance anywhere."""
import numpy as np
import pytest

import jpeg_cases
import jpeg_scaled_rule as R
import oracle_lib as O
from ffpic_amd import capi, ops, synth, tensors
from test_jpeg_mixed_gpu import LAYOUTS, _upload, _writer_file, build_items
from test_tensor_gpu import MEAN, STD, expected

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture
def entropy_env(monkeypatch):
    """FFHIP_JPEG_GPU_ENTROPY for the test, read again by the library; undone (and read again) afterwards"""
    def set_(value):
        if value is None:
            monkeypatch.delenv("FFHIP_JPEG_GPU_ENTROPY", raising=False)
        else:
            monkeypatch.setenv("FFHIP_JPEG_GPU_ENTROPY", value)
        capi.reload_env()
    yield set_
    monkeypatch.undo()
    capi.reload_env()


def dense_planes(rng, geom):
    """dense random coefficients within the baseline range, every one of the 64 set"""
    mk = lambda n: rng.integers(-1024, 1024, n * 64).astype(np.int16)
    cy = mk(geom.y_blocks)
    return (cy, mk(geom.c_blocks), mk(geom.c_blocks)) if geom.ncomp == 3 else (cy, None, None)


# ---------------------------------------------------------------------------------------------------- 1. the items call
def test_every_class_and_denominator_in_one_call_equals_the_rule():
    L = capi.require_device()
    rng = np.random.default_rng(400)
    q = synth.quant_tables()
    wg = L.ffhip_jpeg_scaled_wg_blocks()                    # luma blocks side by side a workgroup covers
    specs = []
    for k, lay in enumerate(LAYOUTS):
        for j, d in enumerate((2, 4, 8)):
            specs.append((lay, (1, 1) if (k + j) % 2 else (3, 2), d))
            specs.append((lay, (3, 2) if (k + j) % 2 else (1, 1), d))
    for lay, d in (("420", 2), ("444", 4), ("h4v1", 8), ("grey", 8), ("422", 2), ("h1v4", 4)):       # one MCU wider than a workgroup covers
        specs.append((lay, (wg // LAYOUTS[lay][1] + 1, 2), d))
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    places, total = [], 0
    for lay, (mc, mr), d in specs:
        ncomp, h, v = LAYOUTS[lay]
        n = 8 // d
        w, hh = n * h * mc, n * v * mr
        pitch = (4 * w + 15) // 16 * 16 + 64               # 64 bytes of padding a row
        total += 2 * pitch + 16 * int(rng.integers(0, 4))  # guard rows in front (and behind the last picture)
        total = (total + 15) // 16 * 16
        places.append((total, pitch, w, hh))
        total += pitch * hh
    total += 2 * 4096
    exp = np.full(total, FILL, np.uint8)
    dout, dq, keep, items = _upload(exp), _upload(q), [], []
    for (lay, (mc, mr), d), (off, pitch, w, hh) in zip(specs, places):
        ncomp, h, v = LAYOUTS[lay]
        geom = capi.jpeg_geom(mc, mr, ncomp, h, v)
        cy, cu, cv = dense_planes(rng, geom)
        bufs = [_upload(c) if c is not None else None for c in (cy, cu, cv)]
        keep += bufs
        it = capi.JpegItem()
        it.geom = geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [b.ptr if b else None for b in bufs]
        it.d_quant, it.d_bgra, it.pitch = dq.ptr, dout.ptr + off, pitch
        items.append(it)
        view = np.lib.stride_tricks.as_strided(exp[off:], (hh, w, 4), (pitch, 4, 1))
        view[...] = R.picture(mc, mr, ncomp, h, v, cy, cu, cv, q, d)
    ops.jpeg_recon_items_scaled(items, [d for _, _, d in specs])
    capi.sync(None)
    got = dout.to_host((total,), np.uint8)
    for k, ((lay, size, d), (off, pitch, w, hh)) in enumerate(zip(specs, places)):
        a = np.lib.stride_tricks.as_strided(got[off:], (hh, w, 4), (pitch, 4, 1))
        b = np.lib.stride_tricks.as_strided(exp[off:], (hh, w, 4), (pitch, 4, 1))
        assert np.array_equal(a, b), (k, lay, size, d)
    assert np.array_equal(got, exp), "bytes outside the pictures were written: row padding, guard rows or the space between"


def test_denominator_one_is_the_full_size_call():
    L = capi.require_device()
    q = synth.quant_tables()
    specs = [("420", 7, 3), ("444", 1, 1), ("422", 9, 2), ("440", 3, 5), ("h4v1", 5, 2), ("h1v4", 2, 2), ("grey", 17, 3), ("420", 40, 2)]
    outs = []
    for scaled in (False, True):
        items, places, dout, total, keep = build_items(L, specs, np.random.default_rng(410), q)
        if scaled:
            ops.jpeg_recon_items_scaled(items, [1] * len(items))
        else:
            ops.jpeg_recon_items(items)
        capi.sync(None)
        outs.append(dout.to_host((total,), np.uint8))
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------- 2. files from known coefficients
def known_files():
    """(case, denominator): 4:2:0, 4:4:4, 4:2:2, grey and the h * v = 4 layouts, with and without restart markers, sizes that do not fill the
    last MCU, every denominator beside every other"""
    c, s = jpeg_cases.case, jpeg_cases.small
    return [(c("420_1_dense"), 2), (s("444", "annexk", 0), 4), (c("422_3x2_laplace_row"), 8), (s("grey", "annexk", 2), 2),
            (c("h1v4_3x2_mixed_long"), 4), (s("420", "long", 2, 3, 1), 8), (s("444", "deep", 2), 2), (c("grey_3x2_dense_ids23_r5"), 8),
            (s("422", "annexk", 0), 4), (c("420_3x2_mixed_deep23_r1"), 1), (c("h4v1_3x2_ones_r1"), 2), (s("420", "annexk", 0), 4),
            (c("420_dense"), 8), (c("422_mixed_row"), 2), (s("440", "shared", 0), 8)]


def expect_file(case, geom, d):
    f = case.facts
    cy, cu, cv = case.coef
    if d == 1:
        return O.oracle_jpeg_recon(O.make_geom(f["mcu_cols"], f["mcu_rows"], f["ncomp"], f["h"], f["v"], tuple(geom.qt_id)), cy, cu, cv, case.quant)[0]
    return R.picture(f["mcu_cols"], f["mcu_rows"], f["ncomp"], f["h"], f["v"], cy, cu, cv, case.quant, d, tuple(geom.qt_id))


@pytest.mark.parametrize("device_entropy", [None, "1", "0"])
def test_files_at_mixed_denominators_equal_the_rule_on_their_coefficients(entropy_env, device_entropy):
    """"0" keeps every file on the host threads: the reconstruction behind their upload; "1" the one behind the device decoder's parts"""
    entropy_env(device_entropy)
    known = known_files()
    files = [c.data for c, _ in known]
    denoms = [d for _, d in known]
    bad = len(files) // 2
    files.insert(bad, known[3][0].data[:len(known[3][0].data) // 2])          # a damaged file in the middle
    denoms.insert(bad, 4)
    geoms, images, _, status = ops.jpeg_decode_files_mixed_device_scaled(files, denoms, n_threads=4, strict=False)
    assert status[bad] != 0 and images[bad] is None
    good = [i for i in range(len(files)) if i != bad]
    for i, (case, d) in zip(good, known):
        assert status[i] == 0, (i, status[i])
        exp = expect_file(case, geoms[i], d)
        assert images[i].shape == exp.shape, (i, case.facts["name"], d)
        assert np.array_equal(images[i], exp), (i, case.facts["name"], d)


# ---------------------------------------------------------------------------------------------------- 3. the torch layer
def taps_matrix(n_in, n_out):
    first, taps = tensors.axis_taps(n_in, n_out, antialias=True)
    W = np.zeros((n_out, n_in), np.int64)
    for o in range(n_out):
        W[o, first[o]:first[o] + len(taps[o])] = taps[o]
    return W


def resize_by_taps(v, oh, ow):
    """[h][w][4] uint8 -> [oh][ow][4]: (sum_y sum_x qy qx v + 2^23) >> 24 with the library's host-side taps"""
    acc = np.einsum("oy,yxc,px->opc", taps_matrix(v.shape[0], oh), v.astype(np.int64), taps_matrix(v.shape[1], ow))
    return ((acc + (1 << 23)) >> 24).astype(np.uint8)


@pytest.fixture(scope="module")
def written():
    """files of three sizes and four layouts with the planes they were written from, and their pictures by the numpy rule at every denominator"""
    rng = np.random.default_rng(420)
    out = []
    for w, h, lay, restart in [(300, 200, "420", 0), (100, 70, "444", 3), (43, 33, "422", 0), (131, 77, "grey", 2), (20, 19, "420", 0)]:
        data, coef = _writer_file(rng, w, h, lay, restart=restart)
        out.append((data, coef, w, h, lay))
    return out


def rule_picture(entry, d):
    data, coef, w, h, lay = entry
    ncomp, hh, vv = LAYOUTS[lay]
    mc, mr = -(-w // (8 * hh)), -(-h // (8 * vv))
    cy, cu, cv = [c.reshape(-1) if c is not None else None for c in coef]
    if d == 1:
        return O.oracle_jpeg_recon(O.make_geom(mc, mr, ncomp, hh, vv), np.ascontiguousarray(cy), cu, cv, synth.quant_tables())[0]
    return R.picture(mc, mr, ncomp, hh, vv, cy, cu, cv, synth.quant_tables(), d)


@pytest.mark.parametrize("kw", [dict(dtype="uint8", layout="CHW"), dict(dtype="float16", layout="HWC", mean=MEAN, std=STD)])
def test_reduce_without_size_has_the_mapped_shape(written, kw):
    import torch
    capi.require_device()
    files = [e[0] for e in written]
    f = tensors.tensor_format(kw["dtype"], kw["layout"], "RGB", kw.get("mean"), kw.get("std"))
    for rois in (None, [(3, 5, e[2] - 4, e[3] - 7) for e in written]):               # the whole picture; rectangles not aligned to 4
        got = tensors.decode_jpeg_to_tensors(files, roi=rois, reduce=4, **kw)
        for i, e in enumerate(written):
            x0, y0, w, h = R.mapped_rect(e[2], e[3], 4, rois[i] if rois else (0, 0, e[2], e[3]))
            exp = expected(rule_picture(e, 4)[y0:y0 + h, x0:x0 + w], f)
            assert tuple(got[i].shape) == exp.shape, i
            assert got[i].dtype == getattr(torch, kw["dtype"])
            assert np.array_equal(got[i].cpu().numpy().view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)), i


def test_auto_chooses_per_file_and_equals_rule_resize_sink(written):
    capi.require_device()
    files = [e[0] for e in written]
    f = tensors.tensor_format("uint8", "CHW")
    for rois in (None, [(1, 2, e[2] - 3, e[3] - 2) for e in written]):
        batch, used = tensors.decode_jpeg_to_tensors(files, roi=rois, reduce="auto", size=(16, 16), stack=True, return_reduce=True)
        rects = rois or [(0, 0, e[2], e[3]) for e in written]
        assert used == [ops.jpeg_scale_choose(r[2], r[3], 16, 16) for r in rects]
        assert used == [R.choose(r[2], r[3], 16, 16) for r in rects]
        if rois is None:
            assert used == [8, 4, 2, 4, 1]                                           # the three sizes take three denominators, and the small one none
        assert tuple(batch.shape) == (len(files), 3, 16, 16)
        for i, (e, d) in enumerate(zip(written, used)):
            x0, y0, w, h = R.mapped_rect(e[2], e[3], d, rects[i])
            exp = expected(resize_by_taps(rule_picture(e, d)[y0:y0 + h, x0:x0 + w], 16, 16), f)
            assert np.array_equal(batch[i].cpu().numpy(), exp), (i, d)


def test_reduce_one_is_the_call_without_the_argument(written):
    capi.require_device()
    files = [e[0] for e in written]
    for kw in (dict(), dict(size=(24, 20), stack=True), dict(roi=(2, 1, 15, 17), dtype="float32", layout="HWC", mean=MEAN, std=STD)):
        a = tensors.decode_jpeg_to_tensors(files, **kw)
        b = tensors.decode_jpeg_to_tensors(files, reduce=1, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())


def test_reduce_with_size_and_parts(written):
    """reduce=2 with a size, the batch cut into many parts by the budget switch: the parts are sized by the SCALED pictures"""
    capi.require_device()
    files = [e[0] for e in written] * 3
    f = tensors.tensor_format("uint8", "CHW")
    one = tensors.decode_jpeg_to_tensors(files, reduce=2, size=(12, 14), stack=True)
    assert ops.tensor_last_parts() == 1
    capi.setenv("FFHIP_TENSOR_PART_BYTES", 70000)                                      # 300 x 200 at 1/2 is 152 x 104 coded: 63 232 bytes
    try:
        many = tensors.decode_jpeg_to_tensors(files, reduce=2, size=(12, 14), stack=True)
        parts = ops.tensor_last_parts()
    finally:
        capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    assert 3 <= parts < len(files)
    assert np.array_equal(one.cpu().numpy(), many.cpu().numpy())
    for i, e in enumerate(written):
        w, h = R.scaled_len(e[2], 2), R.scaled_len(e[3], 2)
        assert np.array_equal(one[i].cpu().numpy(), expected(resize_by_taps(rule_picture(e, 2)[:h, :w], 12, 14), f)), i
