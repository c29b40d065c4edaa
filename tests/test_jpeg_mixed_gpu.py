"""GPU: mixed batches -- pictures of different sizes and layouts in one call.  ffhip_jpeg_decode_files_mixed_device against the
reference's whole-file decode and against ffhip_jpeg_decode_files_device on each file alone; ffhip_jpeg_recon_items against
ffhip_jpeg_recon_batch with n = 1 and the oracle, with every byte outside the items' pictures checked untouched."""
import ctypes as C
import io
import os
import threading

import numpy as np
import pytest

import jpeg_writer
import oracle_lib as O
from ffpic_amd import capi, ops, synth
from test_huff_gpu import _equals_reference_decode
from test_oracle_golden import FILES

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

LAYOUTS = {"420": (3, 2, 2), "444": (3, 1, 1), "422": (3, 2, 1), "440": (3, 1, 2), "h4v1": (3, 4, 1), "h1v4": (3, 1, 4), "grey": (1, 1, 1)}


@pytest.fixture
def entropy_env(monkeypatch):
    def set_(value):
        if value is None:
            monkeypatch.delenv("FFHIP_JPEG_GPU_ENTROPY", raising=False)
        else:
            monkeypatch.setenv("FFHIP_JPEG_GPU_ENTROPY", value)
        capi.reload_env()
    yield set_
    monkeypatch.undo()
    capi.reload_env()


def _alone(data):
    """the picture as ffhip_jpeg_decode_files_device decodes the file alone, cropped to its display size"""
    g, w, h = ops.jpeg_probe(data)
    return ops.jpeg_decode_files_device([data], n_threads=2)[1][0][:h, :w]


def _writer_file(rng, w, h, layout, restart=0, q=None):
    """-> (the file's bytes, the coefficient planes it was written from)"""
    ncomp, hh, vv = LAYOUTS[layout]
    mc, mr = -(-w // (8 * hh)), -(-h // (8 * vv))
    quant = synth.quant_tables() if q is None else q
    coef = [synth._blocks(rng, mc * mr * hh * vv, quant[0])]
    if ncomp == 3:
        coef += [synth._blocks(rng, mc * mr, quant[1]), synth._blocks(rng, mc * mr, quant[1])]
    else:
        coef += [None, None]
    return jpeg_writer.encode(w, h, hh, vv, coef, quant, restart=restart), coef


def _pil_file(rng, w, h, sub=2, mode="RGB", q=85):
    PIL = pytest.importorskip("PIL.Image")
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 9.0), 128 + 90 * np.cos(yy / 7.0), (xx * 3 + yy * 5) % 256], axis=2)
    img = np.clip(img + rng.normal(0, 20, img.shape), 0, 255).astype(np.uint8)
    bio = io.BytesIO()
    kw = dict(quality=q)
    if mode == "RGB":
        kw["subsampling"] = sub
    PIL.fromarray(img).convert(mode).save(bio, "JPEG", **kw)
    return bio.getvalue()


# ---------------------------------------------------------------------------------------------------- 1. the fixture files
@pytest.mark.parametrize("device_entropy", [None, "1", "0"])
def test_all_fixture_files_in_one_call_equal_the_reference_decode(golden, entropy_env, device_entropy):
    entropy_env(device_entropy)
    g = golden("jpeg_files.npz")
    tags = list(FILES) * 2 + list(FILES)[:3]
    rng = np.random.default_rng(7)
    rng.shuffle(tags)
    data = [open(os.path.join(GOLDEN, FILES[t]), "rb").read() for t in tags]
    geoms, images, _ = ops.jpeg_decode_files_mixed_device(data, n_threads=4, crop=False)
    for t, geom, img in zip(tags, geoms, images):
        assert img.shape == (geom.height, geom.width, 4)
        _equals_reference_decode(g, t, geom, img)


# ---------------------------------------------------------------------------------------------------- 2. seeded random batches
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_mixed_batches_equal_single_file_decodes(entropy_env, seed):
    """every picture of the batch equals the same file decoded alone -- and, for the files written here, the oracle's reconstruction of the coefficients
    they were written from (the library against the answer, not only against itself)"""
    entropy_env(None)
    rng = np.random.default_rng(100 + seed)
    files, written = [], []
    for k in range(18):
        layout = list(LAYOUTS)[k % len(LAYOUTS)]
        w, h = int(rng.integers(1, 300)), int(rng.integers(1, 200))
        if k % 6 == 1:
            w, h = int(rng.integers(1, 9)), int(rng.integers(1, 9))           # one MCU
        if k % 6 == 2:
            w = 8 * LAYOUTS[layout][1]                                        # one strip wide
        written.append(_writer_file(rng, w, h, layout, restart=int(rng.integers(0, 3)) * int(rng.integers(1, 7))))
    written.append(_writer_file(rng, 4200, 24, "444", restart=0))            # wider than 4 096
    written.append(_writer_file(rng, 4104, 17, "420", restart=5))
    files = [d for d, _ in written]
    coefs = [c for _, c in written]
    files.append(_pil_file(rng, 333, 211, sub=2))
    files.append(_pil_file(rng, 127, 65, sub=0))
    files.append(_pil_file(rng, 250, 99, sub=1))
    files.append(_pil_file(rng, 97, 203, mode="L"))
    coefs += [None] * 4
    order = rng.permutation(len(files))
    files = [files[i] for i in order]
    coefs = [coefs[i] for i in order]
    geoms, images, _ = ops.jpeg_decode_files_mixed_device(files, n_threads=4)
    q = synth.quant_tables()
    for d, img, coef, g in zip(files, images, coefs, geoms):
        assert np.array_equal(img, _alone(d))
        if coef is not None:
            cy, cu, cv = [np.ascontiguousarray(c.reshape(-1)) if c is not None else None for c in coef]
            exp = O.oracle_jpeg_recon(O.make_geom(g.mcu_cols, g.mcu_rows, g.ncomp, g.h, g.v), cy, cu, cv, q)[0]
            assert np.array_equal(img, exp[:img.shape[0], :img.shape[1]])


# ---------------------------------------------------------------------------------------------------- 3. items on synthetic planes
def _upload(a):
    return ops.DeviceBuffer(host=np.ascontiguousarray(a))


def build_items(L, specs, rng, q, adversarial=True):
    """the pictures of specs = [(layout, mcu_cols, mcu_rows)] as items of one call: synthetic planes of their own, one quantiser set, and ONE output
    allocation filled with 0xA5 that holds every picture at an arbitrary 16-byte offset, with the reference's pitch, a ragged one or the recommended
    one in turn.  Returns (items, places, dout, total, keep): places[k] = (geom, offset, pitch, (cy, cu, cv)); keep holds the device planes alive"""
    keep, items, places = [], [], []
    total = 0
    for k, (lay, mc, mr) in enumerate(specs):
        ncomp, h, v = LAYOUTS[lay]
        geom = capi.jpeg_geom(mc, mr, ncomp, h, v)
        if adversarial and k % 3 == 2:      # full-range adversarial levels
            cy = synth.adversarial_blocks(rng, geom.y_blocks).reshape(-1)
            cu = synth.adversarial_blocks(rng, geom.c_blocks).reshape(-1) if ncomp == 3 else None
            cv = synth.adversarial_blocks(rng, geom.c_blocks).reshape(-1) if ncomp == 3 else None
        else:
            cy, cu, cv = synth.coef_batch(1, mc, mr, ncomp, h, v, first=k)
        pitch = [geom.width * 4, geom.width * 4 + 16 * int(rng.integers(1, 9)), None][k % 3]
        if pitch is None:
            lp, _ = C.c_int64(), C.c_int64()
            capi.check(L.ffhip_bgra_layout(C.byref(geom), C.byref(lp), C.byref(_)))
            pitch = lp.value
        total += 16 * int(rng.integers(0, 5))                                 # arbitrary 16-byte offsets
        places.append((geom, total, pitch, (cy, cu, cv)))
        total += pitch * geom.height
    total += 64
    sentinel = np.full(total, 0xA5, np.uint8)
    dout = _upload(sentinel)
    dq = _upload(q)
    keep.append(dq)
    for geom, off, pitch, (cy, cu, cv) in places:
        by, bu, bv = _upload(cy), _upload(cu) if cu is not None else None, _upload(cv) if cv is not None else None
        keep += [by, bu, bv]
        it = capi.JpegItem()
        it.geom = geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v = by.ptr, bu.ptr if bu else None, bv.ptr if bv else None
        it.d_quant, it.d_bgra, it.pitch = dq.ptr, dout.ptr + off, pitch
        items.append(it)
    return items, places, dout, total, keep


def test_recon_items_share_one_allocation_and_touch_nothing_else():
    L = capi.require_device()
    rng = np.random.default_rng(5)
    q = synth.quant_tables()
    specs = [("420", 7, 3), ("444", 1, 1), ("422", 9, 2), ("440", 3, 5), ("h4v1", 5, 2), ("h1v4", 2, 2), ("grey", 17, 3),
             ("420", 1, 1), ("420", 40, 2), ("444", 33, 1), ("grey", 1, 4), ("422", 4, 1), ("420", 5, 4)]
    items, places, dout, total, keep = build_items(L, specs, rng, q)
    ops.jpeg_recon_items(items)
    capi.check(L.ffhip_stream_sync(None))
    got = dout.to_host((total,), np.uint8)
    touched = np.zeros(total, bool)
    for k, (it, (geom, off, pitch, (cy, cu, cv))) in enumerate(zip(items, places)):
        W, H = geom.width, geom.height
        rows = np.lib.stride_tricks.as_strided(got[off:], shape=(H, W * 4), strides=(pitch, 1))
        for r in range(H):
            touched[off + r * pitch: off + r * pitch + W * 4] = True
        # the same picture by ffhip_jpeg_recon_batch, n = 1
        one = ops.DeviceBuffer(nbytes=pitch * H)
        ops.jpeg_recon_batch(geom, 1, it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, 0, one.ptr, pitch, pitch * H)
        capi.check(L.ffhip_stream_sync(None))
        ref = one.to_host((H, pitch), np.uint8)[:, :W * 4]
        assert np.array_equal(rows, ref), k
        if k % 4 == 0:
            exp = O.oracle_jpeg_recon(O.make_geom(geom.mcu_cols, geom.mcu_rows, geom.ncomp, geom.h, geom.v), cy, cu, cv, q, n_images=1)
            assert np.array_equal(rows.reshape(H, W, 4), exp.reshape(H, W, 4)), k
    assert np.all(got[~touched] == 0xA5), "bytes outside the items' pictures were written"


# ---------------------------------------------------------------------------------------------------- 4. a bad file in the middle
@pytest.mark.parametrize("bad", ["truncated", "progressive", "h3v1"])
def test_bad_file_in_the_middle_fails_alone(entropy_env, bad):
    entropy_env(None)
    rng = np.random.default_rng(11)
    good = [_writer_file(rng, 120, 72, "420", restart=3)[0], _pil_file(rng, 200, 130, sub=2), _writer_file(rng, 64, 40, "444")[0],
            _pil_file(rng, 77, 51, mode="L"), _writer_file(rng, 90, 33, "422", restart=2)[0], _pil_file(rng, 310, 180, sub=2)]
    if bad == "truncated":
        d = _pil_file(rng, 300, 200, sub=2)
        b = d[:len(d) // 2]
    elif bad == "progressive":
        PIL = pytest.importorskip("PIL.Image")
        bio = io.BytesIO()
        PIL.fromarray(rng.integers(0, 255, (64, 96, 3), dtype=np.uint8)).save(bio, "JPEG", progressive=True, quality=80)
        b = bio.getvalue()
    else:
        q = synth.quant_tables()
        coef = [synth._blocks(rng, 2 * 2 * 3, q[0]), synth._blocks(rng, 4, q[1]), synth._blocks(rng, 4, q[1])]
        b = jpeg_writer.encode(48, 16, 3, 1, coef, q)
    files = good[:3] + [b] + good[3:]
    geoms, images, _, status = ops.jpeg_decode_files_mixed_device(files, n_threads=4, strict=False)
    assert status[3] != 0 and images[3] is None
    for i, d in enumerate(files):
        if i != 3:
            assert status[i] == 0
            assert np.array_equal(images[i], _alone(d)), i


# ---------------------------------------------------------------------------------------------------- 5. a uniform batch
def test_uniform_4k_batch_through_items_equals_recon_batch():
    L = capi.require_device()
    n, mc, mr = 64, 240, 135
    geom = capi.jpeg_geom(mc, mr)
    cy1, cu1, cv1 = synth.coef_batch(4, mc, mr)
    reps = n // 4
    dy = _upload(np.tile(cy1, reps)); du = _upload(np.tile(cu1, reps)); dv = _upload(np.tile(cv1, reps))
    dq = _upload(np.tile(synth.quant_tables().reshape(-1), n))
    pitch = geom.width * 4 + 1024
    stride = pitch * geom.height
    a = ops.DeviceBuffer(nbytes=n * stride)
    b = ops.DeviceBuffer(nbytes=n * stride)
    capi.check(L.ffhip_memset(a.ptr, 0, n * stride, None)); capi.check(L.ffhip_memset(b.ptr, 0, n * stride, None))
    ops.jpeg_recon_batch(geom, n, dy.ptr, du.ptr, dv.ptr, dq.ptr, 256, a.ptr, pitch, stride)
    yb, cb = geom.y_blocks * 128, geom.c_blocks * 128
    items = []
    for i in range(n):
        it = capi.JpegItem()
        it.geom = geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v = dy.ptr + i * yb, du.ptr + i * cb, dv.ptr + i * cb
        it.d_quant, it.d_bgra, it.pitch = dq.ptr + i * 512, b.ptr + i * stride, pitch
        items.append(it)
    ops.jpeg_recon_items(items)
    capi.check(L.ffhip_stream_sync(None))
    for k in range(0, n, 16):       # compared in slices: 2 GB of pixels
        ha = np.empty(16 * stride, np.uint8); hb = np.empty(16 * stride, np.uint8)
        capi.check(L.ffhip_memcpy_d2h(ha.ctypes.data, a.ptr + k * stride, 16 * stride, None))
        capi.check(L.ffhip_memcpy_d2h(hb.ctypes.data, b.ptr + k * stride, 16 * stride, None))
        capi.check(L.ffhip_stream_sync(None))
        assert np.array_equal(ha, hb), k


# ---------------------------------------------------------------------------------------------------- 6. thumbnails
def test_4096_thumbnails_of_64_sizes(entropy_env):
    entropy_env(None)
    rng = np.random.default_rng(21)
    sizes = [(int(rng.integers(24, 160)), int(rng.integers(24, 160))) for _ in range(64)]
    layouts = ["420", "444", "422", "grey"]
    protos = [_writer_file(rng, w, h, layouts[k % 4], restart=(k % 3) * 2)[0] for k, (w, h) in enumerate(sizes)]
    alone = [_alone(p) for p in protos]
    pick = rng.integers(0, 64, 4096)
    files = [protos[int(i)] for i in pick]
    _, images, _ = ops.jpeg_decode_files_mixed_device(files, n_threads=8)
    for i, img in zip(pick, images):
        assert np.array_equal(img, alone[int(i)])


# ---------------------------------------------------------------------------------------------------- 7. two threads, two streams
def test_two_threads_on_two_streams():
    L = capi.require_device()
    rng = np.random.default_rng(31)
    batches = []
    for t in range(2):
        fs = [_writer_file(rng, int(rng.integers(8, 400)), int(rng.integers(8, 300)), list(LAYOUTS)[(k + t) % 7], restart=k % 4)[0]
              for k in range(24)]
        fs += [_pil_file(rng, 260 + 40 * t, 170, sub=2), _pil_file(rng, 150, 90 + t, mode="L")]
        batches.append(fs)
    expect = [[_alone(d) for d in fs] for fs in batches]
    streams = [L.ffhip_stream_create() for _ in range(2)]
    results, errors = [None, None], []

    def run(t):
        try:
            for _ in range(3):
                got = ops.jpeg_decode_files_mixed_device(batches[t], n_threads=4, stream=streams[t])[1]
                assert all(np.array_equal(a, b) for a, b in zip(got, expect[t]))
            results[t] = True
        except Exception as e:          # reported below, on the main thread
            errors.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for s in streams:
        L.ffhip_stream_destroy(s)
    assert not errors, errors
    assert results == [True, True]


# ---------------------------------------------------------------------------------------------------- 8. one file call per pixel rule
RULE_SIZES = [(16, 16), (72, 40), (33, 17), (50, 24), (24, 40), (61, 35), (17, 16), (40, 39), (72, 16), (19, 23), (64, 40), (45, 31)]
RULE_LAYOUTS = ["420", "444", "grey"]
RULES = ["full", "scaled", "libjpeg"]


@pytest.fixture(scope="module")
def rule_files():
    """twelve small files of three layouts (restart markers on some) with a truncated file in the middle -> (files, index of the bad one);
    the bad file's header is whole: it is probed, classified and takes its place in its class, and only its scan fails"""
    rng = np.random.default_rng(41)
    files = [_writer_file(rng, w, h, RULE_LAYOUTS[k % 3], restart=(k % 4) * 2)[0] for k, (w, h) in enumerate(RULE_SIZES)]
    whole = _writer_file(rng, 64, 40, "420")[0]
    sos = whole.rfind(b"\xff\xda")
    files.insert(6, whole[:sos + (len(whole) - sos) // 3])
    return files, 6


def _rule_items_call(rule, geom, w, h, denom, planes, quant, pitch, rows):
    """the public items call of the rule on one file's own coefficients -> its output, rows x pitch bytes over 0xA5"""
    L = capi.lib()
    keep = [_upload(p) if p is not None else None for p in planes] + [_upload(quant)]
    out = _upload(np.full(rows * pitch, 0xA5, np.uint8))
    it = capi.JpegItem()
    it.geom = geom
    it.d_coef_y, it.d_coef_u, it.d_coef_v = [b.ptr if b is not None else None for b in keep[:3]]
    it.d_quant, it.d_bgra, it.pitch = keep[3].ptr, out.ptr, pitch
    if rule == "full":
        ops.jpeg_recon_items([it])
    elif rule == "scaled":
        ops.jpeg_recon_items_scaled([it], [denom])
    else:
        ops.jpeg_recon_items_libjpeg([it], [(w, h)])
    capi.check(L.ffhip_stream_sync(None))
    return out.to_host((rows, pitch), np.uint8)


@pytest.mark.parametrize("device_entropy", ["0", "1"])
@pytest.mark.parametrize("rule", RULES)
def test_each_pixel_rule_in_a_file_call_equals_its_items_call(rule_files, entropy_env, rule, device_entropy):
    """ffhip_jpeg_decode_files_mixed_device_ex under each rule -- denominators all 1, denominators 1, 2, 4, 8 in turn, libjpeg's pixels -- over
    the same files: every good file's picture is what the rule's public items call makes of that file's own coefficients
    (ffhip_jpeg_entropy_decode, upload, ffhip_jpeg_recon_items / _scaled / _libjpeg), so a denominator or display size that reached the
    reconstruction from another file's place -- a part's offset, or the host threads' list of good files, which is shorter than the class --
    shows.  The bad file has its code, the call returns it, and the guard bytes behind every row and every output keep their 0xA5."""
    L = capi.require_device()
    entropy_env(device_entropy)
    files, bad = rule_files
    n = len(files)
    denom = [1] * n if rule != "scaled" else [(1, 2, 4, 8)[i % 4] for i in range(n)]
    probed = [ops.jpeg_probe(f) for f in files]
    sizes, offs, pitches, total = [], [], [], 32
    for i, ((g, w, h), d) in enumerate(zip(probed, denom)):
        cw, chh = g.width // d, g.height // d                                       # the coded picture at 1 / d
        pitch = (4 * cw + 15) // 16 * 16 + 16 * (i % 2)                            # a guard behind every row of every other file
        sizes.append((cw, chh))
        offs.append(total)
        pitches.append(pitch)
        total += pitch * chh + 16 * (1 + i % 3)
    dout = _upload(np.full(total, 0xA5, np.uint8))
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    outs = (C.c_void_p * n)(*[dout.ptr + o for o in offs])
    geoms, status = (capi.JpegGeom * n)(), (C.c_int * n)()
    rc = L.ffhip_jpeg_decode_files_mixed_device_ex(ptrs, lens, n, 4, outs, (C.c_int64 * n)(*pitches), None if rule == "libjpeg" else (C.c_int * n)(*denom),
                                                   capi.FFHIP_JPEG_PIXELS_LIBJPEG if rule == "libjpeg" else 0, geoms, status, None)
    capi.check(L.ffhip_stream_sync(None))
    status = list(status)
    assert status[bad] != 0 and rc == status[bad], (rc, status)
    assert all(s == 0 for i, s in enumerate(status) if i != bad), status
    got = dout.to_host((total,), np.uint8)
    written = np.zeros(total, bool)
    for i, ((g, w, h), d, (cw, chh), off, pitch) in enumerate(zip(probed, denom, sizes, offs, pitches)):
        rows = np.lib.stride_tricks.as_strided(got[off:], (chh, 4 * cw), (pitch, 1))
        np.lib.stride_tricks.as_strided(written[off:], (chh, 4 * cw), (pitch, 1))[...] = True
        if i == bad:
            continue
        cy = np.empty(g.y_blocks * 64, np.int16)
        cu, cv = (np.empty(g.c_blocks * 64, np.int16), np.empty(g.c_blocks * 64, np.int16)) if g.ncomp == 3 else (None, None)
        quant = np.empty((4, 64), np.uint16)
        capi.check(L.ffhip_jpeg_entropy_decode(bufs[i].ctypes.data, bufs[i].size, C.byref(g), cy.ctypes.data, cu.ctypes.data if cu is not None else None,
                                               cv.ctypes.data if cv is not None else None, quant.ctypes.data), "ffhip_jpeg_entropy_decode")
        want = _rule_items_call(rule, g, w, h, d, (cy, cu, cv), quant, pitch, chh)[:, :4 * cw]
        if rule == "libjpeg":                                                       # outside the display rectangle the bytes are unspecified
            rows, want = rows[:h, :4 * w], want[:h, :4 * w]
        assert np.array_equal(rows, want), (i, rule, d, int((rows != want).sum()))
    assert (got[~written] == 0xA5).all(), np.flatnonzero((got != 0xA5) & ~written)[:8]
