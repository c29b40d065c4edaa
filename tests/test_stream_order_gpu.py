"""GPU: the enqueue-only entry points hold their stream-order contract (include/ffpic_hip.h; DESIGN.md "Stream order").

Every case runs the scenario of stream_order.py: the entry is called on a stream that is stalled by K 256 MiB copies, its stream-ordered
inputs arrive by device-to-device copies behind the stall (the buffers hold a valid DECOY input when the call is made), a consumer copies
the outputs behind the call and the decoy is written back over the inputs behind that.  Right behind the last enqueue the stall's marker
must still be pending (otherwise the case fails as inconclusive); after the sync the consumer's copy must be, byte for byte, what the
suite's oracles give for the REAL input.  A side stream that does not wait for the caller's stream, a missing join, a pre-pass that reads
an input early, a staging buffer refilled under a queued upload: each of them shows as the decoy's bytes (or 0xA5) in the copy.  The
negative controls run the same scenario with the contract broken by the CALLER (producer on another stream) and must see the decoy's output:
the decoys differ, the stall outlasts the call, and the scenario tells the two apart.

Stall length (measured on an MI355X; per case in DESIGN.md 4.15): one 256 MiB ffhip_copy_calibrate copy takes 0.081 ms; the longest
enqueue sequence among the cases takes 1.47 ms of host time (ffhip_jpeg_recon_items, the first case to run, with whatever the process
does once in it; the longest in the steady state is the HEVC chain x2, 0.98 ms); K = 128 copies stall for 10.3 ms, 7.0 times 1.47 ms,
and stay far under half a second.  test_stall_is_long_enough measures the copy again, holds K to the rule K x copy >= 4 x 1.47 ms, and
prints the host time of every enqueue sequence the session has run (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import exif_cases as X
import jpeg_scaled_rule as R
import oracle_lib as O
import stream_order as SO
from ffpic_amd import capi, ops, synth, tensors
from stream_order import Operand, Output
from test_color_gpu import oracle_420_8, oracle_420_16
from test_heif_gpu import expected_canvas
from test_hevc_gpu import oracle_tus
from test_jpeg_mixed_gpu import LAYOUTS, build_items
from test_resize_gpu import expected, make_format, resize_rule
from test_vp8_frames_gpu import oracle_chain
from test_vp8_lf_gpu import oracle_lf

pytestmark = pytest.mark.gpu

COPY_MS = 0.081        # measured: one 256 MiB copy
HOST_MS_MAX = 1.47     # measured: the longest enqueue sequence (ffhip_jpeg_recon_items as the first case of the module)
K = 128                # copies of one stall: 10.3 ms, 7.0 x HOST_MS_MAX
FILL = SO.FILL
BIL, AA = capi.FFHIP_RESIZE_BILINEAR, capi.FFHIP_RESIZE_ANTIALIAS
U8, F16 = capi.FFHIP_TENSOR_U8, capi.FFHIP_TENSOR_F16


# ---------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def stall():
    capi.require_device(0)
    return SO.Stall()


@pytest.fixture(params=["created", "null"])
def stream(request):
    L = capi.require_device(0)
    if request.param == "null":
        yield None
        return
    s = L.ffhip_stream_create()
    assert s
    yield s
    L.ffhip_stream_destroy(s)


@pytest.fixture
def two_streams(stall):
    """(s, other): two created streams of which `s` runs its work while `other` is stalled -- the first of up to eight candidates that
    does (streams that share a hardware queue do not, and which ones share is the runtime's choice)"""
    L = capi.require_device(0)
    made = [L.ffhip_stream_create() for _ in range(9)]
    assert all(made)
    other = made[0]
    s = next((c for c in made[1:] if stall.runs_beside(c, other)), None)
    yield s, other
    for c in made:
        L.ffhip_stream_destroy(c)


class Case:
    """An entry point with its operands in device memory.  call(s) enqueues it on s; expect(which) -> what each output's copy must hold
    (arrays of the outputs' sizes, 0xA5 where the entry writes nothing) for which = "true" or "decoy"."""

    def __init__(self, name, call, operands, outputs, expect, memsets=(), overwrite=True, keep=None):
        self.name, self.call, self.operands, self.outputs, self.expect = name, call, list(operands), list(outputs), expect
        self.memsets, self.overwrite, self.keep = list(memsets), overwrite, keep


def assert_outputs(case, which, read="copied"):
    for k, (o, e) in enumerate(zip(case.outputs, case.expect(which))):
        got, e = getattr(o, read)(), SO.as_bytes(e)
        assert got.size == e.size, (case.name, k, got.size, e.size)
        assert np.array_equal(got, e), (case.name, which, read, k, np.flatnonzero(got != e)[:4], int((got != e).sum()))


def run_case(case, stall, s):
    rc = SO.run(case.name, stall, s, K, case.call, case.operands, case.outputs, case.memsets, case.overwrite)
    assert rc == 0, rc
    assert_outputs(case, "true")


def run_control(case, stall, streams):
    s, other = streams
    assert s, "inconclusive: no created stream runs beside another one's stall"
    rc = SO.run_broken(case.name, stall, s, other, K, case.call, case.operands, case.outputs, case.memsets)
    assert rc == 0, rc
    assert_outputs(case, "decoy")


def pick(which, true, decoy):
    return true if which == "true" else decoy


def place(buf, off, shape, pitch, pixels):
    """`pixels` [h][w][bytes] into the flat byte array `buf` at `off`, rows `pitch` bytes apart"""
    h, w, b = shape
    np.lib.stride_tricks.as_strided(buf[off:], (h, w, b), (pitch, b, 1))[...] = np.asarray(pixels).reshape(h, w, b)


# ---------------------------------------------------------------------------------------------------- JPEG
JPEG_SPECS = [("420", 3, 2), ("444", 1, 1), ("grey", 17, 3)]
JPEG_SMALL = [("444", 1, 1), ("420", 1, 1), ("grey", 2, 1), ("422", 1, 2)]


def small_items(specs):
    """items, places and total as build_items gives them, without its device copies (the second call of a pair has hundreds of items):
    pictures of one spec share their planes, offsets and pitches vary in turn"""
    items, places, planes, total = [], [], {}, 0
    for k, (lay, mc, mr) in enumerate(specs):
        ncomp, h, v = LAYOUTS[lay]
        geom = capi.jpeg_geom(mc, mr, ncomp, h, v)
        if (lay, mc, mr) not in planes:
            planes[lay, mc, mr] = synth.coef_batch(1, mc, mr, ncomp, h, v, first=k)
        total += 16 * (k % 5)
        pitch = geom.width * 4 + 16 * (k % 3)
        places.append((geom, total, pitch, planes[lay, mc, mr]))
        total += pitch * geom.height
        it = capi.JpegItem()
        it.geom = geom
        items.append(it)
    return items, places, total + 64


def jpeg_items_case(name, specs, denom=None, seed=0, many=False):
    """ffhip_jpeg_recon_items (denom None) / ffhip_jpeg_recon_items_scaled (every item at 1 / denom) on the pictures of `specs`;
    stream-ordered: every coefficient plane and the quantiser tables"""
    L = capi.lib()
    rng = np.random.default_rng(31 + seed)
    q, qd = synth.quant_tables(), synth.quant_tables(quality=50)
    if many:
        items, places, total = small_items(specs)
    else:
        items, places, _, total, _ = build_items(L, specs, rng, q, adversarial=False)      # (its own device copies are not used here)
    if denom:
        n, total, scaled = 8 // denom, 0, []
        for geom, _, _, planes in places:
            w, h = n * geom.h * geom.mcu_cols, n * geom.v * geom.mcu_rows
            pitch = (4 * w + 15) // 16 * 16 + 16 * (len(scaled) % 3)
            total += 32
            scaled.append((geom, total, pitch, planes))
            total += pitch * h
        total += 64
        places = scaled
    dq, out = Operand(q, qd), Output(total)
    operands, planes = [dq], {"true": [], "decoy": []}
    shared = {}                                                   # pictures of one spec read the same planes: many items, few producers
    for k, (it, (geom, off, pitch, true)) in enumerate(zip(items, places)):
        if specs[k] not in shared:
            decoy = synth.coef_batch(1, geom.mcu_cols, geom.mcu_rows, geom.ncomp, geom.h, geom.v, first=1000 + k + seed)
            devs = [Operand(t, d) if t is not None else None for t, d in zip(true, decoy)]
            operands += [d for d in devs if d is not None]
            shared[specs[k]] = (true, decoy, devs)
        true, decoy, devs = shared[specs[k]]
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [d.ptr if d is not None else None for d in devs]
        it.d_quant, it.d_bgra, it.pitch = dq.ptr, out.ptr + off, pitch
        planes["true"].append(true)
        planes["decoy"].append(decoy)
    arr = (capi.JpegItem * len(items))(*items)
    den = (C.c_int * len(items))(*([denom or 1] * len(items)))

    def call(s):
        if denom:
            capi.check(L.ffhip_jpeg_recon_items_scaled(arr, den, len(items), s), "ffhip_jpeg_recon_items_scaled")
        else:
            capi.check(L.ffhip_jpeg_recon_items(arr, len(items), s), "ffhip_jpeg_recon_items")

    def expect(which):
        buf = np.full(total, FILL, np.uint8)
        quant = pick(which, q, qd)
        for (geom, off, pitch, _), (cy, cu, cv) in zip(places, planes[which]):
            if denom:
                px = R.picture(geom.mcu_cols, geom.mcu_rows, geom.ncomp, geom.h, geom.v, cy, cu, cv, quant, denom)
            else:
                px = O.oracle_jpeg_recon(O.make_geom(geom.mcu_cols, geom.mcu_rows, geom.ncomp, geom.h, geom.v), cy, cu, cv, quant, n_images=1)
                px = px.reshape(geom.height, geom.width, 4)
            place(buf, off, px.shape, pitch, px)
        return [buf]
    return Case(name, call, operands, [out], expect)


def jpeg_items_libjpeg_case(name, specs, seed=0):
    """ffhip_jpeg_recon_items_libjpeg on the pictures of `specs`, every display size short of the coded one in both directions (the chroma
    grid ends inside the last MCU: its edge replication is live); stream-ordered: every coefficient plane and the quantiser tables.  The
    expected bytes are the host function's (ffhip_jpeg_libjpeg_picture) inside the display rectangles; what the call writes of a coded
    picture outside its display rectangle is unspecified and is taken from the consumer's copy"""
    L = capi.lib()
    q, qd = synth.quant_tables(), synth.quant_tables(quality=50)
    items, places, total = small_items(specs)
    shown = [(geom.width - 1 - 2 * (k % 2), geom.height - 3) for k, (geom, _, _, _) in enumerate(places)]
    dq, out = Operand(q, qd), Output(total)
    operands, shared, pictures = [dq], {}, {}
    for k, (it, (geom, off, pitch, true)) in enumerate(zip(items, places)):
        if specs[k] not in shared:
            decoy = synth.coef_batch(1, geom.mcu_cols, geom.mcu_rows, geom.ncomp, geom.h, geom.v, first=1000 + k + seed)
            devs = [Operand(t, d) if t is not None else None for t, d in zip(true, decoy)]
            operands += [d for d in devs if d is not None]
            shared[specs[k]] = (true, decoy, devs)
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [d.ptr if d is not None else None for d in shared[specs[k]][2]]
        it.d_quant, it.d_bgra, it.pitch = dq.ptr, out.ptr + off, pitch
    arr = (capi.JpegItem * len(items))(*items)
    sizes = (capi.Size * len(items))(*[capi.Size(w, h) for w, h in shown])

    def call(s):
        capi.check(L.ffhip_jpeg_recon_items_libjpeg(arr, sizes, len(items), s), "ffhip_jpeg_recon_items_libjpeg")

    def expect(which):
        buf, got = np.full(total, FILL, np.uint8), out.copied()
        for k, ((geom, off, pitch, _), (w, h)) in enumerate(zip(places, shown)):
            key = (which, specs[k], w, h)                          # pictures of one spec and display size are one host picture
            if key not in pictures:
                pictures[key] = ops.jpeg_libjpeg_picture(geom, w, h, *shared[specs[k]][which == "decoy"], pick(which, q, qd))
            coded = np.lib.stride_tricks.as_strided(got[off:], (geom.height, geom.width, 4), (pitch, 4, 1)).copy()
            coded[:h, :w] = pictures[key]
            place(buf, off, coded.shape, pitch, coded)
        return [buf]
    return Case(name, call, operands, [out], expect)


def jpeg_batch_case(h=2, v=2, mc=5, mr=4, n=2):
    """ffhip_jpeg_recon_batch; stream-ordered: planes, quantiser tables and (two-pass layouts) the caller's workspace"""
    L = capi.lib()
    geom = capi.jpeg_geom(mc, mr, 3, h, v)
    q, qd = synth.quant_tables(), synth.quant_tables(quality=50)
    true, decoy = synth.coef_batch(n, mc, mr, 3, h, v), synth.coef_batch(n, mc, mr, 3, h, v, first=77)
    devs = [Operand(t, d) for t, d in zip(true, decoy)]
    dq = Operand(q, qd)
    H, W = geom.height, geom.width
    out = Output(n * H * W * 4)
    ws_bytes = L.ffhip_jpeg_workspace_bytes(C.byref(geom), n)
    assert (ws_bytes > 0) == (h == 3), ws_bytes
    operands = devs + [dq]
    ws = None
    if ws_bytes:          # scratch of the call: whatever the stream put there before is gone, whatever comes behind may overwrite it
        rng = np.random.default_rng(5)
        ws = Operand(rng.integers(0, 256, ws_bytes, dtype=np.uint8), rng.integers(0, 256, ws_bytes, dtype=np.uint8))
        operands.append(ws)

    def call(s):
        capi.check(L.ffhip_jpeg_recon_batch(C.byref(geom), n, devs[0].ptr, devs[1].ptr, devs[2].ptr, dq.ptr, 0, out.ptr, W * 4, H * W * 4,
                                            ws.ptr if ws else None, ws_bytes, s), "ffhip_jpeg_recon_batch")

    def expect(which):
        cy, cu, cv = pick(which, true, decoy)
        return [O.oracle_jpeg_recon(O.make_geom(mc, mr, 3, h, v), cy, cu, cv, pick(which, q, qd), n_images=n)]
    return Case(f"jpeg_recon_batch h{h}v{v}", call, operands, [out], expect)


def test_jpeg_recon_items(stall, stream):
    run_case(jpeg_items_case("jpeg_recon_items", JPEG_SPECS), stall, stream)


@pytest.mark.parametrize("denom", [2, 8])
def test_jpeg_recon_items_scaled(stall, stream, denom):
    run_case(jpeg_items_case(f"jpeg_recon_items_scaled d{denom}", JPEG_SPECS, denom), stall, stream)


@pytest.mark.parametrize("h,v,mc,mr", [(2, 2, 5, 4), (3, 1, 3, 2)])
def test_jpeg_recon_batch(stall, stream, h, v, mc, mr):
    run_case(jpeg_batch_case(h, v, mc, mr), stall, stream)


# ---------------------------------------------------------------------------------------------------- colour
def oracle_400_16(y, r, c, ctb):
    H, W = y.shape
    o = np.zeros((H, W * 4), np.uint8)
    O.ffo().ffo_yuv400_to_bgra32_16bit(o.reshape(-1), W * 4, np.ascontiguousarray(y).reshape(-1), W, r, c, ctb)
    return o


def colour_case(bits):
    """ffhip_yuv420_to_bgra (bits 8: 2 x 3 macroblocks) / ffhip_yuv420_to_bgra_16 (16) / ffhip_yuv400_to_bgra_16 (400: luma only), the
    last two on 2 x 3 coding tree blocks of 16; stream-ordered: the planes"""
    L = capi.lib()
    rows, cols, unit = 2, 3, 16
    H, W = rows * unit, cols * unit
    dt = np.uint8 if bits == 8 else np.int16
    name = {8: "yuv420_to_bgra", 16: "yuv420_to_bgra_16", 400: "yuv400_to_bgra_16"}[bits]

    def planes(seed):
        rng = np.random.default_rng(seed)
        return [rng.integers(0, 256, sh).astype(dt) for sh in [(H, W)] + [(H // 2, W // 2)] * (0 if bits == 400 else 2)]
    true, decoy = planes(600 + bits), planes(700 + bits)
    devs = [Operand(t, d) for t, d in zip(true, decoy)]
    out = Output(H * W * 4)

    def call(s):
        if bits == 8:
            capi.check(L.ffhip_yuv420_to_bgra(out.ptr, W * 4, devs[0].ptr, devs[1].ptr, devs[2].ptr, W, W // 2, rows, cols, 1, H * W, H * W // 4, H * W * 4, s))
        elif bits == 16:
            capi.check(L.ffhip_yuv420_to_bgra_16(out.ptr, W * 4, devs[0].ptr, devs[1].ptr, devs[2].ptr, W, W // 2, rows, cols, unit, 1, H * W, H * W // 4,
                                                 H * W * 4, s))
        else:
            capi.check(L.ffhip_yuv400_to_bgra_16(out.ptr, W * 4, devs[0].ptr, W, rows, cols, unit, 1, H * W, H * W * 4, s))

    def expect(which):
        p = pick(which, true, decoy)
        return [oracle_420_8(*p, rows, cols) if bits == 8 else oracle_420_16(*p, rows, cols, unit) if bits == 16 else oracle_400_16(*p, rows, cols, unit)]
    return Case(name, call, devs, [out], expect)


@pytest.mark.parametrize("bits", [8, 16, 400])
def test_yuv420_to_bgra(stall, stream, bits):
    run_case(colour_case(bits), stall, stream)


# ---------------------------------------------------------------------------------------------------- HEVC residual
def hevc_residual_case(n, n_tu):
    """ffhip_hevc_residual_batch; stream-ordered: levels, TU info and the scaling lists"""
    L = capi.lib()

    def inputs(seed):
        rng = np.random.default_rng(seed)
        lv = np.rint(rng.laplace(0, 10, size=(n_tu, n * n))).astype(np.int16)
        info = np.zeros((n_tu, 4), np.uint8)
        info[:, 0] = rng.integers(0, 52, size=n_tu)
        flags = rng.choice([0, 0, 0, 2, 4, 2 | 8, 4 | 8] + ([1, 1] if n == 4 else []), size=n_tu)
        info[:, 1] = flags if n == 4 else flags & ~8
        info[:, 2] = rng.integers(0, 6, size=n_tu)
        return lv, info, rng.integers(1, 256, size=(6, n * n)).astype(np.uint8)
    true, decoy = inputs(n * 1000 + n_tu), inputs(n * 1000 + n_tu + 1)
    devs = [Operand(t, d) for t, d in zip(true, decoy)]
    out = Output(n_tu * n * n * 2)

    def call(s):
        capi.check(L.ffhip_hevc_residual_batch(n, n_tu, devs[0].ptr, devs[1].ptr, devs[2].ptr, 10, 0, out.ptr, s), "ffhip_hevc_residual_batch")

    def expect(which):
        lv, info, sc = pick(which, true, decoy)
        return [oracle_tus(n, lv, info, 10, False, sc)]
    return Case(f"hevc_residual_batch n{n}", call, devs, [out], expect)


@pytest.mark.parametrize("n,n_tu", [(4, 777), (32, 5)])
def test_hevc_residual_batch(stall, stream, n, n_tu):
    run_case(hevc_residual_case(n, n_tu), stall, stream)


# ---------------------------------------------------------------------------------------------------- HEVC intra
def other_residual(res, seed):
    return np.rint(np.random.default_rng(seed).laplace(0, 12, size=res.shape)).astype(np.int16)


def hevc_planes(w, h):
    """three int16 plane outputs of a 4:2:0 picture and the in-stream memsets that zero them (a producer: the oracle's planes start at 0)"""
    outs = [Output(w * h * 2), Output(w * h // 2), Output(w * h // 2)]
    return outs, [(o.ptr, 0, o.nbytes) for o in outs]


_HEVC_LISTS = {}


def hevc_list(w, h, seed, **kw):
    """(tus, residual) of synth.hevc_intra_tus; made once per module"""
    key = (w, h, seed, tuple(sorted(kw.items())))
    if key not in _HEVC_LISTS:
        _HEVC_LISTS[key] = synth.hevc_intra_tus(w, h, seed, **kw)
    return _HEVC_LISTS[key]


def hevc_intra_case(w, h, seed):
    """ffhip_hevc_intra_recon; stream-ordered: d_residual and d_tus (h_tus holds the real records when the call is made; the decoy list is
    the same records with the prediction modes permuted: every host decision -- validation, window, residual needed -- is the same)"""
    L = capi.lib()
    tus, res = hevc_list(w, h, seed)
    tus = np.ascontiguousarray(tus)
    rng = np.random.default_rng(seed)
    decoy_tus = tus.copy()
    free = np.flatnonzero((tus["flags"] & synth.TU_RDPCM) == 0)          # (an rdpcm TU keeps its mode: the flag goes with modes 10 and 26)
    decoy_tus["pred_mode"][free] = tus["pred_mode"][rng.permutation(free)]
    decoy_res = other_residual(res, seed + 1)
    dt, dr = Operand(tus.view(np.uint8), decoy_tus.view(np.uint8)), Operand(res, decoy_res)
    outs, memsets = hevc_planes(w, h)

    def call(s):
        capi.check(L.ffhip_hevc_intra_recon(tus.ctypes.data, dt.ptr, len(tus), dr.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, w, h, w, w // 2, h // 2, w // 2,
                                            8, 8, s), "ffhip_hevc_intra_recon")

    def expect(which):
        return list(O.oracle_hevc_intra(pick(which, tus, decoy_tus), pick(which, res, decoy_res), w, h, True, 8, 8))
    return Case(f"hevc_intra_recon {w}x{h}", call, [dt, dr], outs, expect, memsets, keep=tus)


def assert_device_planner_took_the_list():
    out = (C.c_uint32 * 8)()
    capi.check(capi.lib().ffhip_debug_hevc_plan_result(out), "ffhip_debug_hevc_plan_result")
    assert out[0] == 0 and out[6] == 0 and out[1] > 0, list(out)


BIG = (1600, 1024, 5)       # (width, height, seed) of a list of 33 594 records: at 2^15 and more the library forks its side stream


def test_hevc_intra_recon_everything_on_the_stream(stall, stream):
    case = hevc_intra_case(192, 128, 71)
    assert len(case.keep) < 1 << 15
    run_case(case, stall, stream)
    assert_device_planner_took_the_list()


def test_hevc_intra_recon_forked_side_stream(stall, stream):
    """a list of at least 2^15 records: the substitution table, the depth sweep and the ticket kernels run on the thread's side stream
    (fork / mid / join), the per-pixel programs early on the caller's"""
    case = hevc_intra_case(*BIG)
    assert len(case.keep) >= 1 << 15, len(case.keep)
    run_case(case, stall, stream)
    assert_device_planner_took_the_list()


def hevc_tiles_case(decode, calls=3):
    """ffhip_hevc_intra_recon_tiles / ffhip_hevc_decode_tiles, `calls` of them back to back on ONE list (d_tus is ready when the call is
    made, as the header demands) with a residual buffer and a plane set each: both scratch sets and their guard events are crossed.
    Stream-ordered: d_residual.  Every call has its own consumer copy."""
    L = capi.lib()
    w, h = 512, 256
    tus, res = hevc_list(w, h, 41, tu_mix="c5")
    tus = np.ascontiguousarray(tus)
    d_tus = ops.DeviceBuffer(host=tus.view(np.uint8))
    tf = np.zeros(1, np.int64)
    true = [res] + [other_residual(res, 410 + i) for i in range(1, calls)]
    decoy = [other_residual(res, 420 + i) for i in range(calls)]
    drs = [Operand(t, d) for t, d in zip(true, decoy)]
    sets = [hevc_planes(w, h) for _ in range(calls)]
    bgra = [Output(w * h * 4) for _ in range(calls)] if decode else []

    def one(i, s):
        (y, u, v), _ = sets[i]
        if decode:
            capi.check(L.ffhip_hevc_decode_tiles(tus.ctypes.data, d_tus.ptr, len(tus), tf.ctypes.data, 1, drs[i].ptr, y.ptr, u.ptr, v.ptr, w, h, w, w // 2, h // 2,
                                                 w // 2, 8, 8, bgra[i].ptr, w * 4, s), "ffhip_hevc_decode_tiles")
        else:
            capi.check(L.ffhip_hevc_intra_recon_tiles(tus.ctypes.data, d_tus.ptr, len(tus), tf.ctypes.data, 1, drs[i].ptr, y.ptr, u.ptr, v.ptr, w, h, w, w // 2,
                                                      h // 2, w // 2, 8, 8, s), "ffhip_hevc_intra_recon_tiles")

    def outputs_of(i):
        return sets[i][0] + ([bgra[i]] if decode else [])

    def expect_of(i, which):
        planes = list(O.oracle_hevc_intra(tus, pick(which, true, decoy)[i], w, h, True, 8, 8))
        return planes + ([oracle_420_16(planes[0], planes[1], planes[2], h // 64, w // 64, 64)] if decode else [])
    return one, drs, sets, outputs_of, expect_of, (tus, d_tus, tf)


@pytest.mark.parametrize("decode", [False, True], ids=["recon_tiles", "decode_tiles"])
def test_hevc_tile_calls_back_to_back(stall, stream, decode):
    calls = 3
    one, drs, sets, outputs_of, expect_of, keep = hevc_tiles_case(decode, calls)
    name = "hevc_decode_tiles x3" if decode else "hevc_intra_recon_tiles x3"
    for i in range(calls):                                  # the warm-up: both scratch sets grow here
        SO.warm_up(stream, lambda s: one(i, s), [drs[i]], outputs_of(i), sets[i][1])
    with SO.Scenario(name, stall, stream, K) as sc:
        sc.produce(drs)
        for i in range(calls):
            sc.produce((), sets[i][1])
            one(i, stream)
            sc.consume(outputs_of(i))
        sc.overwrite(drs)
        sc.still_stalled()
    assert sc.finish() == 0
    for i in range(calls):
        assert_outputs(Case(f"{name} call {i}", None, [], outputs_of(i), lambda which, i=i: expect_of(i, which)), "true")


# ---------------------------------------------------------------------------------------------------- VP8
VC, VR, VN = 21, 13, 2


def vp8_inputs(seed):
    modes = np.ascontiguousarray(np.stack([synth.vp8_modes(VC, VR, seed=seed + i) for i in range(VN)]))
    modes.reshape(VN, VR, VC, 20)[:, 1::2, 0, 0] = 3                        # H_PRED down the first column of every other row
    modes[..., 18] = np.random.default_rng(seed).integers(0, 4, size=modes[..., 18].shape)
    resid = np.ascontiguousarray(np.stack([synth.vp8_residual(VC * VR, seed=seed + 10 + i) for i in range(VN)]))
    return modes, resid, np.ascontiguousarray(synth.vp8_filters(seed=seed))


def vp8_planes():
    n_mb = VC * VR
    outs = [Output(VN * 256 * n_mb), Output(VN * 64 * n_mb), Output(VN * 64 * n_mb)]
    return outs, [(o.ptr, 0, o.nbytes) for o in outs]


def stack_planes(per_image):
    return [np.stack([p[k] for p in per_image]) for k in range(3)]


def vp8_predict_case():
    """ffhip_vp8_predict_recon; stream-ordered: residual, residual map, d_modes (h_modes holds the real records when the call is made) and
    the planes' former contents (the in-stream memset: the wrapped H_PRED of the first column reads them)"""
    L = capi.lib()
    (modes, resid, _), (dmodes, dresid, _) = vp8_inputs(1400), vp8_inputs(1500)
    rng = np.random.default_rng(14)
    n_mb = VC * VR
    resmap = np.tile(np.arange(n_mb, dtype=np.int32), (VN, 1))
    skipped = rng.random((VN, n_mb)) < 0.2
    skipped[:, 0] = False
    for i in range(VN):
        for j in np.flatnonzero(skipped[i]):
            resmap[i, j] = resmap[i, j - 1]                                 # a skipped macroblock shows the last coded one's coefficients
    ident = np.tile(np.arange(n_mb, dtype=np.int32), (VN, 1))
    dm, dr, dmap = Operand(modes, dmodes), Operand(resid, dresid), Operand(resmap, ident)
    outs, memsets = vp8_planes()

    def call(s):
        capi.check(L.ffhip_vp8_predict_recon(VC, VR, VN, modes.ctypes.data, dm.ptr, dr.ptr, n_mb * 384, dmap.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                             256 * n_mb, 64 * n_mb, s), "ffhip_vp8_predict_recon")

    def expect(which):
        m, r, mp = pick(which, (modes, resid, resmap), (dmodes, dresid, ident))
        return stack_planes([O.oracle_vp8_frame(VC, VR, m[i], r[i], mp[i]) for i in range(VN)])
    return Case("vp8_predict_recon", call, [dm, dr, dmap], outs, expect, memsets, keep=modes)


def vp8_loopfilter_case():
    """ffhip_vp8_loopfilter; stream-ordered: the planes (filtered in place), the filter parameters and d_modes"""
    L = capi.lib()
    (modes, _, flt), (dmodes, _, dflt) = vp8_inputs(1400), vp8_inputs(1500)
    n_mb = VC * VR
    true = stack_planes([synth.vp8_blocky_planes(VC, VR, seed=20 + i) for i in range(VN)])
    decoy = stack_planes([synth.vp8_blocky_planes(VC, VR, seed=30 + i) for i in range(VN)])
    planes = [Operand(t, d) for t, d in zip(true, decoy)]
    dm, df = Operand(modes, dmodes), Operand(flt, dflt)
    outs = [Output(p.nbytes, of=p) for p in planes]

    def call(s):
        capi.check(L.ffhip_vp8_loopfilter(VC, VR, VN, 2, dm.ptr, df.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr, 256 * n_mb, 64 * n_mb, s),
                   "ffhip_vp8_loopfilter")

    def expect(which):
        m, f, p = pick(which, (modes, flt, true), (dmodes, dflt, decoy))
        return stack_planes([oracle_lf(VC, VR, 2, m[i], f, [q[i] for q in p]) for i in range(VN)])
    return Case("vp8_loopfilter", call, planes + [dm, df], outs, expect)


def vp8_side_by_side_case(ft):
    """ffhip_vp8_predict_loopfilter; stream-ordered: residual, d_modes, filter parameters and the planes' former contents.  No overwrite
    behind the call: its contract keeps inputs and planes unchanged until ffhip_stream_sync has returned (the sync may repeat the call)."""
    L = capi.lib()
    (modes, resid, flt), (dmodes, dresid, dflt) = vp8_inputs(1400), vp8_inputs(1500)
    n_mb = VC * VR
    dm, dr, df = Operand(modes, dmodes), Operand(resid, dresid), Operand(flt, dflt)
    outs, memsets = vp8_planes()

    def call(s):
        capi.check(L.ffhip_vp8_predict_loopfilter(VC, VR, VN, modes.ctypes.data, dm.ptr, dr.ptr, n_mb * 384, None, ft, df.ptr, outs[0].ptr, outs[1].ptr,
                                                  outs[2].ptr, 256 * n_mb, 64 * n_mb, s), "ffhip_vp8_predict_loopfilter")

    def expect(which):
        m, r, f = pick(which, (modes, resid, flt), (dmodes, dresid, dflt))
        return stack_planes([oracle_lf(VC, VR, ft, m[i], f, O.oracle_vp8_frame(VC, VR, m[i], r[i])) for i in range(VN)])
    return Case(f"vp8_predict_loopfilter ft{ft}", call, [dm, dr, df], outs, expect, memsets, overwrite=False, keep=modes)


def vp8_frames_case(form):
    """ffhip_vp8_decode_frames with BGRA and planes; stream-ordered: residual, d_modes, filter parameters.  The row form is a side-by-side
    call underneath and has its contract: no overwrite behind the call."""
    L = capi.lib()
    (modes, resid, flt), (dmodes, dresid, dflt) = vp8_inputs(1400), vp8_inputs(1500)
    n_mb, H, W = VC * VR, 16 * VR, 16 * VC
    dm, dr, df = Operand(modes, dmodes), Operand(resid, dresid), Operand(flt, dflt)
    planes, _ = vp8_planes()
    bgra = Output(VN * H * W * 4)

    def call(s):
        capi.check(L.ffhip_vp8_decode_frames(VC, VR, VN, modes.ctypes.data, dm.ptr, dr.ptr, n_mb * 384, None, 2, df.ptr, bgra.ptr, W * 4, H * W * 4, planes[0].ptr,
                                             planes[1].ptr, planes[2].ptr, 256 * n_mb, 64 * n_mb, s), "ffhip_vp8_decode_frames")

    def expect(which):
        m, r, f = pick(which, (modes, resid, flt), (dmodes, dresid, dflt))
        chains = [oracle_chain(VC, VR, 2, m[i], r[i], f) for i in range(VN)]
        return [np.stack([c[0] for c in chains])] + stack_planes([c[1] for c in chains])
    return Case(f"vp8_decode_frames {form}", call, [dm, dr, df], [bgra] + planes, expect, overwrite=form == "fused", keep=modes)


def vp8_items_case():
    """ffhip_vp8_decode_items, two frames: simple filter with host modes, normal filter checked on the device; stream-ordered: d_modes,
    residual"""
    L = capi.lib()
    (modes, resid, flt), (dmodes, dresid, _) = vp8_inputs(1400), vp8_inputs(1500)
    H, W = 16 * VR, 16 * VC
    pitch = W * 4 + 32
    out = Output(VN * H * pitch + 64)
    operands, items = [], []
    for i in range(VN):
        dm, dr = Operand(modes[i], dmodes[i]), Operand(resid[i], dresid[i])
        operands += [dm, dr]
        it = capi.Vp8Item()
        it.mbcols, it.mbrows = VC, VR
        it.h_modes = modes[i].ctypes.data if i == 0 else None
        it.d_modes, it.d_residual, it.filter_type = dm.ptr, dr.ptr, 1 + i
        for k, v in enumerate(flt.reshape(-1)):
            it.filters[k] = int(v)
        it.d_bgra, it.pitch = out.ptr + 32 + i * H * pitch, pitch
        items.append(it)
    arr = (capi.Vp8Item * VN)(*items)

    def call(s):
        capi.check(L.ffhip_vp8_decode_items(arr, VN, s), "ffhip_vp8_decode_items")

    def expect(which):
        m, r = pick(which, (modes, resid), (dmodes, dresid))
        buf = np.full(out.nbytes, FILL, np.uint8)
        for i in range(VN):
            place(buf, 32 + i * H * pitch, (H, W, 4), pitch, oracle_chain(VC, VR, 1 + i, m[i], r[i], flt)[0])
        return [buf]
    return Case("vp8_decode_items", call, operands, [out], expect, keep=modes)


def run_vp8_with_retry(case, stall, s):
    """a side-by-side call: where ffhip_stream_sync had to repeat it (FFHIP_RETRIED), what the caller put behind the call is void -- the
    planes themselves hold the answer, and the consumer is enqueued again, as the header tells a caller to"""
    rc = SO.run(case.name, stall, s, K, case.call, case.operands, case.outputs, case.memsets, case.overwrite)
    assert rc in (0, capi.FFHIP_RETRIED), rc
    if rc == capi.FFHIP_RETRIED:
        assert_outputs(case, "true", read="written")
        SO.Scenario(case.name, stall, s, 0).consume(case.outputs)
        assert capi.sync(s) == 0
    assert_outputs(case, "true")


def test_vp8_predict_recon(stall, stream):
    run_case(vp8_predict_case(), stall, stream)


def test_vp8_loopfilter(stall, stream):
    run_case(vp8_loopfilter_case(), stall, stream)


@pytest.mark.parametrize("ft", [1, 2])
def test_vp8_predict_loopfilter(stall, stream, ft):
    run_vp8_with_retry(vp8_side_by_side_case(ft), stall, stream)


@pytest.mark.parametrize("form", ["fused", "rows"])
def test_vp8_decode_frames(stall, stream, form, monkeypatch):
    monkeypatch.setenv("FFHIP_VP8_FRAMES", form)
    capi.reload_env()
    run_vp8_with_retry(vp8_frames_case(form), stall, stream)


def test_vp8_decode_items(stall, stream):
    run_case(vp8_items_case(), stall, stream)


# ---------------------------------------------------------------------------------------------------- resize, orient, tensor items
def pixels(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def layout(sizes, unit=4):
    """outputs of (h, w) pixels of `unit` bytes in one allocation: [(offset, pitch)], total bytes"""
    places, at = [], 16
    for k, (h, w) in enumerate(sizes):
        pitch = unit * w + 4 * (k % 3)
        places.append((at, pitch))
        at += (pitch * h + 16 + 15) // 16 * 16
    return places, at


RESIZE_SHAPES = [((17, 65), (7, 33)), ((40, 5), (3, 64))]          # (source h, w) -> (output h, w)


def resize_case(filt, count=2, seed=0):
    """ffhip_bgra_resize_items; stream-ordered: the source pixels"""
    L = capi.lib()
    shapes = [RESIZE_SHAPES[k % 2] if k < 2 else ((5 + k % 7, 9 + k % 5), (3 + k % 4, 4 + k % 6)) for k in range(count)]
    srcs = {sh: (pixels(800 + seed + k, *sh), pixels(900 + seed + k, *sh)) for k, sh in enumerate(dict.fromkeys(s for s, _ in shapes))}
    devs = {sh: Operand(t, d) for sh, (t, d) in srcs.items()}
    places, total = layout([o for _, o in shapes])
    out = Output(total)
    items = [capi.ResizeItem(devs[sh].ptr, 4 * sh[1], 0, 0, sh[1], sh[0], out.ptr + off, pitch, ow, oh)
             for (sh, (oh, ow)), (off, pitch) in zip(shapes, places)]
    arr = (capi.ResizeItem * count)(*items)

    def call(s):
        capi.check(L.ffhip_bgra_resize_items(arr, count, filt, s), "ffhip_bgra_resize_items")

    def expect(which):
        buf = np.full(total, FILL, np.uint8)
        for (sh, (oh, ow)), (off, pitch) in zip(shapes, places):
            place(buf, off, (oh, ow, 4), pitch, resize_rule(srcs[sh][which == "decoy"], oh, ow, filt))
        return [buf]
    return Case(f"bgra_resize_items f{filt} n{count}", call, list(devs.values()), [out], expect)


def orient_case(count=3, seed=0):
    """ffhip_bgra_orient_items, orientations 2, 6, 8 (and on) of a 70 x 33 source; stream-ordered: the source pixels"""
    L = capi.lib()
    w, h = 70, 33
    true, decoy = pixels(810 + seed, h, w), pixels(910 + seed, h, w)
    src = Operand(true, decoy)
    orients = [(2, 6, 8, 5, 3, 7, 4, 1)[k % 8] for k in range(count)]
    rects = [(0, 0, w, h) if k < 3 else (k % 9, k % 5, 3 + k % 40, 2 + k % 20) for k in range(count)]
    sizes = [X.upright_size(rw, rh, o)[::-1] for (_, _, rw, rh), o in zip(rects, orients)]
    places, total = layout(sizes)
    out = Output(total)
    items = [capi.OrientItem(src.ptr, 4 * w, x0, y0, rw, rh, out.ptr + off, pitch, o) for (x0, y0, rw, rh), o, (off, pitch) in zip(rects, orients, places)]
    arr = (capi.OrientItem * count)(*items)

    def call(s):
        capi.check(L.ffhip_bgra_orient_items(arr, count, s), "ffhip_bgra_orient_items")

    def expect(which):
        buf, px = np.full(total, FILL, np.uint8), pick(which, true, decoy)
        for (x0, y0, rw, rh), o, (uh, uw), (off, pitch) in zip(rects, orients, sizes, places):
            place(buf, off, (uh, uw, 4), pitch, X.orient(px[y0:y0 + rh, x0:x0 + rw], o))
        return [buf]
    return Case(f"bgra_orient_items n{count}", call, [src], [out], expect)


def tensor_case(dtype, planar, count=2, seed=0):
    """ffhip_bgra_to_tensor_items (f16 CHW with mean and std, u8 HWC); stream-ordered: the source pixels"""
    L = capi.lib()
    w, h = 37, 21
    f = make_format(dtype, planar, 0)
    es = 2 if dtype == F16 else 1
    true, decoy = pixels(820 + seed, h, w), pixels(920 + seed, h, w)
    src = Operand(true, decoy)
    rects = [(0, 0, w, h), (3, 2, 17, 9)][:count] + [(k % 11, k % 7, 2 + k % 20, 1 + k % 12) for k in range(2, count)]
    places, at = [], 8
    for (_, _, rw, rh) in rects:                                   # element offsets; rows and planes dense
        places.append(at)
        at += 3 * rw * rh + 5
    total = at * es
    out = Output(total)
    items = [capi.TensorItem(src.ptr, 4 * w, x0, y0, rw, rh, out.ptr + off * es, rw if planar else 3 * rw, rw * rh)
             for (x0, y0, rw, rh), off in zip(rects, places)]
    arr = (capi.TensorItem * count)(*items)

    def call(s):
        capi.check(L.ffhip_bgra_to_tensor_items(arr, count, C.byref(f), s), "ffhip_bgra_to_tensor_items")

    def expect(which):
        buf, px = np.full(total, FILL, np.uint8), pick(which, true, decoy)
        for (x0, y0, rw, rh), off in zip(rects, places):
            e = SO.as_bytes(expected(px[y0:y0 + rh, x0:x0 + rw], f))
            buf[off * es:off * es + e.size] = e
        return [buf]
    return Case(f"bgra_to_tensor_items d{dtype} n{count}", call, [src], [out], expect, keep=f)


@pytest.mark.parametrize("filt", [BIL, AA])
def test_bgra_resize_items(stall, stream, filt):
    run_case(resize_case(filt), stall, stream)


def test_bgra_orient_items(stall, stream):
    run_case(orient_case(), stall, stream)


@pytest.mark.parametrize("dtype,planar", [(F16, 1), (U8, 0)])
def test_bgra_to_tensor_items(stall, stream, dtype, planar):
    run_case(tensor_case(dtype, planar), stall, stream)


# ---------------------------------------------------------------------------------------------------- HEIF
def heif_case():
    """ffhip_heif_grid_compose, 2 x 3 tiles of 64 x 32 into 180 x 50; stream-ordered: the tiles"""
    L = capi.lib()
    rows, cols, tw, th, ow, oh = 2, 3, 64, 32, 180, 50
    true = np.random.default_rng(830).integers(0, 256, (rows * cols, th, tw, 4), dtype=np.uint8)
    decoy = np.random.default_rng(930).integers(0, 256, (rows * cols, th, tw, 4), dtype=np.uint8)
    tiles = Operand(true, decoy)
    out = Output(ow * oh * 4)

    def call(s):
        capi.check(L.ffhip_heif_grid_compose(out.ptr, ow * 4, ow, oh, tiles.ptr, tw * 4, tw * th * 4, tw, th, rows, cols, s), "ffhip_heif_grid_compose")

    def expect(which):
        return [expected_canvas(pick(which, true, decoy), cols, ow, oh)]
    return Case("heif_grid_compose", call, [tiles], [out], expect)


def test_heif_grid_compose(stall, stream):
    run_case(heif_case(), stall, stream)


# ---------------------------------------------------------------------------------------------------- two items calls back to back
ITEMS_ENTRIES = {
    "jpeg_recon_items": lambda count, seed: jpeg_items_case(f"jpeg_recon_items n{count}", [JPEG_SMALL[(k + seed) % 4] for k in range(count)], None, seed, many=True),
    "jpeg_recon_items_scaled": lambda count, seed: jpeg_items_case(f"jpeg_recon_items_scaled n{count}", [JPEG_SMALL[(k + seed) % 4] for k in range(count)], 4, seed, many=True),
    "jpeg_recon_items_libjpeg": lambda count, seed: jpeg_items_libjpeg_case(f"jpeg_recon_items_libjpeg n{count}", [JPEG_SMALL[(k + seed) % 4] for k in range(count)], seed),
    "bgra_resize_items": lambda count, seed: resize_case(AA, count, seed),
    "bgra_orient_items": lambda count, seed: orient_case(count, seed),
    "bgra_to_tensor_items": lambda count, seed: tensor_case(F16, 1, count, seed),
}


@pytest.mark.parametrize("grow", [False, True], ids=["other_items", "scratch_grows"])
@pytest.mark.parametrize("entry", list(ITEMS_ENTRIES))
def test_two_items_calls_on_one_stalled_stream(stall, stream, entry, grow):
    """Two calls of one items entry behind one stall.  The second call refills the pinned descriptor staging the first call's upload is
    still queued from: it has to wait for that upload (the `staged` event), so the pending assertion comes behind the FIRST call only.
    grow: the second call has many more items than anything the stream has seen -- its scratch is reallocated while the stream holds work."""
    first = ITEMS_ENTRIES[entry](3, 0)
    second = ITEMS_ENTRIES[entry](400 if grow else 4, 1)
    SO.warm_up(stream, first.call, first.operands, first.outputs)
    if not grow:
        SO.warm_up(stream, second.call, second.operands, second.outputs)
    with SO.Scenario(f"{entry} x2{' grow' if grow else ''}", stall, stream, K) as sc:
        sc.produce(first.operands + second.operands)
        first.call(stream)
        sc.consume(first.outputs)
        sc.still_stalled()
        second.call(stream)
        sc.consume(second.outputs)
        sc.overwrite(first.operands + second.operands)
    assert sc.finish() == 0
    assert_outputs(first, "true")
    assert_outputs(second, "true")


# ---------------------------------------------------------------------------------------------------- chains
def hevc_chain_picture(seed):
    """levels -> four ffhip_hevc_residual_batch calls (one per TU size, into one residual buffer) -> ffhip_hevc_intra_recon_tiles ->
    ffhip_yuv420_to_bgra_16 for one 192 x 128 picture, as test_heic_chain_levels_to_bgra lays it out; stream-ordered: levels and TU info
    of every size; the residual buffer and the planes are the caller's intermediates"""
    L = capi.lib()
    w, h, bd = 192, 128, 8
    tus, _ = hevc_list(w, h, seed)
    tus = np.ascontiguousarray(tus).copy()
    tus["flags"] &= ~np.uint8(synth.TU_RDPCM)
    groups, off = {}, 0
    for n in (4, 8, 16, 32):                                        # the TUs of one size side by side in the residual buffer
        idx = np.flatnonzero(tus["log2_size"] == int(np.log2(n)))
        tus["res_offset"][idx] = off + np.arange(len(idx)) * n * n
        groups[n] = (idx, off)
        off += len(idx) * n * n
    d_tus = ops.DeviceBuffer(host=tus.view(np.uint8))
    d_res = ops.DeviceBuffer(nbytes=off * 2 + 32)
    tf = np.zeros(1, np.int64)
    inputs, operands = {}, []
    for n, (idx, _) in groups.items():
        def make(sd, n=n, idx=idx):
            rng = np.random.default_rng(sd)
            lv = np.rint(rng.laplace(0, 6, size=(len(idx), n * n))).astype(np.int16)
            info = np.zeros((len(idx), 4), np.uint8)
            info[:, 0] = rng.integers(20, 38, size=len(idx))
            if n == 4:
                info[tus["cidx"][idx] == 0, 1] = 1                  # luma intra 4x4: DST-VII
            return lv, info
        if len(idx):
            true, decoy = make(seed * 10 + n), make(seed * 10 + n + 1)
            devs = [Operand(t, d) for t, d in zip(true, decoy)]
            operands += devs
            inputs[n] = (true, devs)
    planes, memsets = hevc_planes(w, h)
    bgra = Output(w * h * 4)

    def call(s):
        for n, ((lv, _), devs) in inputs.items():
            capi.check(L.ffhip_hevc_residual_batch(n, len(lv), devs[0].ptr, devs[1].ptr, None, bd, 0, d_res.ptr + groups[n][1] * 2, s), "ffhip_hevc_residual_batch")
        capi.check(L.ffhip_hevc_intra_recon_tiles(tus.ctypes.data, d_tus.ptr, len(tus), tf.ctypes.data, 1, d_res.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr,
                                                  w, h, w, w // 2, h // 2, w // 2, bd, bd, s), "ffhip_hevc_intra_recon_tiles")
        capi.check(L.ffhip_yuv420_to_bgra_16(bgra.ptr, w * 4, planes[0].ptr, planes[1].ptr, planes[2].ptr, w, w // 2, h // 64, w // 64, 64, 1, 0, 0, 0, s),
                   "ffhip_yuv420_to_bgra_16")

    def expect(which):
        assert which == "true"
        res = np.zeros(off + 16, np.int16)
        for n, ((lv, info), _) in inputs.items():
            res[groups[n][1]:groups[n][1] + lv.size] = oracle_tus(n, lv, info, bd, 0, None).reshape(-1)
        y, u, v = O.oracle_hevc_intra(tus, res, w, h, True, bd, bd)
        return [oracle_420_16(y, u, v, h // 64, w // 64, 64)]
    return Case(f"hevc chain {seed}", call, operands, [bgra], expect, memsets, keep=(tus, d_tus, d_res, tf, planes))


def test_hevc_chain_twice_behind_one_stall(stall, stream):
    pics = [hevc_chain_picture(61), hevc_chain_picture(63)]
    for p in pics:
        SO.warm_up(stream, p.call, p.operands, p.outputs, p.memsets)
    with SO.Scenario("hevc chain x2", stall, stream, K) as sc:
        for p in pics:
            sc.produce(p.operands, p.memsets)
            p.call(stream)
            sc.consume(p.outputs)
        sc.overwrite(pics[0].operands + pics[1].operands)
        sc.still_stalled()
    assert sc.finish() == 0
    for p in pics:
        assert_outputs(p, "true")


def test_jpeg_chain_behind_one_stall(stall, stream):
    """ffhip_jpeg_recon_items -> ffhip_bgra_resize_items -> ffhip_bgra_orient_items -> ffhip_bgra_to_tensor_items, the intermediates the
    caller's own; stream-ordered: coefficient planes and quantiser tables"""
    L = capi.lib()
    mc, mr = 5, 4
    geom = capi.jpeg_geom(mc, mr)
    W, H, ow, oh = geom.width, geom.height, 33, 21
    q, qd = synth.quant_tables(), synth.quant_tables(quality=50)
    true, decoy = synth.coef_batch(1, mc, mr), synth.coef_batch(1, mc, mr, first=9)
    devs, dq = [Operand(t, d) for t, d in zip(true, decoy)], Operand(q, qd)
    full, small, turned = ops.DeviceBuffer(nbytes=W * H * 4), ops.DeviceBuffer(nbytes=ow * oh * 4), ops.DeviceBuffer(nbytes=ow * oh * 4)
    f = make_format(F16, 1, 0)
    out = Output(3 * ow * oh * 2)
    it = capi.JpegItem()
    it.geom = geom
    it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, it.d_bgra, it.pitch = devs[0].ptr, devs[1].ptr, devs[2].ptr, dq.ptr, full.ptr, W * 4
    ji = (capi.JpegItem * 1)(it)
    ri = (capi.ResizeItem * 1)(capi.ResizeItem(full.ptr, W * 4, 0, 0, W, H, small.ptr, ow * 4, ow, oh))
    oi = (capi.OrientItem * 1)(capi.OrientItem(small.ptr, ow * 4, 0, 0, ow, oh, turned.ptr, oh * 4, 6))
    ti = (capi.TensorItem * 1)(capi.TensorItem(turned.ptr, oh * 4, 0, 0, oh, ow, out.ptr, oh, oh * ow))

    def call(s):
        capi.check(L.ffhip_jpeg_recon_items(ji, 1, s), "ffhip_jpeg_recon_items")
        capi.check(L.ffhip_bgra_resize_items(ri, 1, AA, s), "ffhip_bgra_resize_items")
        capi.check(L.ffhip_bgra_orient_items(oi, 1, s), "ffhip_bgra_orient_items")
        capi.check(L.ffhip_bgra_to_tensor_items(ti, 1, C.byref(f), s), "ffhip_bgra_to_tensor_items")

    def expect(which):
        px = O.oracle_jpeg_recon(O.make_geom(mc, mr), *pick(which, true, decoy), pick(which, q, qd), n_images=1).reshape(H, W, 4)
        return [expected(X.orient(resize_rule(px, oh, ow, AA), 6), f)]
    run_case(Case("jpeg chain", call, devs + [dq], [out], expect), stall, stream)


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_resize_under_a_torch_stream(stall):
    """tensors.resize_bgra on torch's current stream, a torch copy as producer and torch.empty_like(...).copy_() as consumer"""
    import torch
    capi.require_device(0)
    (h, w), (oh, ow) = RESIZE_SHAPES[0]
    true, decoy = pixels(840, h, w), pixels(940, h, w)
    dev = torch.device("cuda", 0)
    t_true, t_decoy = torch.from_numpy(true).to(dev), torch.from_numpy(decoy).to(dev)
    t_in, t_out = t_decoy.clone(), torch.full((oh, ow, 4), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()                                                   # (the streams below do not wait for the default stream)
    item = [capi.ResizeItem(t_in.data_ptr(), 4 * w, 0, 0, w, h, t_out.data_ptr(), 4 * ow, ow, oh)]
    ts = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(ts):
        s = torch.cuda.current_stream().cuda_stream
        tensors.resize_bgra(item, antialias=True, stream=s)                    # warm-up: scratch, and the allocator's block for the copy
        del_me = torch.empty_like(t_out).copy_(t_out)
        ts.synchronize()
        del del_me
        t_out.fill_(FILL)
        ts.synchronize()
        marker = torch.cuda.Event()
        stall.enqueue(s, K)
        marker.record(ts)
        t_in.copy_(t_true, non_blocking=True)
        tensors.resize_bgra(item, antialias=True, stream=s)
        t_copy = torch.empty_like(t_out).copy_(t_out, non_blocking=True)
        t_in.copy_(t_decoy, non_blocking=True)
        assert not marker.query(), "inconclusive: the stall had finished before the last enqueue returned"
        ts.synchronize()
    assert capi.sync(s) == 0
    assert np.array_equal(t_copy.cpu().numpy(), resize_rule(true, oh, ow, AA))


# ---------------------------------------------------------------------------------------------------- negative controls
CONTROLS = {
    "jpeg": lambda: jpeg_items_case("jpeg_recon_items", JPEG_SPECS),
    "colour": lambda: colour_case(8),
    "hevc_residual": lambda: hevc_residual_case(4, 777),
    "hevc_intra": lambda: hevc_intra_case(192, 128, 71),
    "vp8": vp8_predict_case,
    "items": lambda: resize_case(AA),
    "heif": heif_case,
}


@pytest.mark.parametrize("family", list(CONTROLS))
def test_control_a_caller_that_breaks_the_contract_gets_the_decoy(stall, two_streams, family):
    """The contract broken on the CALLER's side -- the producer on another stream, behind that stream's stall; the call on a stream that
    does not wait for it -- gives the decoy's output: the decoy differs from the input, the stall outlasts the call, the scenario can
    tell the two apart."""
    case = CONTROLS[family]()
    assert any(not np.array_equal(SO.as_bytes(t), SO.as_bytes(d)) for t, d in zip(case.expect("true"), case.expect("decoy")))
    run_control(case, stall, two_streams)


# ---------------------------------------------------------------------------------------------------- the stall's length
def test_stall_is_long_enough(stall):
    """One 256 MiB copy is measured again with ffhip_event_elapsed_ms, on a stream of its own: K of them must last at least four times
    HOST_MS_MAX, the longest enqueue sequence measured (module docstring), and under half a second.  The host times of the enqueue
    sequences this session has run so far are printed next to it -- the table of DESIGN.md 4.15 comes from that line -- and nothing is
    asserted of them: a case whose host was held up for longer than its stall has failed its own pending assertion."""
    L = capi.require_device(0)
    s = L.ffhip_stream_create()
    assert s
    ms = stall.copy_ms(s)
    assert capi.sync(s) == 0
    L.ffhip_stream_destroy(s)
    host = {k: v * 1e3 for k, v in SO.HOST_SECONDS.items() if not k.endswith("/broken")}
    print(f"\nstream order: one 256 MiB copy {ms:.4f} ms; K = {K}: stall {K * ms:.2f} ms; enqueue sequences, ms of host time: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(host.items(), key=lambda kv: -kv[1])))
    assert K * max(ms, COPY_MS) < 500.0, (K, ms, COPY_MS)
    assert K * ms >= 4.0 * HOST_MS_MAX, (K, ms, HOST_MS_MAX)
