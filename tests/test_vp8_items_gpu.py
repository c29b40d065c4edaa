"""GPU: ffhip_vp8_decode_items -- key frames of mixed sizes, quantisers and loop filters in one call, against the reference's
whole-file decodes and against ffhip_vp8_residual_batch + ffhip_vp8_decode_frames(n = 1) on each frame alone, with every byte
outside each frame's picture (the pitch's padding included) checked untouched."""
import ctypes as C
import threading

import numpy as np
import pytest

from ffpic_amd import capi, ops, synth
from test_oracle_golden import vp8_filter_header

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def filters_of(lf, hdr):
    filt = np.zeros((4, 2, 3), np.uint8)
    ft = C.c_int(-1)
    capi.check(capi.lib().ffhip_vp8_filter_params(C.byref(vp8_filter_header(lf, hdr)), filt.ctypes.data, C.byref(ft)))
    return ft.value, filt


class Frame:
    """one item: its inputs in device memory, its sentinel-filled output (16 * r rows of `pitch` bytes)"""

    def __init__(self, c, r, modes, ft, filt, residual=None, levels=None, info=None, quant=None, resmap=None, host_modes=True,
                 pitch=None):
        self.c, self.r, self.ft = c, r, ft
        self.modes = np.ascontiguousarray(modes, np.uint8).reshape(c * r, 20)
        self.filt = np.zeros((4, 2, 3), np.uint8) if filt is None else np.ascontiguousarray(filt, np.uint8).reshape(4, 2, 3)
        self.residual, self.levels, self.info, self.resmap, self.host_modes = residual, levels, info, resmap, host_modes
        self.quant = None if quant is None else np.ascontiguousarray(quant, np.uint16)
        self.dm = ops.DeviceBuffer(self.modes)
        self.dr = ops.DeviceBuffer(np.ascontiguousarray(residual)) if residual is not None else None
        self.dl = ops.DeviceBuffer(np.ascontiguousarray(levels)) if levels is not None else None
        self.di = ops.DeviceBuffer(np.ascontiguousarray(info)) if info is not None else None
        self.dmap = ops.DeviceBuffer(np.ascontiguousarray(resmap, np.int32)) if resmap is not None else None
        self.pitch = pitch or 64 * c
        self.H = 16 * r
        self.do = ops.DeviceBuffer(nbytes=self.H * self.pitch)
        self.reset()

    def reset(self, stream=None):
        capi.check(capi.lib().ffhip_memset(self.do.ptr, SENTINEL, self.do.nbytes, stream))

    def item(self):
        it = capi.Vp8Item()
        it.mbcols, it.mbrows = self.c, self.r
        it.h_modes = self.modes.ctypes.data if self.host_modes else None
        it.d_modes = self.dm.ptr
        if self.dl is not None:
            it.d_levels, it.d_mbinfo = self.dl.ptr, self.di.ptr
            for s in range(4):
                for k in range(8):
                    it.quant[s][k] = int(self.quant[s, k])
        else:
            it.d_residual = self.dr.ptr
        it.d_resmap = self.dmap.ptr if self.dmap is not None else None
        it.filter_type = self.ft
        for k, v in enumerate(self.filt.reshape(-1)):
            it.filters[k] = int(v)
        it.d_bgra, it.pitch = self.do.ptr, self.pitch
        return it

    def out(self, stream=None):
        o = np.empty((self.H, self.pitch), np.uint8)
        L = capi.lib()
        capi.check(L.ffhip_memcpy_d2h(o.ctypes.data, self.do.ptr, o.nbytes, stream))
        capi.check(L.ffhip_stream_sync(stream))
        return o

    def alone(self):
        """the same frame through ffhip_vp8_residual_batch + ffhip_vp8_decode_frames(n = 1)"""
        res = self.residual if self.levels is None else ops.vp8_residual_batch(self.levels, self.info, self.quant)
        bgra = ops.vp8_decode_frames(self.c, self.r, self.modes[None], res[None], self.ft, self.filt if self.ft else None,
                                     resmap=None if self.resmap is None else self.resmap[None], pitch=self.pitch)
        return bgra[0]


def run(frames, stream=None):
    for f in frames:
        f.reset(stream)
    ops.vp8_decode_items([f.item() for f in frames], stream)
    capi.sync(stream)


def check_against(f, exp):
    got = f.out()
    w = 64 * f.c
    assert np.array_equal(got[:, :w], exp[:, :w]), np.argwhere(got[:, :w] != exp[:, :w])[:4]
    assert (got[:, w:] == SENTINEL).all(), "the pitch's padding was written"


# ---- 1. real files in one call ----

def _golden_frames(golden):
    out = []
    g = golden("webp_file.npz")                             # q100, loop filter off
    w, h, pitch = [int(x) for x in g["dims"]]
    c, r = (w + 15) // 16, (h + 15) // 16
    out.append((Frame(c, r, g["modes"], 0, None, residual=g["residual"], pitch=pitch), h, g["bgra"]))
    g = golden("webp_file_lf.npz")
    for tag in ("q55", "q40"):                              # normal filter, levels 15 / 19
        w, h, pitch = [int(x) for x in g[f"{tag}_dims"]]
        c, r = (w + 15) // 16, (h + 15) // 16
        ft, filt = filters_of(g[f"{tag}_lf"], g[f"{tag}_lf_header"])
        out.append((Frame(c, r, g[f"{tag}_modes"], ft, filt, residual=g[f"{tag}_residual"], pitch=pitch), h, g[f"{tag}_bgra"]))
    return out


def _frame_1080p(golden, host_modes=True):
    g = golden("webp_file_1080p.npz")                        # a real encoder's stream, level 40
    w, h, pitch = [int(x) for x in g["dims"]]
    c, r = (w + 15) // 16, (h + 15) // 16
    ft, filt = filters_of(g["lf"], g["lf_header"])
    return Frame(c, r, g["modes"], ft, filt, residual=g["residual"], pitch=pitch, host_modes=host_modes), h, g


def _is_reference_decode_1080p(g, bgra, h):
    assert np.array_equal(bgra[:32], g["bgra_head"])
    rows = np.ascontiguousarray(bgra[:h]).reshape(h, -1).view(np.uint32).astype(np.uint64)
    sums = (rows * (np.arange(rows.shape[1], dtype=np.uint64) + np.uint64(1))).sum(axis=1, dtype=np.uint64)
    assert (sums == g["bgra_row_sums"]).all()


@pytest.mark.parametrize("order", ["forward", "reverse", "1080p x 8 between"])
def test_real_files_in_one_call(golden, order):
    small = _golden_frames(golden)
    big = [_frame_1080p(golden, host_modes=(k % 2 == 0)) for k in range(8 if order == "1080p x 8 between" else 1)]
    if order == "forward":
        seq = small + big
    elif order == "reverse":
        seq = (small + big)[::-1]
    else:
        seq = small[:1] + big + small[1:]
    run([f for f, _, _ in seq])
    for f, h, exp in seq:
        got = f.out()
        if isinstance(exp, dict):
            _is_reference_decode_1080p(exp, got, h)
        else:
            assert np.array_equal(got[:h], exp)


# ---- 2. per-item quantisers against the reference ----

def test_per_item_quantisers_against_the_reference(golden):
    g = golden("vp8_residual_driven.npz")
    frames, exp = [], []
    for k, regime in enumerate(("random", "sparse", "dense")):
        modes = synth.vp8_modes(16, 16, seed=700 + k)
        ft, filt = k % 3, synth.vp8_filters(seed=700 + k)
        frames.append(Frame(16, 16, modes, ft, filt, levels=g[f"{regime}_levels"], info=g[f"{regime}_info"], quant=g[f"{regime}_quant"]))
        exp.append(ops.vp8_decode_frames(16, 16, modes[None], g[f"{regime}_residual"][None], ft, filt if ft else None)[0])
    run(frames)
    for f, e in zip(frames, exp):
        check_against(f, e)


# ---- 3. equivalence sweep ----

SIZES = [(1, 1), (1, 9), (9, 1), (240, 2), (2, 68), (120, 68), (1, 2), (2, 1), (3, 2), (5, 3), (17, 9), (40, 23), (7, 15), (20, 15)]


def _sweep_frames(n, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        c, r = SIZES[i] if i < len(SIZES) else (int(rng.integers(1, 24)), int(rng.integers(1, 18)))
        n_mb = c * r
        modes = synth.vp8_modes(c, r, seed=seed + i, bpred_share=0.9 if i % 4 == 0 else 0.4)
        modes[:, 18] = rng.integers(0, 4, size=n_mb)
        if i % 3 == 1:                       # rows that open with 16x16 H_PRED: the wrapped read at x = 0
            modes.reshape(r, c, 20)[1:, 0, 0] = 3
        resmap = np.maximum.accumulate(np.where(rng.random(n_mb) < 0.3, 0, np.arange(n_mb))).astype(np.int32) if i % 2 else None
        ft, filt = i % 3, synth.vp8_filters(seed=seed + i)
        pitch = 64 * c + (16 * int(rng.integers(0, 4)))
        host = i % 5 != 2
        if i % 4 < 2:
            lv, info = synth.vp8_macroblocks(n_mb, seed=seed + i)
            info[:, 26] = modes[:, 18]
            frames.append(Frame(c, r, modes, ft, filt, levels=lv, info=info, quant=synth.vp8_quant(seed=seed + i), resmap=resmap,
                                host_modes=host, pitch=pitch))
        else:
            frames.append(Frame(c, r, modes, ft, filt, residual=synth.vp8_residual(n_mb, seed=seed + i), resmap=resmap, host_modes=host,
                                pitch=pitch))
    return frames


def test_equivalence_sweep():
    frames = _sweep_frames(320, 5000)
    run(frames)
    for i, f in enumerate(frames):
        try:
            check_against(f, f.alone())
        except AssertionError as e:
            raise AssertionError(f"item {i}: {f.c}x{f.r} ft {f.ft} levels {f.levels is not None} map {f.resmap is not None}: {e}")


# ---- 4. refusal ----

def test_bad_device_modes_refuse_at_the_sync_and_write_nothing():
    L = capi.require_device()
    frames = _sweep_frames(12, 6000)
    bad = frames[7]
    bad.host_modes = False
    m = bad.modes.copy()
    m[-1, 0] = 9
    bad.dm = ops.DeviceBuffer(m)
    for f in frames:
        f.reset()
    arr = (capi.Vp8Item * len(frames))(*[f.item() for f in frames])
    assert L.ffhip_vp8_decode_items(arr, len(frames), None) == 0
    assert L.ffhip_stream_sync(None) == capi.FFHIP_EINVAL
    for f in frames:
        assert (f.out() == SENTINEL).all()
    assert L.ffhip_stream_sync(None) == 0


def test_device_check_agrees_with_host_check():
    """One 1x1-macroblock item per record of a table (positions 0..17; per position the limit, limit + 1, 0x0f, 0x10, 0x7f, 0x80, 0xff; each
    once in a B_PRED record and once in a DC record), filter_type 0, the residual form: with h_modes the host check refuses a bad record at
    the call, without it the device check refuses at the next ffhip_stream_sync, which says FFHIP_EINVAL exactly once.  Both are the numpy
    rule, case by case: the smallest shape at which the shared predicate, the merged check kernel and its refusal stores can go wrong."""
    L = capi.require_device()
    bases = [np.array([4, 1] + [(3 * k + 1) % 10 for k in range(16)] + [0, 0], np.uint8), np.array([0, 2] + [(3 * k + 1) % 10 for k in range(16)] + [0, 0], np.uint8)]
    recs = []
    for p in range(18):
        lim = 4 if p == 0 else (3 if p == 1 else 9)
        for v in (lim, lim + 1, 0x0f, 0x10, 0x7f, 0x80, 0xff):
            for b in bases:
                rec = b.copy()
                rec[p] = v
                recs.append(rec)
    recs = np.stack(recs)
    want = (recs[:, 0] <= 4) & (recs[:, 1] <= 3) & ((recs[:, 0] != 4) | (recs[:, 2:18] <= 9).all(axis=1))
    assert len(recs) == 252 and want.sum() not in (0, len(want))
    f = Frame(1, 1, recs[0][None].copy(), 0, None, residual=synth.vp8_residual(1, seed=77))
    for rec, ok in zip(recs, want):
        f.modes[0] = rec
        capi.check(L.ffhip_memcpy_h2d(f.dm.ptr, f.modes.ctypes.data, 20, None))
        for host in (True, False):
            f.host_modes = host
            arr = (capi.Vp8Item * 1)(f.item())
            rc = L.ffhip_vp8_decode_items(arr, 1, None)
            first, second = L.ffhip_stream_sync(None), L.ffhip_stream_sync(None)
            exp = (0, 0, 0) if ok else ((capi.FFHIP_EINVAL, 0, 0) if host else (0, capi.FFHIP_EINVAL, 0))
            assert (rc, first, second) == exp, (rec, host)


def test_bad_host_modes_refuse_the_call_with_nothing_enqueued():
    L = capi.require_device()
    frames = _sweep_frames(6, 6100)
    frames[3].modes[0, 1] = 7
    for f in frames:
        f.reset()
    arr = (capi.Vp8Item * len(frames))(*[f.item() for f in frames])
    assert L.ffhip_vp8_decode_items(arr, len(frames), None) == capi.FFHIP_EINVAL
    assert L.ffhip_stream_sync(None) == 0
    for f in frames:
        assert (f.out() == SENTINEL).all()


def _compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("host_modes", [True, False])
def test_several_frames_per_workgroup(host_modes):
    """ONE launch (normal filter, no residual map) of more than 8 frames per compute unit.  The grid is at most 4 workgroups per CU
    (four waves per workgroup, four waves per SIMD), so every workgroup's share holds at least two frames: progress bases that do
    not start at 0, the waves' walk over the share's slots, filter parameters refilled when a wave moves to the next frame, line
    slots reused by frames of different widths, and frames narrower and shorter than the wave count (several in flight in one
    workgroup).  With host copies the call may pick four waves per workgroup (rows that open with H_PRED), without them eight."""
    n = 8 * _compute_units() + 37
    rng = np.random.default_rng(11 if host_modes else 12)
    frames = []
    for i in range(n):
        c, r = (int(rng.integers(1, 5)), int(rng.integers(1, 5))) if i % 97 else [(40, 3), (120, 2), (9, 7), (2, 30)][(i // 97) % 4]
        modes = synth.vp8_modes(c, r, seed=20000 + i, bpred_share=0.6)
        modes[:, 18] = rng.integers(0, 4, size=c * r)
        if i % 3 == 0 and r > 1:
            modes.reshape(r, c, 20)[1:, 0, 0] = 3            # rows that wait for the whole row above
        pitch = 64 * c + 16 * int(rng.integers(0, 3))
        if i % 2:
            lv, info = synth.vp8_macroblocks(c * r, seed=20000 + i)
            info[:, 26] = modes[:, 18]
            frames.append(Frame(c, r, modes, 2, synth.vp8_filters(seed=20000 + i), levels=lv, info=info, quant=synth.vp8_quant(seed=i),
                                host_modes=host_modes, pitch=pitch))
        else:
            frames.append(Frame(c, r, modes, 2, synth.vp8_filters(seed=20000 + i), residual=synth.vp8_residual(c * r, seed=20000 + i),
                                host_modes=host_modes, pitch=pitch))
    run(frames)
    for i, f in enumerate(frames):
        try:
            check_against(f, f.alone())
        except AssertionError as e:
            raise AssertionError(f"item {i}: {f.c}x{f.r}: {e}")


# ---- 5. concurrency ----

def test_two_threads_two_streams():
    L = capi.require_device()
    sets = [_sweep_frames(24, 8000), _sweep_frames(24, 9000)]
    exp = []
    for fr in sets:
        run(fr)
        exp.append([f.out() for f in fr])
    errors = []

    def worker(k):
        st = L.ffhip_stream_create()
        try:
            for _ in range(4):
                for f in sets[k]:
                    f.reset(st)
                ops.vp8_decode_items([f.item() for f in sets[k]], st)
                if L.ffhip_stream_sync(st) != 0:
                    errors.append((k, "sync"))
                    return
                for f, e in zip(sets[k], exp[k]):
                    if not np.array_equal(f.out(st), e):
                        errors.append((k, "bytes"))
                        return
        finally:
            L.ffhip_stream_destroy(st)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
