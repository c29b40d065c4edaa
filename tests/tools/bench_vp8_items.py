"""ffhip_vp8_decode_items against the calls a caller has without it; one JSON line.

  uniform   N copies of the real encoder's 1080p frame (tests/golden/webp_file_1080p.npz), residual form: one items call against one
            ffhip_vp8_decode_frames call on the same buffers (device events, warm-up, A/B alternating in one process)
  mixed     512 frames of six sizes from 320x240 to 1920x1088, filter types 0/1/2, a quantiser set per frame, levels form: one items
            call; one ffhip_vp8_residual_batch + ffhip_vp8_decode_frames call per frame (what a caller must do today); and, as a
            reference bar, one such pair per size (as if frames of a size shared quantisers and filters).  Under rocprofv3 --kernel-trace
            the items call's k_vp8_frames_items launches give its largest launch's kernel time (the cost of the other launches and of imbalance)
  levels    the residual stage: ffhip_vp8_residual_batch against the items call's levels form (k_vp8_residual against k_vp8_residual_items
            in a kernel trace)

  python tests/tools/bench_vp8_items.py [--uniform 256,1024] [--levels 256] [--no-mixed] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ffpic_amd import capi, ops, synth  # noqa: E402

L = capi.require_device()
ev0, ev1 = L.ffhip_event_create(), L.ffhip_event_create()


def timed(fn, reps):
    fn()
    capi.check(L.ffhip_stream_sync(None))
    out = []
    for _ in range(reps):
        L.ffhip_event_record(ev0, None)
        fn()
        L.ffhip_event_record(ev1, None)
        capi.check(L.ffhip_stream_sync(None))
        out.append(L.ffhip_event_elapsed_ms(ev0, ev1))
    return float(np.median(out))


def item(c, r, dm, hm, ft, filt, dbgra, pitch, dres=None, dlv=None, dinfo=None, quant=None):
    it = capi.Vp8Item()
    it.mbcols, it.mbrows, it.h_modes, it.d_modes = c, r, hm, dm
    if dres is not None:
        it.d_residual = dres
    else:
        it.d_levels, it.d_mbinfo = dlv, dinfo
        for s in range(4):
            for k in range(8):
                it.quant[s][k] = int(quant[s, k])
    it.filter_type = ft
    for k, v in enumerate(np.asarray(filt, np.uint8).reshape(-1)):
        it.filters[k] = int(v)
    it.d_bgra, it.pitch = dbgra, pitch
    return it


def uniform(n, reps):
    from test_oracle_golden import vp8_filter_header
    g = np.load(os.path.join(ROOT, "tests", "golden", "webp_file_1080p.npz"))
    w, h, _ = [int(x) for x in g["dims"]]
    c, r = (w + 15) // 16, (h + 15) // 16
    n_mb, pitch, H = c * r, 64 * c, 16 * r
    filt = np.zeros((4, 2, 3), np.uint8)
    ft = C.c_int(-1)
    capi.check(L.ffhip_vp8_filter_params(C.byref(vp8_filter_header(g["lf"], g["lf_header"])), filt.ctypes.data, C.byref(ft)))
    modes = np.ascontiguousarray(np.broadcast_to(g["modes"], (n,) + g["modes"].shape))
    dm, dr, df = ops.DeviceBuffer(modes), ops.DeviceBuffer(np.ascontiguousarray(g["residual"])), ops.DeviceBuffer(filt)
    do = ops.DeviceBuffer(nbytes=n * H * pitch)
    items = (capi.Vp8Item * n)(*[item(c, r, dm.ptr + i * n_mb * 20, None, ft.value, filt, do.ptr + i * H * pitch, pitch, dres=dr.ptr)
                                 for i in range(n)])
    a = lambda: capi.check(L.ffhip_vp8_decode_frames(c, r, n, None, dm.ptr, dr.ptr, 0, None, ft.value, df.ptr, do.ptr, pitch, H * pitch,
                                                     None, None, None, 0, 0, None))
    b = lambda: capi.check(L.ffhip_vp8_decode_items(items, n, None))
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    px = n * w * h
    return {"frames": n, "decode_frames_ms": ta, "items_ms": tb, "ratio_rate": float(np.median(ta) / np.median(tb)),
            "decode_frames_gpx_s": px / np.median(ta) / 1e6, "items_gpx_s": px / np.median(tb) / 1e6}


def mixed(reps):
    sizes = [(20, 15), (40, 30), (64, 48), (80, 45), (100, 75), (120, 68)]
    src = {}
    for k, (c, r) in enumerate(sizes):
        n_mb = c * r
        modes = synth.vp8_modes(c, r, seed=40 + k)
        lv, info = synth.vp8_macroblocks(n_mb, seed=40 + k)
        info[:, 26] = modes[:, 18] = np.random.default_rng(k).integers(0, 4, size=n_mb)
        src[(c, r)] = (modes, ops.DeviceBuffer(modes), ops.DeviceBuffer(lv), ops.DeviceBuffer(info))
    n = 512
    frames = []
    for i in range(n):
        c, r = sizes[i % len(sizes)]
        frames.append((c, r, i % 3, synth.vp8_filters(seed=i), synth.vp8_quant(seed=i)))
    outs = [ops.DeviceBuffer(nbytes=16 * r * 64 * c) for c, r, _, _, _ in frames]
    items = [item(c, r, src[(c, r)][1].ptr, src[(c, r)][0].ctypes.data, ft, filt, o.ptr, 64 * c, dlv=src[(c, r)][2].ptr,
                  dinfo=src[(c, r)][3].ptr, quant=q) for (c, r, ft, filt, q), o in zip(frames, outs)]
    arr = (capi.Vp8Item * n)(*items)
    max_mb = max(c * r for c, r in sizes)
    dres = ops.DeviceBuffer(nbytes=n * max_mb * 768)          # per frame its own residual, as a caller would keep it
    dq = [ops.DeviceBuffer(np.ascontiguousarray(q)) for _, _, _, _, q in frames]
    df = [ops.DeviceBuffer(np.ascontiguousarray(f)) for _, _, _, f, _ in frames]

    def per_frame():
        for i, (c, r, ft, _, _) in enumerate(frames):
            s = src[(c, r)]
            res = dres.ptr + i * max_mb * 768
            capi.check(L.ffhip_vp8_residual_batch(c * r, s[2].ptr, s[3].ptr, dq[i].ptr, res, None))
            capi.check(L.ffhip_vp8_decode_frames(c, r, 1, s[0].ctypes.data, s[1].ptr, res, 0, None, ft, df[i].ptr, outs[i].ptr, 64 * c, 0,
                                                 None, None, None, 0, 0, None))

    # one call pair per size: the frames of a size as one batch (their modes and levels repeated; the first frame's quantisers and filter)
    per_size = {}
    for k, (c, r) in enumerate(sizes):
        idx = [i for i in range(n) if i % len(sizes) == k]
        m = len(idx)
        modes = np.ascontiguousarray(np.broadcast_to(src[(c, r)][0], (m,) + src[(c, r)][0].shape))
        per_size[(c, r)] = (m, modes, ops.DeviceBuffer(modes), ops.DeviceBuffer(nbytes=m * c * r * 768),
                            ops.DeviceBuffer(nbytes=m * 16 * r * 64 * c), frames[idx[0]][2], df[idx[0]], dq[idx[0]])
    lv_rep = {}
    for (c, r), v in per_size.items():
        m = v[0]
        lv = np.asarray(synth.vp8_macroblocks(c * r, seed=40 + sizes.index((c, r)))[0])
        info = np.asarray(synth.vp8_macroblocks(c * r, seed=40 + sizes.index((c, r)))[1])
        lv_rep[(c, r)] = (ops.DeviceBuffer(np.ascontiguousarray(np.broadcast_to(lv, (m,) + lv.shape))),
                          ops.DeviceBuffer(np.ascontiguousarray(np.broadcast_to(info, (m,) + info.shape))))

    def one_per_size():
        for (c, r), (m, modes, dmm, dr, do, ft, dff, dqq) in per_size.items():
            capi.check(L.ffhip_vp8_residual_batch(m * c * r, lv_rep[(c, r)][0].ptr, lv_rep[(c, r)][1].ptr, dqq.ptr, dr.ptr, None))
            capi.check(L.ffhip_vp8_decode_frames(c, r, m, modes.ctypes.data, dmm.ptr, dr.ptr, c * r * 384, None, ft, dff.ptr, do.ptr, 64 * c,
                                                 16 * r * 64 * c, None, None, None, 0, 0, None))

    fn_items = lambda: capi.check(L.ffhip_vp8_decode_items(arr, n, None))
    t = {"items": [], "per_frame": [], "per_size": []}
    for _ in range(3):
        t["items"].append(timed(fn_items, reps))
        t["per_frame"].append(timed(per_frame, 1))
        t["per_size"].append(timed(one_per_size, reps))
    px = sum(256 * c * r for c, r, _, _, _ in frames)
    return {"frames": n, "sizes": sizes, "mpixels": px / 1e6, "ms": t,
            "gpx_s": {k: px / float(np.median(v)) / 1e6 for k, v in t.items()}}


def levels(n, reps):
    """the residual stage alone on n 1080p-sized frames of synthetic levels: ffhip_vp8_residual_batch over all of them against the
    items call in the levels form (filter off); run under rocprofv3 --kernel-trace, k_vp8_residual against k_vp8_residual_items"""
    c, r = 120, 68
    n_mb = c * r
    lv, info = synth.vp8_macroblocks(n_mb, seed=77)
    q = synth.vp8_quant(seed=77)
    modes = synth.vp8_modes(c, r, seed=77)
    dl = ops.DeviceBuffer(np.ascontiguousarray(np.broadcast_to(lv, (n,) + lv.shape)))
    di = ops.DeviceBuffer(np.ascontiguousarray(np.broadcast_to(info, (n,) + info.shape)))
    dq, dm = ops.DeviceBuffer(q), ops.DeviceBuffer(modes)
    dr = ops.DeviceBuffer(nbytes=n * n_mb * 768)
    do = ops.DeviceBuffer(nbytes=n * 16 * r * 64 * c)
    items = (capi.Vp8Item * n)(*[item(c, r, dm.ptr, modes.ctypes.data, 0, np.zeros(24, np.uint8), do.ptr + i * 16 * r * 64 * c, 64 * c,
                                      dlv=dl.ptr + i * n_mb * 800, dinfo=di.ptr + i * n_mb * 32, quant=q) for i in range(n)])
    a = lambda: capi.check(L.ffhip_vp8_residual_batch(n * n_mb, dl.ptr, di.ptr, dq.ptr, dr.ptr, None))
    b = lambda: capi.check(L.ffhip_vp8_decode_items(items, n, None))
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    return {"frames": n, "residual_batch_ms": ta, "items_levels_form_ms": tb}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--uniform", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", default="")
    ap.add_argument("--no-mixed", action="store_true")
    a = ap.parse_args()
    res = {"uniform": [uniform(int(x), a.reps) for x in a.uniform.split(",") if x]}
    res["levels"] = [levels(int(x), a.reps) for x in a.levels.split(",") if x]
    if not a.no_mixed:
        res["mixed"] = mixed(a.reps)
    print(json.dumps(res))
