#!/usr/bin/env python3
"""Mixed batches (ffhip_jpeg_recon_items, ffhip_jpeg_decode_files_mixed_device); prints one JSON line.
  items:  ffhip_jpeg_recon_items against ffhip_jpeg_recon_batch on the same 256 x 3840x2160 4:2:0 buffers, ms per call by HIP events
  files:  1 024 seeded files of ten sizes (320x240 .. 3840x2160, some odd) in 4:2:0, 4:4:4, 4:2:2 and grey, half with restart markers:
          ONE mixed call against what a caller can do without it -- group by exact geometry, one ffhip_jpeg_decode_files_device call
          per group on the same stream -- wall time of the whole batch, best of --reps
--part items|files|all (default all).  Needs PIL and torch."""
import argparse, ctypes as C, io, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from ffpic_amd import capi, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["items", "files", "all"])
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
L = capi.require_device(0)
import torch
out = {"tool": "bench_mixed_files"}


def items_part():
    n, mc, mr = 256, 240, 135
    geom = capi.jpeg_geom(mc, mr)
    cy, cu, cv = synth.coef_batch(4, mc, mr)
    dy = torch.from_numpy(cy).cuda().repeat(n // 4)
    du = torch.from_numpy(cu).cuda().repeat(n // 4)
    dv = torch.from_numpy(cv).cuda().repeat(n // 4)
    dq = torch.from_numpy(np.tile(synth.quant_tables().reshape(-1), n).astype(np.int16)).cuda()
    pitch = geom.width * 4 + 1024
    stride = pitch * geom.height
    dout = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    yb, cb = geom.y_blocks * 128, geom.c_blocks * 128
    arr = (capi.JpegItem * n)()
    for i in range(n):
        it = arr[i]
        it.geom = geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v = dy.data_ptr() + i * yb, du.data_ptr() + i * cb, dv.data_ptr() + i * cb
        it.d_quant, it.d_bgra, it.pitch = dq.data_ptr() + i * 512, dout.data_ptr() + i * stride, pitch
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()

    def batch():
        capi.check(L.ffhip_jpeg_recon_batch(C.byref(geom), n, dy.data_ptr(), du.data_ptr(), dv.data_ptr(), dq.data_ptr(), 256, dout.data_ptr(),
                                            pitch, stride, None, 0, st))

    def items():
        capi.check(L.ffhip_jpeg_recon_items(arr, n, st))

    def timed(f, k=10):
        L.ffhip_event_record(e0, st)
        for _ in range(k):
            f()
        L.ffhip_event_record(e1, st)
        capi.check(L.ffhip_stream_sync(st))
        return L.ffhip_event_elapsed_ms(e0, e1) / k

    for f in (batch, items):
        timed(f, 3)
    res = {"batch": [], "items": []}
    for _ in range(args.reps):        # interleaved: the same placement and clocks for both
        res["batch"].append(timed(batch))
        res["items"].append(timed(items))
    b, i = float(np.median(res["batch"])), float(np.median(res["items"]))
    px = n * geom.width * geom.height
    out["items_vs_batch_4k420x256"] = {"batch_ms": round(b, 3), "items_ms": round(i, 3), "items_over_batch": round(i / b, 4),
                                       "batch_Gpx_s": round(px / b / 1e6, 1), "items_Gpx_s": round(px / i / 1e6, 1),
                                       "batch_all_ms": [round(x, 3) for x in res["batch"]], "items_all_ms": [round(x, 3) for x in res["items"]]}
    L.ffhip_event_destroy(e0); L.ffhip_event_destroy(e1)


def files_part():
    from PIL import Image
    rng = np.random.default_rng(2024)
    sizes = [(320, 240), (333, 251), (640, 480), (801, 599), (1024, 768), (1280, 720), (1919, 1081), (2048, 1152), (2560, 1440), (3840, 2160)]
    kinds = [("RGB", 2), ("RGB", 0), ("RGB", 1), ("L", None)]
    protos = {}
    for si, (w, h) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / 37.0) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / 53.0), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        for ki, (mode, sub) in enumerate(kinds):
            for dri in (0, 1):
                bio = io.BytesIO()
                kw = dict(quality=85)
                if sub is not None:
                    kw["subsampling"] = sub
                if dri:
                    kw["restart_marker_rows"] = 1
                Image.fromarray(img).convert(mode).save(bio, "JPEG", **kw)
                protos[(si, ki, dri)] = bio.getvalue()
    keys = list(protos)
    pick = [keys[int(k)] for k in rng.integers(0, len(keys), 1024)]
    files = [protos[k] for k in pick]
    n = len(files)
    probes = [ops.jpeg_probe(f) for f in files]
    offs, pitches, total = [], [], 0
    for g, _, _ in probes:
        offs.append(total); pitches.append(g.width * 4)
        total += (g.width * 4 * g.height + 255) & ~255
    dout = torch.empty(total, dtype=torch.uint8, device="cuda")
    base = dout.data_ptr()
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    outs = (C.c_void_p * n)(*[base + o for o in offs])
    pa = (C.c_int64 * n)(*pitches)
    geoms = (capi.JpegGeom * n)()
    status = (C.c_int * n)()
    st = torch.cuda.current_stream().cuda_stream

    def mixed():
        capi.check(L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n, 16, outs, pa, geoms, status, st))

    groups = {}
    for i, k in enumerate(pick):
        groups.setdefault(k[:2], []).append(i)   # exact geometry: size and layout (a file with or without markers has the same geometry)
    gcalls = []
    for idx in groups.values():
        # the group's pictures placed one behind the other at image_stride = pitch x height: a separate allocation per group, as such a caller has
        g = probes[idx[0]][0]
        m = len(idx)
        buf = torch.empty(m * g.width * 4 * g.height, dtype=torch.uint8, device="cuda")
        gp = (C.c_void_p * m)(*[ptrs[i] for i in idx])
        gl = (C.c_size_t * m)(*[lens[i] for i in idx])
        gs = (C.c_int * m)()
        gcalls.append((gp, gl, m, buf, g.width * 4, g.width * 4 * g.height, gs))

    def grouped():
        for gp, gl, m, buf, p, s, gs in gcalls:
            g2 = capi.JpegGeom()
            capi.check(L.ffhip_jpeg_decode_files_device(gp, gl, m, 16, C.byref(g2), buf.data_ptr(), p, s, gs, st))

    def wall(f):
        capi.check(L.ffhip_stream_sync(st))
        t0 = time.perf_counter(); f(); capi.check(L.ffhip_stream_sync(st))
        return (time.perf_counter() - t0) * 1e3

    mixed(); grouped()
    tm, tg = [], []
    for _ in range(args.reps):
        tm.append(wall(mixed)); tg.append(wall(grouped))
    px = sum(g.width * g.height for g, _, _ in probes)
    bm, bg = min(tm), min(tg)
    out["files_1024_mixed"] = {"groups": len(groups), "Mpx": round(px / 1e6, 1), "scan_MB": round(sum(len(f) for f in files) / 1e6, 1),
                               "mixed_ms": round(bm, 2), "grouped_ms": round(bg, 2), "mixed_over_grouped": round(bm / bg, 3),
                               "mixed_Gpx_s": round(px / bm / 1e6, 1), "grouped_Gpx_s": round(px / bg / 1e6, 1),
                               "mixed_all_ms": [round(x, 1) for x in tm], "grouped_all_ms": [round(x, 1) for x in tg]}


if args.part in ("items", "all"):
    items_part()
if args.part in ("files", "all"):
    files_part()
print(json.dumps(out))
