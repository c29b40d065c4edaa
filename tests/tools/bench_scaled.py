#!/usr/bin/env python3
"""Reduced-size JPEG decode (reduce= of decode_jpeg_to_tensors, ffhip_jpeg_recon_items_scaled); prints one JSON line.
  files:   256 files of 3840x2160 and 1 024 of 1920x1080, 4:2:0, to [N,3,224,224] uint8: reduce=1 (the full-size path) against
           reduce="auto" in the same process -- wall time of the whole call (it synchronises), one warm-up each, then --reps interleaved
           repetitions; medians, every repetition's figure, the ratio, the spread of each side (max - min over its median), the
           denominators chosen and the parts tensor_files_run took
  kernels: on the 256 x 4K batch's synthetic planes, ffhip_jpeg_recon_items against ffhip_jpeg_recon_items_scaled at 2, 4 and 8, ms per
           call by HIP events (interleaved), and what the reduced kernel reaches in bytes per second over the PLANES' size: it uses 32, 8 or 2
           of every 128 coefficient bytes, so its traffic is probably every coefficient line whatever the denominator
--scale divides the counts; --part files|kernels|all.  Needs PIL and torch."""
import argparse, ctypes as C, io, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from ffpic_amd import capi, ops, synth, tensors

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["files", "kernels", "all"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--threads", type=int, default=16)
args = ap.parse_args()
L = capi.require_device(0)
import torch
out = {"tool": "bench_scaled"}


def photo_like(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 37.0 + rng.random()), 128 + 90 * np.cos(yy / 29.0), (xx * 3 + yy * 5) // 16 % 256], axis=2)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def files_part(name, n, w, h):
    from PIL import Image
    rng = np.random.default_rng(w)
    protos = []
    for _ in range(4):
        bio = io.BytesIO()
        Image.fromarray(photo_like(rng, w, h)).save(bio, "JPEG", quality=85, subsampling=2)
        protos.append(bio.getvalue())
    files = [protos[i % 4] for i in range(n)]

    def run(reduce):
        t0 = time.perf_counter()
        batch, used = tensors.decode_jpeg_to_tensors(files, size=(224, 224), stack=True, n_threads=args.threads, reduce=reduce, return_reduce=True)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, used, ops.tensor_last_parts(), batch

    res = {"files": n, "file_bytes": len(protos[0])}
    for reduce in (1, "auto"):
        run(reduce)                                                      # warm-up: scratch grown, kernels loaded
    full, auto = [], []
    for _ in range(args.reps):                                           # interleaved: the same clocks for both
        ms, _, parts_full, a = run(1)
        full.append(ms)
        ms, used, parts_auto, b = run("auto")
        auto.append(ms)
    res["mean_abs_diff_of_the_tensors"] = round(float((a.float() - b.float()).abs().mean()), 3)   # two low-pass filters of one picture
    del a, b
    mf, ma = statistics.median(full), statistics.median(auto)
    res.update(full_ms=round(mf, 2), auto_ms=round(ma, 2), auto_over_full=round(ma / mf, 4),
               full_spread=round((max(full) - min(full)) / mf, 4), auto_spread=round((max(auto) - min(auto)) / ma, 4),
               full_all_ms=[round(x, 2) for x in full], auto_all_ms=[round(x, 2) for x in auto],
               denominators=sorted(set(used)), parts_full=parts_full, parts_auto=parts_auto)
    out[name] = res
    torch.cuda.empty_cache()


def kernels_part(n):
    mc, mr = 240, 135
    geom = capi.jpeg_geom(mc, mr)
    cy, cu, cv = synth.coef_batch(4, mc, mr)
    dy = torch.from_numpy(cy).cuda().repeat(n // 4)
    du = torch.from_numpy(cu).cuda().repeat(n // 4)
    dv = torch.from_numpy(cv).cuda().repeat(n // 4)
    dq = torch.from_numpy(np.tile(synth.quant_tables().reshape(-1), n).astype(np.int16)).cuda()
    pitch = geom.width * 4
    dout = torch.empty(n * pitch * geom.height, dtype=torch.uint8, device="cuda")
    yb, cb = geom.y_blocks * 128, geom.c_blocks * 128
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()

    def items_at(d):
        arr = (capi.JpegItem * n)()
        p = pitch // d
        for i in range(n):
            it = arr[i]
            it.geom = geom
            it.d_coef_y, it.d_coef_u, it.d_coef_v = dy.data_ptr() + i * yb, du.data_ptr() + i * cb, dv.data_ptr() + i * cb
            it.d_quant, it.d_bgra, it.pitch = dq.data_ptr() + i * 512, dout.data_ptr() + i * p * (geom.height // d), p
        return arr, (C.c_int * n)(*[d] * n)

    calls = {}
    for d in (1, 2, 4, 8):
        arr, den = items_at(d)
        calls[d] = (lambda arr=arr, den=den: capi.check(L.ffhip_jpeg_recon_items_scaled(arr, den, n, st)))

    def timed(f, k=5):
        L.ffhip_event_record(e0, st)
        for _ in range(k):
            f()
        L.ffhip_event_record(e1, st)
        capi.check(L.ffhip_stream_sync(st))
        return L.ffhip_event_elapsed_ms(e0, e1) / k

    for f in calls.values():
        timed(f, 2)
    ms = {d: [] for d in calls}
    for _ in range(args.reps):
        for d, f in calls.items():
            ms[d].append(timed(f))
    plane_bytes = n * (yb + 2 * cb)
    res = {"pictures": n, "planes_GB": round(plane_bytes / 1e9, 3)}
    for d in calls:
        m = statistics.median(ms[d])
        res[f"d{d}"] = {"ms": round(m, 3), "all_ms": [round(x, 3) for x in ms[d]], "planes_GBps": round(plane_bytes / m / 1e6, 1),
                        "bgra_GB": round(n * pitch * geom.height / d / d / 1e9, 3)}
    out["kernels_4k420"] = res
    L.ffhip_event_destroy(e0); L.ffhip_event_destroy(e1)


n4k, nhd = max(4, 256 // args.scale), max(4, 1024 // args.scale)
if args.part in ("files", "all"):
    files_part(f"4k_x{n4k}_to_224", n4k, 3840, 2160)
    files_part(f"1080p_x{nhd}_to_224", nhd, 1920, 1080)
if args.part in ("kernels", "all"):
    kernels_part(n4k // 4 * 4)
print(json.dumps(out))
