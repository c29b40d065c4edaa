#!/usr/bin/env python3
"""The alpha plane of lossy WebP files: what FFHIP_WEBP_ALPHA costs on top of the pixels='libwebp' file call, and where its time goes.

  sets      a1080: 64 x 1920x1080;  a256: 1024 x 256x256 -- PIL-encoded RGBA (quality 75) with a soft-edged mask as alpha
  kinds     lossless  the files as PIL writes them (a headerless VP8L stream, the filter the encoder chose)
            raw       the same colour and the same plane as a raw ALPH chunk, no filter (webp_alpha_writer)
            gradient  a1080 only: the same plane raw under the gradient filter, forced through the writer (the VP8L writer of the tests is
                      plain Python and too slow for 2 Mpixel planes, so the forced filter rides on a raw plane)
  reported  per set and kind, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up, in ms:
            flagged     ffhip_webp_decode_files_device_ex with both bits, wall clock
            host / upload / unfilter / merge   the alpha stage's four times (FFHIP_WEBP_ALPHA_TIMES; upload includes the VP8L kernels)
            unfilter_GBps, merge_GBps   alpha plane bytes per second through the two kernels; unfilter_us_per_MB
  yardsticks  unflagged  the same call without FFHIP_WEBP_ALPHA on the same files: the parent's code path; flagged - unflagged is alpha's cost
              pil_16     PIL's Image.open(...).convert("RGBA") on one core x n / 16
              png_unfilter_us_per_MB   k_png_unfilter per filtered megabyte, from profiles/r8_png_bench.json
              sink       k_bgra_to_tensor (uint8 CHW) on the same pixels: a streaming kernel of k_webp_alpha_merge's shape
There is no pass / fail bar.  Prints one JSON line."""
import argparse, ctypes as C, io, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="a1080,a256")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--scale", type=int, default=1, help="divide the sets' file counts (a quick look)")
args = ap.parse_args()
os.environ["FFHIP_WEBP_ALPHA_TIMES"] = "1"
from PIL import Image
import webp_alpha_writer as A
from ffpic_amd import capi, ops, tensors
L = capi.require_device(0)
import torch

SETS = {"a1080": (64, 1920, 1080), "a256": (1024, 256, 256)}
BOTH = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA


def protos(w, h, rng):
    """[(PIL's file, the plane PIL decodes from it)]"""
    out = []
    for k in range(4):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        r2 = ((xx - w * (0.4 + 0.05 * k)) / (0.45 * w)) ** 2 + ((yy - h / 2) / (0.4 * h)) ** 2
        mask = np.clip((1.0 - r2) * 6 * 255, 0, 255).astype(np.uint8)                       # opaque inside, a soft edge, clear outside
        bio = io.BytesIO()
        Image.fromarray(np.dstack([img, mask]), "RGBA").save(bio, "WEBP", quality=75)
        data = bio.getvalue()
        out.append((data, np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))[..., 3].copy()))
    return out


def wall(call):
    L.ffhip_stream_sync(None)
    t0 = time.perf_counter()
    call()
    L.ffhip_stream_sync(None)
    return (time.perf_counter() - t0) * 1e3


def fold(rounds):
    return {"median": round(statistics.median(rounds), 3), "min": round(min(rounds), 3), "max": round(max(rounds), 3)}


res = {"tool": "bench_webp_alpha", "threads": args.threads, "rounds": args.rounds, "reps": args.reps}
try:
    with open(os.path.join(ROOT, "profiles", "r8_png_bench.json")) as f:
        png = json.load(f)
    png_us = {k: round(1e3 * v["unfilter"]["median"] / v["filtered_MB"], 3) for k, v in png.items() if isinstance(v, dict) and "unfilter" in v}
except OSError:
    png_us = {}
res["png_unfilter_us_per_MB"] = png_us
for name in args.sets.split(","):
    n, w, h = SETS[name]
    n = max(1, n // args.scale)
    rng = np.random.default_rng(415)
    ps = protos(w, h, rng)
    pick = rng.integers(0, len(ps), n)
    kinds = {"lossless": [p for p, _ in ps], "raw": [A.wrap(p, a, A.RAW, A.NONE) for p, a in ps]}
    if name == "a1080":
        kinds["gradient"] = [A.wrap(p, a, A.RAW, A.GRADIENT) for p, a in ps]
    _, _, mbc, mbr = ops.webp_probe(ps[0][0], "libwebp")
    pitch, rows = 64 * mbc, 16 * mbr
    d_out = ops.DeviceBuffer(nbytes=n * pitch * rows)
    fmt = tensors.tensor_format()
    t_out = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
    items = (capi.TensorItem * n)(*[capi.TensorItem(d_out.ptr + i * pitch * rows, pitch, 0, 0, w, h, t_out[i].data_ptr(), w, w * h) for i in range(n)])
    e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()

    def sink_ms():
        L.ffhip_event_record(e0, None)
        capi.check(L.ffhip_bgra_to_tensor_items(items, n, C.byref(fmt), None))
        L.ffhip_event_record(e1, None)
        capi.check(L.ffhip_stream_sync(None))
        return L.ffhip_event_elapsed_ms(e0, e1)

    res[name] = {"files": n, "width": w, "height": h}
    for kind, protos_k in kinds.items():
        files = [protos_k[k] for k in pick]
        bufs, ptrs, lens = ops.file_args(files)
        outs = (C.c_void_p * n)(*[d_out.ptr + i * pitch * rows for i in range(n)])
        pitches, status = (C.c_int64 * n)(*([pitch] * n)), (C.c_int * n)()

        def call(flags):
            capi.check(L.ffhip_webp_decode_files_device_ex(ptrs, lens, n, args.threads, outs, pitches, None, flags, None, status, None), "ffhip_webp_decode_files_device_ex")

        def pil_all():
            for p in protos_k:
                Image.open(io.BytesIO(p)).convert("RGBA").load()

        rowsd = {k: [] for k in ("flagged", "unflagged", "host", "upload", "unfilter", "merge", "pil_16", "sink")}
        last = None
        for _ in range(args.rounds):
            call(BOTH)
            calls, stages = [], []
            for _ in range(args.reps):
                calls.append(wall(lambda: call(BOTH)))
                stages.append(ops.webp_alpha_times())
            last = ops.webp_alpha_last()
            rowsd["flagged"].append(statistics.median(calls))
            for k, key in enumerate(("host", "upload", "unfilter", "merge")):
                rowsd[key].append(statistics.median(s[k] for s in stages))
            call(capi.FFHIP_WEBP_PIXELS_LIBWEBP)
            rowsd["unflagged"].append(statistics.median(wall(lambda: call(capi.FFHIP_WEBP_PIXELS_LIBWEBP)) for _ in range(args.reps)))
            rowsd["pil_16"].append(statistics.median(wall(pil_all) for _ in range(args.reps)) / len(protos_k) * n / 16)
            sink_ms()
            rowsd["sink"].append(statistics.median(sink_ms() for _ in range(args.reps)))
        med = {k: statistics.median(v) for k, v in rowsd.items()}
        px = n * w * h
        r = {k: fold(v) for k, v in rowsd.items()}
        r.update(filters=sorted({ops.webp_alpha_probe(p)[2] for p in protos_k}), compression=sorted({ops.webp_alpha_probe(p)[1] for p in protos_k}),
                 planes_lossless_launches_parts=list(last), plane_MB=round(px / 1e6, 1), file_MB=round(sum(len(f) for f in files) / 1e6, 1),
                 alpha_cost_ms=round(med["flagged"] - med["unflagged"], 3),
                 unfilter_GBps=round(px / med["unfilter"] / 1e6, 2) if last[2] else None,          # no launch: the interval is two event records
                 unfilter_us_per_MB=round(1e3 * med["unfilter"] / (px / 1e6), 3) if last[2] else None,
                 merge_GBps=round(px / med["merge"] / 1e6, 1) if med["merge"] else None,
                 merge_Gpx_s=round(px / med["merge"] / 1e6, 2) if med["merge"] else None, sink_Gpx_s=round(px / med["sink"] / 1e6, 2),
                 host_MBps=round(px / med["host"] / 1e3, 1), files_per_s=round(n / med["flagged"] * 1e3),
                 pil_16_over_flagged=round(med["pil_16"] / med["flagged"], 2))
        res[name][kind] = r
    del t_out, d_out
    torch.cuda.empty_cache()
print(json.dumps(res))
