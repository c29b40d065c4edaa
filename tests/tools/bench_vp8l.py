#!/usr/bin/env python3
"""Lossless WebP files to device pixels: where the time of ffhip_vp8l_decode_files_device goes, beside yardsticks measured in the same session.

  sets      rgb1080: 256 x 1920x1080 RGB;  rgba256: 4096 x 256x256 RGBA -- PIL-encoded (lossless=True) from the pictures time_progressive.py synthesises
  reported  per set, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up, in ms:
            file_call   the whole call, wall clock        stream_1t   one thread's stream decode (transform sub-images and residual image), per file
            host        the call's host threads            upload / predict / finish   by HIP events (FFHIP_VP8L_TIMES)
            tensor_call decode_webp_lossless_to_tensors to uint8 CHW at 224 x 224
  yardsticks  pil_16   PIL's Image.open(...).convert("RGBA") on one core x n / 16: the CPU loader this replaces, on the sixteen CPUs a job gets
              sink     k_bgra_to_tensor (uint8 CHW) on the same pixel count: a streaming kernel of k_vp8l_finish's shape
              png_unfilter_ms_per_MB   k_png_unfilter's time per filtered megabyte, from profiles/r8_png_bench.json, beside predict_ms_per_MB
There is no pass / fail bar.  Prints one JSON line."""
import argparse, ctypes as C, io, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="rgb1080,rgba256")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--scale", type=int, default=1, help="divide the sets' file counts (a quick look)")
ap.add_argument("--one-call", action="store_true", help="per set ONE file call and nothing else: for rocprofv3 --kernel-trace --stats")
args = ap.parse_args()
os.environ["FFHIP_VP8L_TIMES"] = "1"
from PIL import Image
from ffpic_amd import capi, ops, tensors
L = capi.require_device(0)
import torch

SETS = {"rgb1080": (256, 1920, 1080, "RGB"), "rgba256": (4096, 256, 256, "RGBA")}


def protos(w, h, mode, rng):
    out = []
    for k in range(6):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        if mode == "RGBA":
            img = np.dstack([img, ((xx + yy + 31 * k) % 256).astype(np.uint8)])
        bio = io.BytesIO()
        Image.fromarray(img, mode).save(bio, "WEBP", lossless=True)
        out.append(bio.getvalue())
    return out


def wall(call):
    L.ffhip_stream_sync(None)
    t0 = time.perf_counter()
    call()
    L.ffhip_stream_sync(None)
    return (time.perf_counter() - t0) * 1e3


def fold(rounds):
    """[per-round value] -> 'median (min .. max)' as numbers"""
    return {"median": round(statistics.median(rounds), 3), "min": round(min(rounds), 3), "max": round(max(rounds), 3)}


def file_args(files, w, h, d_out, pitch):
    n = len(files)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * n)(*[d_out.ptr + i * pitch * h for i in range(n)])
    return bufs, ptrs, lens, outs, (C.c_int64 * n)(*([pitch] * n)), (C.c_int * n)()


res = {"tool": "bench_vp8l", "threads": args.threads, "rounds": args.rounds, "reps": args.reps}
try:
    with open(os.path.join(ROOT, "profiles", "r8_png_bench.json")) as f:
        png = json.load(f)
except OSError:
    png = {}
for name in args.sets.split(","):
    n, w, h, mode = SETS[name]
    n = max(1, n // args.scale)
    rng = np.random.default_rng(414)
    ps = protos(w, h, mode, rng)
    files = [ps[k] for k in rng.integers(0, len(ps), n)]
    infos = [ops.vp8l_info(p) for p in ps]
    pitch = (4 * w + 15) & ~15
    d_out = ops.DeviceBuffer(nbytes=n * pitch * h)
    bufs, ptrs, lens, outs, pitches, status = file_args(files, w, h, d_out, pitch)
    one = file_args(ps, w, h, d_out, pitch)

    def file_call():
        capi.check(L.ffhip_vp8l_decode_files_device(ptrs, lens, n, args.threads, outs, pitches, None, status, None), "ffhip_vp8l_decode_files_device")

    if args.one_call:
        file_call()
        res[name] = {"files": n, "parts_levels_host": list(ops.vp8l_last()), "stages_ms": [round(t, 3) for t in ops.vp8l_times()]}
        continue

    def stream_1t():
        """the six pictures through the call on ONE host thread: its host stage is one thread's stream decode"""
        capi.check(L.ffhip_vp8l_decode_files_device(one[1], one[2], len(ps), 1, one[3], one[4], None, one[5], None), "ffhip_vp8l_decode_files_device")
        return ops.vp8l_times()[0] / len(ps)

    def pil_all():
        for p in ps:
            Image.open(io.BytesIO(p)).convert("RGBA").load()

    def tensor_call():
        tensors.decode_webp_lossless_to_tensors(files, size=(224, 224), stack=True, n_threads=args.threads)

    # the sink's yardstick: the same pictures' BGRA (the file call has just written them) to uint8 CHW
    fmt = tensors.tensor_format()
    t_out = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
    items = (capi.TensorItem * n)(*[capi.TensorItem(d_out.ptr + i * pitch * h, pitch, 0, 0, w, h, t_out[i].data_ptr(), w, w * h) for i in range(n)])
    e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()

    def sink_ms():
        L.ffhip_event_record(e0, None)
        capi.check(L.ffhip_bgra_to_tensor_items(items, n, C.byref(fmt), None))
        L.ffhip_event_record(e1, None)
        capi.check(L.ffhip_stream_sync(None))
        return L.ffhip_event_elapsed_ms(e0, e1)

    rows = {k: [] for k in ("file_call", "host", "upload", "predict", "finish", "stream_1t", "tensor_call", "pil_16", "sink")}
    last = None
    for _ in range(args.rounds):
        file_call()
        calls, stages = [], []
        for _ in range(args.reps):
            calls.append(wall(file_call))
            stages.append(ops.vp8l_times())
        last = ops.vp8l_last()
        rows["file_call"].append(statistics.median(calls))
        for k, key in enumerate(("host", "upload", "predict", "finish")):
            rows[key].append(statistics.median(s[k] for s in stages))
        stream_1t()
        rows["stream_1t"].append(statistics.median(stream_1t() for _ in range(args.reps)))
        tensor_call()
        rows["tensor_call"].append(statistics.median(wall(tensor_call) for _ in range(args.reps)))
        rows["pil_16"].append(statistics.median(wall(pil_all) for _ in range(args.reps)) / len(ps) * n / 16)
        sink_ms()
        rows["sink"].append(statistics.median(sink_ms() for _ in range(args.reps)))
    med = {k: statistics.median(v) for k, v in rows.items()}
    px = n * w * h
    residual = 4 * sum(i.residual_width * i.height for i in infos) / len(infos) * n        # bytes of residual images in the call
    r = {k: fold(v) for k, v in rows.items()}
    r.update(files=n, width=w, height=h, mode=mode, file_MB=round(sum(len(f) for f in files) / 1e6, 1), residual_MB=round(residual / 1e6, 1),
             transforms=sorted({tuple(i.transforms[:i.n_transforms]) for i in infos}), cache_bits=sorted({i.cache_bits for i in infos}),
             meta=sorted({i.has_meta for i in infos}), parts_levels_host=list(last),
             stream_1t_MBps=round(residual / n / med["stream_1t"] / 1e3, 1), host_GBps=round(residual / med["host"] / 1e6, 2),
             upload_GBps=round(residual / med["upload"] / 1e6, 1),
             predict_GBps=round(2 * residual / med["predict"] / 1e6, 1) if med["predict"] else None,
             predict_ms_per_MB=round(med["predict"] / (residual / 1e6), 5),
             png_unfilter_ms_per_MB=round(png[name]["unfilter"]["median"] / png[name]["filtered_MB"], 5) if name in png else None,
             finish_GBps=round((residual + 4 * px) / med["finish"] / 1e6, 1), finish_Gpx_s=round(px / med["finish"] / 1e6, 2),
             sink_GBps=round(7 * px / med["sink"] / 1e6, 1), sink_Gpx_s=round(px / med["sink"] / 1e6, 2),
             files_per_s=round(n / med["file_call"] * 1e3), pil_16_over_file_call=round(med["pil_16"] / med["file_call"], 2))
    res[name] = r
    del t_out, d_out
    torch.cuda.empty_cache()
print(json.dumps(res))
