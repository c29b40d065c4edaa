#!/usr/bin/env python3
"""PNG files to device pixels: where the time of ffhip_png_decode_files_device goes, beside two yardsticks measured in the same session.

  sets      rgb1080: 256 x 1920x1080 RGB 8;  rgba256: 4096 x 256x256 RGBA 8 -- PIL-encoded from the pictures time_progressive.py synthesises
  reported  per set, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up, in ms:
            file_call   the whole call, wall clock        inflate_1t  one thread's ffhip_inflate, per file
            host        the call's host threads (chunk walk, CRCs, inflate)      upload / unfilter / expand   by HIP events (FFHIP_PNG_TIMES)
            tensor_call decode_png_to_tensors to uint8 CHW at 224 x 224
  yardsticks  pil_16   PIL's Image.open(...).convert("RGBA") on one core x n / 16: the CPU loader this replaces, on the sixteen CPUs a job gets
              sink     k_bgra_to_tensor (uint8 CHW) on the same pixel count: a streaming kernel of k_png_expand's shape
There is no pass / fail bar.  Prints one JSON line."""
import argparse, ctypes as C, io, json, os, statistics, struct, sys, time

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
os.environ["FFHIP_PNG_TIMES"] = "1"
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
        Image.fromarray(img, mode).save(bio, "PNG")
        out.append(bio.getvalue())
    return out


def idat(f):
    at, out = 8, b""
    while at < len(f):
        n = struct.unpack(">I", f[at:at + 4])[0]
        if f[at + 4:at + 8] == b"IDAT":
            out += f[at + 8:at + 8 + n]
        at += 12 + n
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


res = {"tool": "bench_png", "threads": args.threads, "rounds": args.rounds, "reps": args.reps}
for name in args.sets.split(","):
    n, w, h, mode = SETS[name]
    n = max(1, n // args.scale)
    rng = np.random.default_rng(414)
    ps = protos(w, h, mode, rng)
    files = [ps[k] for k in rng.integers(0, len(ps), n)]
    info = ops.png_probe(files[0])
    pitch = (4 * w + 15) & ~15
    d_out = ops.DeviceBuffer(nbytes=n * pitch * h)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * n)(*[d_out.ptr + i * pitch * h for i in range(n)])
    pitches, status = (C.c_int64 * n)(*([pitch] * n)), (C.c_int * n)()

    def file_call():
        capi.check(L.ffhip_png_decode_files_device(ptrs, lens, n, args.threads, outs, pitches, None, status, None), "ffhip_png_decode_files_device")

    if args.one_call:
        file_call()
        res[name] = {"files": n, "parts_levels": list(ops.png_last()), "stages_ms": [round(t, 3) for t in ops.png_times()]}
        continue

    streams = [np.frombuffer(idat(p), np.uint8) for p in ps]
    scratch = np.zeros(info.filtered_bytes, np.uint8)
    got = C.c_size_t()

    def inflate_all():
        for z in streams:
            capi.check(L.ffhip_inflate(z.ctypes.data, z.size, scratch.ctypes.data, scratch.size, C.byref(got)), "ffhip_inflate")

    def pil_all():
        for p in ps:
            Image.open(io.BytesIO(p)).convert("RGBA").load()

    def tensor_call():
        tensors.decode_png_to_tensors(files, size=(224, 224), stack=True, n_threads=args.threads)

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

    rows = {k: [] for k in ("file_call", "host", "upload", "unfilter", "expand", "inflate_1t", "tensor_call", "pil_16", "sink")}
    for _ in range(args.rounds):
        file_call()
        calls, stages = [], []
        for _ in range(args.reps):
            calls.append(wall(file_call))
            stages.append(ops.png_times())
        rows["file_call"].append(statistics.median(calls))
        for k, key in enumerate(("host", "upload", "unfilter", "expand")):
            rows[key].append(statistics.median(s[k] for s in stages))
        inflate_all()
        rows["inflate_1t"].append(statistics.median(wall(inflate_all) for _ in range(args.reps)) / len(ps))
        tensor_call()
        rows["tensor_call"].append(statistics.median(wall(tensor_call) for _ in range(args.reps)))
        rows["pil_16"].append(statistics.median(wall(pil_all) for _ in range(args.reps)) / len(ps) * n / 16)
        sink_ms()
        rows["sink"].append(statistics.median(sink_ms() for _ in range(args.reps)))
    px, filtered = n * w * h, n * info.filtered_bytes
    r = {k: fold(v) for k, v in rows.items()}
    r.update(files=n, width=w, height=h, mode=mode, file_MB=round(sum(len(f) for f in files) / 1e6, 1), filtered_MB=round(filtered / 1e6, 1),
             parts_levels=list(ops.png_last()),
             inflate_1t_MBps=round(info.filtered_bytes / rows_med / 1e3, 1) if (rows_med := statistics.median(rows["inflate_1t"])) else None,
             host_GBps=round(filtered / statistics.median(rows["host"]) / 1e6, 2),
             upload_GBps=round(filtered / statistics.median(rows["upload"]) / 1e6, 1),
             unfilter_GBps=round(2 * filtered / statistics.median(rows["unfilter"]) / 1e6, 1),
             expand_GBps=round((filtered + 4 * px) / statistics.median(rows["expand"]) / 1e6, 1), expand_Gpx_s=round(px / statistics.median(rows["expand"]) / 1e6, 2),
             sink_GBps=round(7 * px / statistics.median(rows["sink"]) / 1e6, 1), sink_Gpx_s=round(px / statistics.median(rows["sink"]) / 1e6, 2),
             files_per_s=round(n / statistics.median(rows["file_call"]) * 1e3), pil_16_over_file_call=round(statistics.median(rows["pil_16"]) / statistics.median(rows["file_call"]), 2))
    res[name] = r
    del t_out, d_out
    torch.cuda.empty_cache()
print(json.dumps(res))
