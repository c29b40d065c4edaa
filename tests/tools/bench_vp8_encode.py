#!/usr/bin/env python3
"""Device pictures to lossy WebP files: what ffhip_vp8_encode_items takes, beside PIL's lossy WebP encoder at method 0 measured in the
same session.  The twin of bench_vp8l_encode.py.

  sets      uhd: 256 x 3840x2160 RGB;  thumb: 4096 x 256x256 RGB -- HWC pictures on the device, every item a picture of its own (six
            synthetic prototypes, each item's rolled by its index), quality 75, the rule's own loop filter level
  reported  per set the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up: ms a call between two events
            on the call's stream (the call synchronises once a part, so host time between parts is inside), files/s, Gpixel/s, the files'
            bytes and their share of the pixels' bytes
  yardstick pil_16: PIL's Image.save(quality=75, method=0) of the same pictures from --threads threads; its files' bytes
  per kernel  --one-call: per set ONE call and nothing else, for rocprofv3 --kernel-trace --stats in a run of its own
There is no pass / fail bar.  Prints one JSON line."""
import argparse, io, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="uhd,thumb")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--quality", type=int, default=75)
ap.add_argument("--scale", type=int, default=1, help="divide the sets' picture counts (a quick look)")
ap.add_argument("--one-call", action="store_true", help="per set ONE call and nothing else: for rocprofv3 --kernel-trace --stats")
ap.add_argument("--no-pil", action="store_true")
args = ap.parse_args()
import torch
from ffpic_amd import capi, ops
L = capi.require_device(0)

SETS = {"uhd": (256, 3840, 2160), "thumb": (4096, 256, 256)}


def protos(w, h, rng):
    out = []
    for k in range(6):
        yy, xx = np.mgrid[0:h, 0:w]
        planes = [128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2]
        img = np.stack(planes, axis=2) + rng.normal(0, 2, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def summary(values):
    return [round(statistics.median(values), 3), round(min(values), 3), round(max(values), 3)]


stream = torch.cuda.Stream()


def timed(call):
    """milliseconds between two events on the call's stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


result = {"quality": args.quality, "threads": args.threads}
rng = np.random.default_rng(3)
for name in args.sets.split(","):
    n, w, h = SETS[name]
    n = max(n // args.scale, 1)
    pics = protos(w, h, rng)
    host = [np.roll(pics[i % len(pics)], i, axis=0) for i in range(n)]    # every item a picture of its own
    dev = [ops.DeviceBuffer(host=p) for p in host]
    cap = (w * h * 3 // 2 + 255) & ~255                                   # half the pixels' bytes, as tensors.encode_webp starts
    out = ops.DeviceBuffer(nbytes=n * cap)
    items = []
    for i in range(n):
        it = capi.Vp8EncodeItem()
        it.src = capi.jpeg_source(dev[i].ptr, w, h, 3 * w, 3, (0, 1, 2), 3)
        it.quality, it.filter, it.d_out, it.cap = args.quality, -1, out.ptr + i * cap, cap
        items.append(it)
    lens = []

    def call():
        lens[:] = ops.vp8_encode_items(items, stream.cuda_stream)[0]
    if args.one_call:
        call()
        result[name] = {"files": n, "bytes": sum(lens)}
        continue
    call()                                                                # warm-up: the scratch grows here
    rounds = []
    for _ in range(args.rounds):
        rounds.append(statistics.median([timed(call) for _ in range(args.reps)]))
    ms = summary(rounds)
    row = {"files": n, "width": w, "height": h, "call_ms": ms, "files_per_s": round(n / ms[0] * 1e3, 1), "gpixel_per_s": round(n * w * h / ms[0] / 1e6, 3),
           "bytes": sum(lens), "share_of_pixels": round(sum(lens) / (n * w * h * 3), 4)}
    if not args.no_pil:
        from PIL import Image
        count = min(n, 2 * args.threads if name == "uhd" else n // 4)

        def save(i):
            bio = io.BytesIO()
            Image.fromarray(host[i], "RGB").save(bio, "WEBP", quality=args.quality, method=0)
            return bio.tell()
        with ThreadPoolExecutor(args.threads) as pool:
            list(pool.map(save, range(min(args.threads, count))))
            t = time.perf_counter()
            sizes = list(pool.map(save, range(count)))
            dt = time.perf_counter() - t
        row["pil_16"] = {"files": count, "files_per_s": round(count / dt, 1), "gpixel_per_s": round(count * w * h / dt / 1e9, 3),
                         "share_of_pixels": round(sum(sizes) / (count * w * h * 3), 4), "ours_bytes_same_files": sum(lens[:count]), "bytes": sum(sizes)}
    result[name] = row
    del out, dev
print(json.dumps(result))
