#!/usr/bin/env python3
"""Device pictures to lossless WebP files: what ffhip_vp8l_encode_items takes, beside ffhip_png_encode_items on the same tensors in the same
process and PIL's lossless WebP encoder measured in the same session.  The twin of bench_png_encode.py.

  sets      uhd: 256 x 3840x2160 RGB;  thumb: 4096 x 256x256 RGBA -- HWC pictures on the device, every item a picture of its own (six
            synthetic prototypes, each item's rolled by its index), both transforms
  reported  per set and encoder, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up, the two
            encoders' calls interleaved: ms a call between two events on the call's stream (the call synchronises once a part, so host
            time between parts is inside), files/s, Gpixel/s, the files' bytes and their share of the pixels' bytes
  yardstick pil_16: PIL's Image.save(lossless=True, method=0, quality=0) of the same pictures from --threads threads; its files' bytes
  per kernel  --one-call: per set ONE lossless WebP call and nothing else, for rocprofv3 --kernel-trace --stats in a run of its own
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
ap.add_argument("--scale", type=int, default=1, help="divide the sets' picture counts (a quick look)")
ap.add_argument("--one-call", action="store_true", help="per set ONE lossless WebP call and nothing else: for rocprofv3 --kernel-trace --stats")
ap.add_argument("--no-pil", action="store_true")
args = ap.parse_args()
import torch
from ffpic_amd import capi, ops
L = capi.require_device(0)

SETS = {"uhd": (256, 3840, 2160, 3), "thumb": (4096, 256, 256, 4)}


def protos(w, h, c, rng):
    out = []
    for k in range(6):
        yy, xx = np.mgrid[0:h, 0:w]
        planes = [128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2,
                  255 * ((xx // 32 + yy // 32 + k) % 3 > 0)][:c]
        img = np.stack(planes, axis=2)
        img[..., :3] += rng.normal(0, 2, img[..., :3].shape)
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


result = {"flags": "subtract green, predict", "threads": args.threads}
rng = np.random.default_rng(3)
for name in args.sets.split(","):
    n, w, h, c = SETS[name]
    n = max(n // args.scale, 1)
    pics = protos(w, h, c, rng)
    host = [np.roll(pics[i % len(pics)], i, axis=0) for i in range(n)]    # every item a picture of its own
    dev = [ops.DeviceBuffer(host=p) for p in host]
    cap = (max(ops.vp8l_encode_bound(w, h), ops.png_encode_bound(w, h, c)) + 255) & ~255
    out = ops.DeviceBuffer(nbytes=n * cap)
    webp_items, png_items = [], []
    for i in range(n):
        it = capi.Vp8lEncodeItem()
        it.src = capi.png_source(dev[i].ptr, w, h, c * w, c, tuple(range(c)))
        it.flags, it.d_out, it.cap = 3, out.ptr + i * cap, cap
        webp_items.append(it)
        it = capi.PngEncodeItem()
        it.src = capi.png_source(dev[i].ptr, w, h, c * w, c, tuple(range(c)))
        it.filter, it.d_out, it.cap = capi.FFHIP_PNG_FILTER_ADAPTIVE, out.ptr + i * cap, cap
        png_items.append(it)
    lens = {"webp": [], "png": []}

    def webp_call():
        lens["webp"][:] = ops.vp8l_encode_items(webp_items, stream.cuda_stream)[0]

    def png_call():
        lens["png"][:] = ops.png_encode_items(png_items, stream.cuda_stream)[0]
    if args.one_call:
        webp_call()
        result[name] = {"files": n, "bytes": sum(lens["webp"])}
        continue
    webp_call()                                                       # warm-up: the scratch grows here
    png_call()
    rounds = {"webp": [], "png": []}
    for _ in range(args.rounds):
        reps = {"webp": [], "png": []}
        for _ in range(args.reps):                                    # interleaved: both see the same machine
            reps["webp"].append(timed(webp_call))
            reps["png"].append(timed(png_call))
        for k in reps:
            rounds[k].append(statistics.median(reps[k]))
    row = {"files": n, "width": w, "height": h, "channels": c}
    for k in ("webp", "png"):
        ms = summary(rounds[k])
        row[k] = {"call_ms": ms, "files_per_s": round(n / ms[0] * 1e3, 1), "gpixel_per_s": round(n * w * h / ms[0] / 1e6, 3), "bytes": sum(lens[k]),
                  "share_of_pixels": round(sum(lens[k]) / (n * w * h * c), 4)}
    if not args.no_pil:
        from PIL import Image
        mode = "RGB" if c == 3 else "RGBA"
        count = min(n, 2 * args.threads if name == "uhd" else n // 4)

        def save(i):
            bio = io.BytesIO()
            Image.fromarray(host[i], mode).save(bio, "WEBP", lossless=True, method=0, quality=0)
            return bio.tell()
        with ThreadPoolExecutor(args.threads) as pool:
            list(pool.map(save, range(min(args.threads, count))))
            t = time.perf_counter()
            sizes = list(pool.map(save, range(count)))
            dt = time.perf_counter() - t
        row["pil_16"] = {"files": count, "files_per_s": round(count / dt, 1), "gpixel_per_s": round(count * w * h / dt / 1e9, 3),
                         "share_of_pixels": round(sum(sizes) / (count * w * h * c), 4)}
    result[name] = row
    del out, dev
print(json.dumps(result))
