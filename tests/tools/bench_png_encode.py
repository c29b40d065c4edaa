#!/usr/bin/env python3
"""Device pictures to PNG files: what ffhip_png_encode_items takes, beside PIL's encoder measured in the same session.

  sets      uhd: 256 x 3840x2160 RGB;  thumb: 4096 x 256x256 RGBA -- HWC pictures on the device, every item a picture of its own (six
            synthetic prototypes, each item's rolled by its index), adaptive filters
  reported  per set, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up: ms a call, files/s, Gpixel/s,
            the files' bytes and their share of the pixels' bytes
  yardstick pil_16: PIL's Image.save(compress_level=1) of the same pictures from --threads threads (zlib releases the GIL); its files' bytes
  per kernel  --one-call: per set ONE file call and nothing else, for rocprofv3 --kernel-trace --stats in a run of its own
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
ap.add_argument("--one-call", action="store_true", help="per set ONE file call and nothing else: for rocprofv3 --kernel-trace --stats")
ap.add_argument("--no-pil", action="store_true")
args = ap.parse_args()
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


def wall(call):
    L.ffhip_stream_sync(None)
    t = time.perf_counter()
    call()
    L.ffhip_stream_sync(None)
    return (time.perf_counter() - t) * 1e3


result = {"filter": "adaptive", "threads": args.threads}
rng = np.random.default_rng(3)
for name in args.sets.split(","):
    n, w, h, c = SETS[name]
    n = max(n // args.scale, 1)
    pics = protos(w, h, c, rng)
    host = [np.roll(pics[i % len(pics)], i, axis=0) for i in range(n)]    # every item a picture of its own
    dev = [ops.DeviceBuffer(host=p) for p in host]
    cap = (ops.png_encode_bound(w, h, c) + 255) & ~255
    out = ops.DeviceBuffer(nbytes=n * cap)
    items = []
    for i in range(n):
        it = capi.PngEncodeItem()
        it.src = capi.png_source(dev[i].ptr, w, h, c * w, c, tuple(range(c)))
        it.filter, it.d_out, it.cap = capi.FFHIP_PNG_FILTER_ADAPTIVE, out.ptr + i * cap, cap
        items.append(it)
    lens = []

    def call():
        lens[:] = ops.png_encode_items(items)[0]
    if args.one_call:
        call()
        result[name] = {"files": n, "bytes": sum(lens)}
        continue
    call()                                                            # warm-up: the scratch grows here
    rounds = [statistics.median(wall(call) for _ in range(args.reps)) for _ in range(args.rounds)]
    ms = summary(rounds)
    row = {"files": n, "width": w, "height": h, "channels": c, "call_ms": ms, "files_per_s": round(n / ms[0] * 1e3, 1),
           "gpixel_per_s": round(n * w * h / ms[0] / 1e6, 3), "bytes": sum(lens), "share_of_pixels": round(sum(lens) / (n * w * h * c), 4)}
    if not args.no_pil:
        from PIL import Image
        mode = "RGB" if c == 3 else "RGBA"
        count = min(n, 4 * args.threads if name == "uhd" else n)

        def save(i):
            bio = io.BytesIO()
            Image.fromarray(host[i], mode).save(bio, "PNG", compress_level=1)
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
