#!/usr/bin/env python3
"""Device pictures to baseline JPEG files: what ffhip_jpeg_encode_items takes, beside PIL's encoder measured in the same session.

  sets      uhd: 256 x 3840x2160;  thumb: 4096 x 256x256 -- HWC RGB pictures on the device (six synthetic prototypes, every item a picture of
            its own output), quality 75, 4:2:0, no restart intervals
  reported  per set, the median (min .. max) over --rounds rounds of the median of --reps calls after a warm-up: ms a call, files/s, Gpixel/s,
            the files' bytes; fdct_ms: ffhip_jpeg_fdct_items alone on the same pictures (events)
  yardstick pil_16: PIL's Image.save(quality=75, subsampling=2) of the same pictures from --threads threads (the encoder releases the GIL)
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

SETS = {"uhd": (256, 3840, 2160), "thumb": (4096, 256, 256)}
QUALITY, LAYOUT = 75, capi.FFHIP_JPEG_ENC_420


def protos(w, h, rng):
    out = []
    for k in range(6):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
        out.append(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))
    return out


def summary(values):
    return [round(statistics.median(values), 3), round(min(values), 3), round(max(values), 3)]


def wall(call):
    L.ffhip_stream_sync(None)
    t = time.perf_counter()
    call()
    L.ffhip_stream_sync(None)
    return (time.perf_counter() - t) * 1e3


result = {"quality": QUALITY, "subsampling": "4:2:0", "threads": args.threads}
rng = np.random.default_rng(3)
for name in args.sets.split(","):
    n, w, h = SETS[name]
    n = max(n // args.scale, 1)
    pics = protos(w, h, rng)
    dev = [ops.DeviceBuffer(host=p) for p in pics]
    cap = (w * h + 4095) & ~4095                                      # a third of the pixels' bytes: ample at quality 75
    out = ops.DeviceBuffer(nbytes=n * cap)
    items = []
    for i in range(n):
        it = capi.JpegEncodeItem()
        it.src = capi.jpeg_source(dev[i % len(dev)].ptr, w, h, 3 * w, 3, (0, 1, 2), 3)
        it.layout, it.quality, it.restart, it.d_out, it.cap = LAYOUT, QUALITY, 0, out.ptr + i * cap, cap
        items.append(it)
    lens = []

    def call():
        lens[:] = ops.jpeg_encode_items(items)[0]
    if args.one_call:
        call()
        result[name] = {"files": n, "bytes": sum(lens)}
        continue
    call()                                                            # warm-up: the scratch grows here
    rounds = [statistics.median(wall(call) for _ in range(args.reps)) for _ in range(args.rounds)]
    ms = summary(rounds)
    row = {"files": n, "width": w, "height": h, "call_ms": ms, "files_per_s": round(n / ms[0] * 1e3, 1), "gpixel_per_s": round(n * w * h / ms[0] / 1e6, 3),
           "bytes": sum(lens), "mean_file_bytes": sum(lens) // n}
    # the first stage alone, into planes of its own
    blocks = (-(-w // 16)) * (-(-h // 16)) * 6
    group = max(min(n, (1 << 30) // (blocks * 128)), 1)
    planes = ops.DeviceBuffer(nbytes=group * blocks * 128)
    fitems = []
    for i in range(group):
        f = capi.JpegFdctItem()
        f.src, f.layout, f.quality = items[i].src, LAYOUT, QUALITY
        base = planes.ptr + i * blocks * 128
        f.d_coef_y, f.d_coef_u, f.d_coef_v = base, base + blocks * 128 * 4 // 6, base + blocks * 128 * 5 // 6
        fitems.append(f)
    ops.jpeg_fdct_items(fitems)
    fd = summary([statistics.median(wall(lambda: ops.jpeg_fdct_items(fitems)) for _ in range(args.reps)) for _ in range(args.rounds)])
    row["fdct_ms"], row["fdct_files"], row["fdct_gpixel_per_s"] = fd, group, round(group * w * h / fd[0] / 1e6, 3)
    if not args.no_pil:
        from PIL import Image
        images = [Image.fromarray(p, "RGB") for p in pics]
        count = min(n, 8 * args.threads if name == "uhd" else n)

        def save(i):
            bio = io.BytesIO()
            images[i % len(images)].save(bio, "JPEG", quality=QUALITY, subsampling=2)
            return bio.tell()
        with ThreadPoolExecutor(args.threads) as pool:
            list(pool.map(save, range(args.threads)))
            t = time.perf_counter()
            sizes = list(pool.map(save, range(count)))
            dt = time.perf_counter() - t
        row["pil_16"] = {"files": count, "files_per_s": round(count / dt, 1), "gpixel_per_s": round(count * w * h / dt / 1e9, 3)}
        assert sizes[0] == lens[0], (sizes[0], lens[0])                # the same file
    result[name] = row
    del out, planes
print(json.dumps(result))
