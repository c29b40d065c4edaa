#!/usr/bin/env python3
"""ffhip_bgra_resize_items on large batches; prints one JSON line.
  256 random pictures of 3840x2160 -> 224x224 and 1 024 of 1920x1080 -> 224x224 (--scale divides both counts), both filters: ms per call by
  HIP events (warm-up, then --blocks blocks of --reps calls; the median block), next to the time ffhip_copy_calibrate would need to READ the
  same source bytes once at the rate it reaches in the same process (a copy of B bytes moves 2 B), and the ratio of the two.  The kernel
  reads a source row once per output row whose run holds it: about twice with ANTIALIAS when shrinking, two rows of every shrink factor's
  worth with BILINEAR.  Pictures are spread over several allocations.  Needs torch."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ffpic_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--allocations", type=int, default=8)
args = ap.parse_args()
L = capi.require_device(0)
import torch
st = torch.cuda.current_stream().cuda_stream
e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()
out = {"tool": "bench_resize"}


def timed(f, k):
    L.ffhip_event_record(e0, st)
    for _ in range(k):
        f()
    L.ffhip_event_record(e1, st)
    capi.check(L.ffhip_stream_sync(st))
    return L.ffhip_event_elapsed_ms(e0, e1) / k


def run(name, n, w, h, ow, oh, cal):
    a = max(1, min(args.allocations, n))
    per = [(n - k + a - 1) // a for k in range(a)]
    bufs = [torch.empty(max(p, 1) * w * h * 4, dtype=torch.uint8, device="cuda").random_(0, 256) for p in per]
    dst = torch.empty(n * ow * oh * 4, dtype=torch.uint8, device="cuda")
    arr = (capi.ResizeItem * n)()
    for i in range(n):
        arr[i] = capi.ResizeItem(bufs[i % a].data_ptr() + (i // a) * w * h * 4, 4 * w, 0, 0, w, h, dst.data_ptr() + i * ow * oh * 4, 4 * ow, ow, oh)
    src_bytes = n * w * h * 4
    half = (src_bytes // 2) & ~255

    def copy():
        capi.check(L.ffhip_copy_calibrate(cal[0].data_ptr(), cal[1].data_ptr(), half, st))

    res = {"pictures": n, "source_GB": round(src_bytes / 1e9, 2)}
    for filt, fname in ((capi.FFHIP_RESIZE_ANTIALIAS, "antialias"), (capi.FFHIP_RESIZE_BILINEAR, "bilinear")):
        def resize():
            capi.check(L.ffhip_bgra_resize_items(arr, n, filt, st))
        for fn in (resize, copy):
            timed(fn, 2)
        blocks = [(timed(resize, args.reps), timed(copy, args.reps)) for _ in range(args.blocks)]
        r_ms, c_ms = statistics.median(b[0] for b in blocks), statistics.median(b[1] for b in blocks)
        rate = 2 * half / c_ms / 1e6                                      # GB/s the copy moves
        read_once = src_bytes / rate / 1e6
        res[fname] = {"resize_ms": round(r_ms, 3), "copy_GBps": round(rate, 1), "read_once_ms": round(read_once, 3), "resize_over_read_once": round(r_ms / read_once, 2),
                      "Gpx_s": round(n * w * h / r_ms / 1e6, 1), "all_resize_ms": [round(b[0], 3) for b in blocks]}
    out[name] = res


n4k, nhd = max(1, 256 // args.scale), max(1, 1024 // args.scale)
most = max(n4k * 3840 * 2160, nhd * 1920 * 1080) * 4
cal = [torch.empty(most // 2 + 256, dtype=torch.uint8, device="cuda") for _ in range(2)]
cal[1].random_(0, 256)
run(f"4k_x{n4k}_to_224", n4k, 3840, 2160, 224, 224, cal)
torch.cuda.empty_cache()
run(f"1080p_x{nhd}_to_224", nhd, 1920, 1080, 224, 224, cal)
print(json.dumps(out))
