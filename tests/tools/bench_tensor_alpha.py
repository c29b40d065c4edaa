#!/usr/bin/env python3
"""The alpha forms of the tensor sink (ffhip_bgra_to_tensor_items_alpha) and the premultiplying resize
(ffhip_bgra_resize_items_premultiplied); prints one JSON line.  The method of bench_tensor_sink.py and bench_resize.py: HIP events, a
warm-up and a first block, then the median of --blocks blocks of --reps calls.
  sink:    each dtype x layout (order RGB; --orders RGB,BGR for both) x the five policies a mode and a source kind come to, on --pictures
           (256) random pictures of 3840x2160: ms per call, GB/s of (4 + output bytes) x pixels, next to ffhip_copy_calibrate moving the
           same number of bytes and next to the three-channel form of the same dtype and layout, all three timed in the same process and
           alternating within every block; the ratios to both, and the twin's own spread over its blocks (max / min).
  resize:  the same 4K pictures -> 224x224, both filters, the premultiplying call beside ffhip_bgra_resize_items, alternating.
--part sink|resize|all (default all).  Needs torch."""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ffpic_amd import capi, tensors

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["sink", "resize", "all"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--pictures", type=int, default=256)
ap.add_argument("--orders", default="RGB")
ap.add_argument("--allocations", type=int, default=8)
args = ap.parse_args()
L = capi.require_device(0)
import torch
out = {"tool": "bench_tensor_alpha", "pictures": args.pictures, "reps": args.reps, "blocks": args.blocks}
W, H = 3840, 2160
ES = {"uint8": 1, "float16": 2, "float32": 4}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
#            name                         alpha=                      the source is premultiplied
POLICIES = [("straight_keep", "straight", False), ("premultiply", "premultiplied", False), ("unpremultiply", "straight", True),
            ("over_straight", ("over", (255, 255, 255)), False), ("over_premultiplied", ("over", (255, 255, 255)), True)]
st = torch.cuda.current_stream().cuda_stream
e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()


def timed(f, k):
    L.ffhip_event_record(e0, st)
    for _ in range(k):
        f()
    L.ffhip_event_record(e1, st)
    capi.check(L.ffhip_stream_sync(st))
    return L.ffhip_event_elapsed_ms(e0, e1) / k


def measure(calls):
    """calls {name: fn}: warm-up, a first block, then --blocks blocks, every block timing every call in turn -> {name: [ms per block]}"""
    for fn in calls.values():
        timed(fn, 2)
    first = {k: timed(fn, args.reps) for k, fn in calls.items()}
    t = {k: [] for k in calls}
    for _ in range(args.blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, args.reps))
    return t, first


def spread(byte_sizes):
    """every size its place (256-byte aligned) in one of --allocations allocations, dealt round robin -> (tensors kept alive, addresses)"""
    a = max(1, min(args.allocations, len(byte_sizes)))
    fill, where = [0] * a, []
    for i, b in enumerate(byte_sizes):
        where.append((i % a, fill[i % a]))
        fill[i % a] += (b + 255) & ~255
    bufs = [torch.empty(max(f, 256), dtype=torch.uint8, device="cuda") for f in fill]
    return bufs, [bufs[k].data_ptr() + o for k, o in where]


n, px = args.pictures, args.pictures * W * H
src_bufs, src = spread([4 * W * H] * n)
for b in src_bufs:
    b.random_(0, 256)                                                       # alpha random too: every branch of the rule is taken


def sink_part():
    cal = [torch.empty(10 * px + 256, dtype=torch.uint8, device="cuda") for _ in range(2)]
    cal[1].random_(0, 256)
    res = {}
    for dtype in ES:
        for layout in ("CHW", "HWC"):
            for order in args.orders.split(","):
                es = ES[dtype]
                f = tensors.tensor_format(dtype, layout, order, None if dtype == "uint8" else MEAN, None if dtype == "uint8" else STD)
                out_bufs, dst = spread([4 * W * H * es] * n)              # room for four channels; the twin uses three of them
                items = {}
                for nc in (3, 4):
                    items[nc] = (capi.TensorItem * n)(*[capi.TensorItem(src[i], 4 * W, 0, 0, W, H, dst[i], W if layout == "CHW" else nc * W, W * H)
                                                       for i in range(n)])
                for name, alpha, pre in POLICIES:
                    record = tensors.tensor_alpha(alpha, normalised=dtype != "uint8", source_premultiplied=pre)
                    nc = tensors.alpha_channels(alpha)
                    traffic, twin_traffic = (4 + nc * es) * px, (4 + 3 * es) * px
                    half = (traffic // 2) & ~255                            # a copy of `half` bytes moves the form's bytes
                    calls = {
                        "alpha": lambda: capi.check(L.ffhip_bgra_to_tensor_items_alpha(items[nc], n, C.byref(f), C.byref(record), st)),
                        "copy": lambda: capi.check(L.ffhip_copy_calibrate(cal[0].data_ptr(), cal[1].data_ptr(), half, st)),
                        "twin": lambda: capi.check(L.ffhip_bgra_to_tensor_items(items[3], n, C.byref(f), st)),
                    }
                    t, first = measure(calls)
                    ms = {k: statistics.median(v) for k, v in t.items()}
                    rate = {"alpha": traffic / ms["alpha"] / 1e6, "copy": 2 * half / ms["copy"] / 1e6, "twin": twin_traffic / ms["twin"] / 1e6}
                    res[f"{dtype}_{layout}_{order}_{name}"] = {
                        "channels": nc, "ms": round(ms["alpha"], 3), "GBps": round(rate["alpha"], 1), "copy_ms": round(ms["copy"], 3),
                        "copy_GBps": round(rate["copy"], 1), "twin_ms": round(ms["twin"], 3), "twin_GBps": round(rate["twin"], 1),
                        "over_copy": round(rate["alpha"] / rate["copy"], 3), "over_twin": round(rate["alpha"] / rate["twin"], 3),
                        "twin_spread": round(max(t["twin"]) / min(t["twin"]), 3), "blocks_ms": [round(x, 3) for x in t["alpha"]],
                        "first_block_ms": {k: round(v, 3) for k, v in first.items()}}
                del out_bufs
                torch.cuda.empty_cache()
    out["sink_4k"] = res


def resize_part():
    side = 224
    dst_bufs, dst = spread([4 * side * side] * n)
    arr = (capi.ResizeItem * n)(*[capi.ResizeItem(src[i], 4 * W, 0, 0, W, H, dst[i], 4 * side, side, side) for i in range(n)])
    res = {}
    for name, filt in (("bilinear", capi.FFHIP_RESIZE_BILINEAR), ("antialias", capi.FFHIP_RESIZE_ANTIALIAS)):
        calls = {"premultiplied": lambda: capi.check(L.ffhip_bgra_resize_items_premultiplied(arr, n, filt, st)),
                 "plain": lambda: capi.check(L.ffhip_bgra_resize_items(arr, n, filt, st))}
        t, first = measure(calls)
        ms = {k: statistics.median(v) for k, v in t.items()}
        res[name] = {"premultiplied_ms": round(ms["premultiplied"], 3), "plain_ms": round(ms["plain"], 3),
                     "premultiplied_over_plain": round(ms["premultiplied"] / ms["plain"], 3),
                     "plain_spread": round(max(t["plain"]) / min(t["plain"]), 3), "Gpx_s_in": round(px / ms["premultiplied"] / 1e6, 1),
                     "blocks_ms": [round(x, 3) for x in t["premultiplied"]], "first_block_ms": {k: round(v, 3) for k, v in first.items()}}
    out["resize_4k_to_224"] = res


if args.part in ("sink", "all"):
    sink_part()
if args.part in ("resize", "all"):
    resize_part()
print(json.dumps(out))
