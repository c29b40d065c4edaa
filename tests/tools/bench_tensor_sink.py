#!/usr/bin/env python3
"""The tensor sink (ffhip_bgra_to_tensor_items) and the file calls on it; prints one JSON line.
  sink:   each of the 12 formats on --pictures (256) random pictures of 3840x2160 and on 1 024 pictures of the ten sizes of
          bench_mixed_files.py: ms per call by HIP events (warm-up, then two blocks; the second counts), GB/s of (4 + output bytes) x pixels,
          next to ffhip_copy_calibrate moving the same number of bytes in the same process, and the ratio of the two rates.  Pictures and
          outputs are spread over several allocations.
  files:  ffhip_jpeg_decode_files_tensor against ffhip_jpeg_decode_files_mixed_device on the same batch (--files (256) copies of a 4K 4:2:0
          file, and the 1 024-file mixed set with --mixed-files), wall time of the whole call, best of --reps, alternating: the difference
          is the price of the extra pass.
--part sink|files|all (default all).  Needs torch; the files part needs PIL."""
import argparse, ctypes as C, io, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from ffpic_amd import capi, ops, tensors

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["sink", "files", "all"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pictures", type=int, default=256)
ap.add_argument("--files", type=int, default=256)
ap.add_argument("--mixed-files", action="store_true")
ap.add_argument("--allocations", type=int, default=8)
args = ap.parse_args()
L = capi.require_device(0)
import torch
out = {"tool": "bench_tensor_sink"}
SIZES = [(320, 240), (333, 251), (640, 480), (801, 599), (1024, 768), (1280, 720), (1919, 1081), (2048, 1152), (2560, 1440), (3840, 2160)]
FORMATS = [(d, l, o) for d in ("uint8", "float16", "float32") for l in ("CHW", "HWC") for o in ("RGB", "BGR")]
ES = {"uint8": 1, "float16": 2, "float32": 4}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
st = torch.cuda.current_stream().cuda_stream
e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()


def timed(f, k):
    L.ffhip_event_record(e0, st)
    for _ in range(k):
        f()
    L.ffhip_event_record(e1, st)
    capi.check(L.ffhip_stream_sync(st))
    return L.ffhip_event_elapsed_ms(e0, e1) / k


def spread(byte_sizes):
    """every size its place (256-byte aligned) in one of --allocations allocations, dealt round robin -> (tensors kept alive, addresses)"""
    a = max(1, min(args.allocations, len(byte_sizes)))
    fill, where = [0] * a, []
    for i, b in enumerate(byte_sizes):
        where.append((i % a, fill[i % a]))
        fill[i % a] += (b + 255) & ~255
    bufs = [torch.empty(max(f, 256), dtype=torch.uint8, device="cuda") for f in fill]
    return bufs, [bufs[k].data_ptr() + o for k, o in where]


def sink_set(name, dims, cal):
    px = sum(w * h for w, h in dims)
    pitches = [4 * ((w + 15) & ~15) for w, _ in dims]
    src_bufs, src = spread([p * h for p, (_, h) in zip(pitches, dims)])
    for b in src_bufs:
        b.random_(0, 256)
    res = {"pictures": len(dims), "Mpx": round(px / 1e6, 1), "formats": {}}
    for dtype, layout, order in FORMATS:
        es = ES[dtype]
        f = tensors.tensor_format(dtype, layout, order, None if dtype == "uint8" else MEAN, None if dtype == "uint8" else STD)
        out_bufs, dst = spread([3 * w * h * es for w, h in dims])
        arr = (capi.TensorItem * len(dims))()
        for i, (w, h) in enumerate(dims):
            arr[i] = capi.TensorItem(src[i], pitches[i], 0, 0, w, h, dst[i], w if layout == "CHW" else 3 * w, w * h)
        traffic = (4 + 3 * es) * px
        half = (traffic // 2) & ~255                                      # a copy of `half` bytes moves the sink's bytes

        def sink():
            capi.check(L.ffhip_bgra_to_tensor_items(arr, len(dims), C.byref(f), st))

        def copy():
            capi.check(L.ffhip_copy_calibrate(cal[0].data_ptr(), cal[1].data_ptr(), half, st))

        for fn in (sink, copy):
            timed(fn, 2)
        blocks = [(timed(sink, args.reps), timed(copy, args.reps)) for _ in range(2)]
        s_ms, c_ms = blocks[1]
        s_rate, c_rate = traffic / s_ms / 1e6, 2 * half / c_ms / 1e6
        res["formats"][f"{dtype}_{layout}_{order}"] = {"sink_ms": round(s_ms, 3), "sink_GBps": round(s_rate, 1), "copy_ms": round(c_ms, 3),
                                                       "copy_GBps": round(c_rate, 1), "sink_over_copy": round(s_rate / c_rate, 3),
                                                       "Gpx_s": round(px / s_ms / 1e6, 1), "first_block_ms": [round(x, 3) for x in blocks[0]]}
        del out_bufs
    out[name] = res


def sink_part():
    rng = np.random.default_rng(2024)
    sets = {"sink_4k": [(3840, 2160)] * args.pictures, "sink_mixed_1024": [SIZES[int(k)] for k in rng.integers(0, len(SIZES), 1024)]}
    most = max(sum(w * h for w, h in d) for d in sets.values())
    cal = [torch.empty(8 * most + 256, dtype=torch.uint8, device="cuda") for _ in range(2)]
    cal[1].random_(0, 256)
    for name, dims in sets.items():
        sink_set(name, dims, cal)
        torch.cuda.empty_cache()


def make_file(w, h, mode, sub, dri, rng):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 37.0) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / 53.0), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    bio = io.BytesIO()
    kw = dict(quality=85)
    if sub is not None:
        kw["subsampling"] = sub
    if dri:
        kw["restart_marker_rows"] = 1
    Image.fromarray(img).convert(mode).save(bio, "JPEG", **kw)
    return bio.getvalue()


def files_set(name, files):
    n = len(files)
    probes = [ops.jpeg_probe(f) for f in files]
    px = sum(w * h for _, w, h in probes)
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    status = (C.c_int * n)()
    bgra_bufs, bgra = spread([g.width * 4 * g.height for g, _, _ in probes])
    bo = (C.c_void_p * n)(*bgra)
    bp = (C.c_int64 * n)(*[g.width * 4 for g, _, _ in probes])
    calls = {"bgra": lambda: capi.check(L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n, 16, bo, bp, None, status, st))}
    keep = [bgra_bufs]
    for dtype, layout in (("uint8", "CHW"), ("uint8", "HWC"), ("float16", "CHW"), ("float32", "CHW")):
        f = tensors.tensor_format(dtype, layout, "RGB", None if dtype == "uint8" else MEAN, None if dtype == "uint8" else STD)
        tb, dst = spread([3 * w * h * ES[dtype] for _, w, h in probes])
        o = (capi.TensorOut * n)(*[capi.TensorOut(dst[i], w if layout == "CHW" else 3 * w, w * h) for i, (_, w, h) in enumerate(probes)])
        keep.append((f, tb, o))
        calls[f"{dtype}_{layout}"] = (lambda f=f, o=o: capi.check(L.ffhip_jpeg_decode_files_tensor(ptrs, lens, n, 16, C.byref(f), o, None, None, status, st)))

    def wall(fn):
        capi.check(L.ffhip_stream_sync(st))
        t0 = time.perf_counter(); fn(); capi.check(L.ffhip_stream_sync(st))
        return (time.perf_counter() - t0) * 1e3

    for fn in calls.values():
        fn()
    t = {k: [] for k in calls}
    for _ in range(args.reps):                                             # alternating: the same clocks and neighbours for all
        for k, fn in calls.items():
            t[k].append(wall(fn))
    base = min(t["bgra"])
    out[name] = {"files": n, "Mpx": round(px / 1e6, 1), "scan_MB": round(sum(len(f) for f in files) / 1e6, 1),
                 **{k: {"ms": round(min(v), 2), "Gpx_s": round(px / min(v) / 1e6, 1), "over_bgra": round(min(v) / base, 3), "all_ms": [round(x, 1) for x in v]}
                    for k, v in t.items()}}


def files_part():
    rng = np.random.default_rng(2024)
    files_set(f"files_4k420x{args.files}", [make_file(3840, 2160, "RGB", 2, 0, rng)] * args.files)
    if args.mixed_files:
        kinds = [("RGB", 2), ("RGB", 0), ("RGB", 1), ("L", None)]
        protos = [make_file(w, h, mode, sub, dri, rng) for w, h in SIZES for mode, sub in kinds for dri in (0, 1)]
        files_set("files_mixed_1024", [protos[int(k)] for k in rng.integers(0, len(protos), 1024)])


if args.part in ("sink", "all"):
    sink_part()
if args.part in ("files", "all"):
    files_part()
print(json.dumps(out))
