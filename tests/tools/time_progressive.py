#!/usr/bin/env python3
"""Progressive JPEG front ends against each other and against the baseline twins; prints one JSON line.

  --set 1080p256 | 1080p1024 | thumb4096   256 / 1 024 files of 1920x1080 4:2:0, or 4 096 thumbnails of 256x256: a handful of distinct PIL
                                           pictures, each saved progressive and baseline under the same arguments, repeated
  --modes a,b,c,d   a  the baseline twins through ffhip_jpeg_decode_files_mixed_device (the call as it was)
                    b  the progressive files, host-thread front end (FFHIP_JPEG_PROGRESSIVE_GPU=0), 16 threads
                    c  the progressive files, device front end (=1)
                    d  c at 1/8 size (k_max = 0: the DC scans only)
                    e  b at 1/8 size
  --lib PATH        another build of libffpic_hip.so (mode a only: the parent commit's has none of the new calls)
Wall time of the whole call, which ends in a stream synchronise; --warmup calls first, then --reps, median / min / max in ms.  The output
pictures live in one device allocation made before the clock starts.  Needs PIL."""
import argparse, ctypes as C, io, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--set", default="1080p256", choices=["1080p256", "1080p1024", "thumb4096"])
ap.add_argument("--modes", default="a,b,c,d")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--lib", default=os.path.join(ROOT, "ffpic_amd", "libffpic_hip.so"))
args = ap.parse_args()
from PIL import Image

L = C.CDLL(args.lib, mode=C.RTLD_GLOBAL)
vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
L.ffhip_malloc.argtypes, L.ffhip_malloc.restype = [sz], vp
L.ffhip_stream_sync.argtypes = [vp]
L.ffhip_jpeg_decode_files_mixed_device.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
if L.ffhip_device_count() < 1 or L.ffhip_init(0):
    sys.exit("no gfx950 device: nothing to measure")

n, (w, h) = {"1080p256": (256, (1920, 1080)), "1080p1024": (1024, (1920, 1080)), "thumb4096": (4096, (256, 256))}[args.set]
rng = np.random.default_rng(414)
protos = []
for k in range(6):
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    pair = []
    for progressive in (True, False):
        bio = io.BytesIO()
        Image.fromarray(img).save(bio, "JPEG", quality=85, subsampling=2, progressive=progressive)
        pair.append(bio.getvalue())
    protos.append(pair)
pick = rng.integers(0, len(protos), n)
sets = {"prog": [protos[k][0] for k in pick], "base": [protos[k][1] for k in pick]}
cw, ch = -(-w // 16) * 16, -(-h // 16) * 16
pitch = cw * 4
d_out = L.ffhip_malloc(n * pitch * ch)
if not d_out:
    sys.exit("device allocation failed")


def arrays(files, denom):
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    return dict(bufs=bufs, ptrs=(vp * n)(*[b.ctypes.data for b in bufs]), lens=(sz * n)(*[b.size for b in bufs]),
                outs=(vp * n)(*[d_out + i * pitch * ch for i in range(n)]), pitch=(C.c_int64 * n)(*([pitch // denom] * n)),
                denom=(ci * n)(*([denom] * n)), status=(ci * n)())


def timed(call):
    for _ in range(args.warmup):
        call()
    out = []
    for _ in range(args.reps):
        L.ffhip_stream_sync(None)
        t0 = time.perf_counter()
        rc = call()
        L.ffhip_stream_sync(None)
        out.append((time.perf_counter() - t0) * 1e3)
        if rc:
            sys.exit(f"call failed: {rc}")
    return {"median_ms": round(statistics.median(out), 2), "min_ms": round(min(out), 2), "max_ms": round(max(out), 2), "all_ms": [round(x, 1) for x in out]}


res = {"tool": "time_progressive", "set": args.set, "files": n, "lib": os.path.relpath(args.lib, ROOT), "threads": args.threads,
       "prog_MB": round(sum(len(f) for f in sets["prog"]) / 1e6, 1), "base_MB": round(sum(len(f) for f in sets["base"]) / 1e6, 1)}
for mode in args.modes.split(","):
    if mode == "a":
        A = arrays(sets["base"], 1)
        res["a_baseline"] = timed(lambda: L.ffhip_jpeg_decode_files_mixed_device(A["ptrs"], A["lens"], n, args.threads, A["outs"], A["pitch"], None, A["status"], None))
        continue
    L.ffhip_jpeg_decode_files_mixed_device_ex.argtypes = [vp, vp, ci, ci, vp, vp, vp, C.c_uint, vp, vp, vp]
    os.environ["FFHIP_JPEG_PROGRESSIVE_GPU"] = "0" if mode in "be" else "1"
    L.ffhip_reload_env()
    A = arrays(sets["prog"], 8 if mode in "de" else 1)
    name = {"b": "b_progressive_host", "c": "c_progressive_device", "d": "d_progressive_device_eighth", "e": "e_progressive_host_eighth"}[mode]
    res[name] = timed(lambda: L.ffhip_jpeg_decode_files_mixed_device_ex(A["ptrs"], A["lens"], n, args.threads, A["outs"], A["pitch"],
                                                                         A["denom"] if mode in "de" else None, 1, None, A["status"], None))
    last = (ci * 5)()
    L.ffhip_debug_progressive_last(last)
    res[name]["last"] = list(last)
print(json.dumps(res))
