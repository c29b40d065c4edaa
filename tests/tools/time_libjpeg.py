#!/usr/bin/env python3
"""libjpeg's pixel rule against the reference's on the device; prints one JSON line.

  --set 1080p420 | 1080p444 | thumb420   256 x 1920x1080 4:2:0, 256 x 1920x1080 4:4:4, 4 096 x 256x256 4:2:0
  --part items      ffhip_jpeg_recon_items_libjpeg and ffhip_jpeg_recon_items on the same items (synthetic planes, a few distinct pictures
                    uploaded once per item so that no item reads another's cache lines), ALTERNATING in one session, device events around each
                    call; beside them a streaming copy of the output's size (ffhip_copy_calibrate), the rate the kernels are held against
  --part files      ffhip_jpeg_decode_files_mixed_device_ex with and without FFHIP_JPEG_PIXELS_LIBJPEG on PIL-written files of the set's size
                    (a few distinct pictures, repeated), alternating, wall time of the whole call (it ends in a stream synchronise)
  --lib PATH        another build of libffpic_hip.so: one without the new calls (the parent commit's) runs the default path alone
--warmup calls of each first, then --reps of each; median / min / max in ms.  Needs PIL for --part files."""
import argparse, ctypes as C, io, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--set", default="1080p420", choices=["1080p420", "1080p444", "thumb420"])
ap.add_argument("--part", default="items", choices=["items", "files"])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--lib", default=os.path.join(ROOT, "ffpic_amd", "libffpic_hip.so"))
args = ap.parse_args()

from ffpic_amd import capi, synth
L = C.CDLL(args.lib, mode=C.RTLD_GLOBAL)
vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
L.ffhip_malloc.argtypes, L.ffhip_malloc.restype = [sz], vp
L.ffhip_stream_sync.argtypes = [vp]
L.ffhip_memcpy_h2d.argtypes = [vp, vp, sz, vp]
L.ffhip_event_create.restype = vp
L.ffhip_event_record.argtypes = [vp, vp]
L.ffhip_event_elapsed_ms.argtypes, L.ffhip_event_elapsed_ms.restype = [vp, vp], C.c_float
L.ffhip_copy_calibrate.argtypes = [vp, vp, sz, vp]
L.ffhip_jpeg_recon_items.argtypes = [C.POINTER(capi.JpegItem), ci, vp]
L.ffhip_jpeg_decode_files_mixed_device_ex.argtypes = [vp, vp, ci, ci, vp, vp, vp, C.c_uint, vp, vp, vp]
have_new = hasattr(L, "ffhip_jpeg_recon_items_libjpeg")
if have_new:
    L.ffhip_jpeg_recon_items_libjpeg.argtypes = [C.POINTER(capi.JpegItem), C.POINTER(capi.Size), ci, vp]
if L.ffhip_device_count() < 1 or L.ffhip_init(0):
    sys.exit("no gfx950 device: nothing to measure")

n, (w, h), (hs, vs) = {"1080p420": (256, (1920, 1080), (2, 2)), "1080p444": (256, (1920, 1080), (1, 1)), "thumb420": (4096, (256, 256), (2, 2))}[args.set]
mc, mr = -(-w // (8 * hs)), -(-h // (8 * vs))
geom = capi.jpeg_geom(mc, mr, 3, hs, vs)
cw, ch = geom.width, geom.height
pitch = cw * 4
res = {"tool": "time_libjpeg", "set": args.set, "part": args.part, "pictures": n, "lib": os.path.relpath(args.lib, ROOT), "new_calls": have_new}


def alloc(nbytes):
    p = L.ffhip_malloc(nbytes)
    if not p:
        sys.exit("device allocation failed")
    return p


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternate(calls, timer):
    """{name: call} -> {name: summary}: warm-up of each, then reps rounds in which each is timed once, in turn"""
    for _ in range(args.warmup):
        for c in calls.values():
            timer(c)
    out = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, c in calls.items():
            out[k].append(timer(c))
    return {k: summary(v) for k, v in out.items()}


d_out = alloc(n * pitch * ch)
if args.part == "items":
    protos = [synth.coef_batch(1, mc, mr, 3, hs, vs, first=k) for k in range(6)]
    q = synth.quant_tables()
    d_q = alloc(q.nbytes)
    L.ffhip_memcpy_h2d(d_q, q.ctypes.data, q.nbytes, None)
    yb, cb = protos[0][0].nbytes, protos[0][1].nbytes
    d_planes = alloc(n * (yb + 2 * cb))
    items = (capi.JpegItem * n)()
    shown = (capi.Size * n)(*([capi.Size(w, h)] * n))
    for i in range(n):
        cy, cu, cv = protos[i % len(protos)]
        base = d_planes + i * (yb + 2 * cb)
        for off, a in ((0, cy), (yb, cu), (yb + cb, cv)):
            L.ffhip_memcpy_h2d(base + off, a.ctypes.data, a.nbytes, None)
        it = items[i]
        it.geom = geom
        it.d_coef_y, it.d_coef_u, it.d_coef_v, it.d_quant, it.d_bgra, it.pitch = base, base + yb, base + yb + cb, d_q, d_out + i * pitch * ch, pitch
    L.ffhip_stream_sync(None)
    e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()

    def timer(call):
        L.ffhip_event_record(e0, None)
        rc = call()
        L.ffhip_event_record(e1, None)
        L.ffhip_stream_sync(None)
        if rc:
            sys.exit(f"call failed: {rc}")
        return L.ffhip_event_elapsed_ms(e0, e1)

    d_copy = alloc(n * pitch * ch)
    calls = {"reference_items": lambda: L.ffhip_jpeg_recon_items(items, n, None),
             "copy_of_output_size": lambda: L.ffhip_copy_calibrate(d_copy, d_out, n * pitch * ch, None)}
    if have_new:
        calls["libjpeg_items"] = lambda: L.ffhip_jpeg_recon_items_libjpeg(items, shown, n, None)
    res.update(alternate(calls, timer))
    px = n * cw * ch
    coef_bytes = n * (yb + 2 * cb)
    plane_bytes = coef_bytes // 2
    moved = {"reference_items": coef_bytes + 4 * px, "libjpeg_items": coef_bytes + 2 * plane_bytes + 4 * px, "copy_of_output_size": 8 * px}
    for k in calls:
        res[k]["bytes_per_pixel"] = round(moved[k] / px, 2)
        res[k]["GB_per_s"] = round(moved[k] / res[k]["median_ms"] / 1e6, 1)
    for k in ("reference_items", "libjpeg_items"):
        if k in res:
            res[k]["share_of_copy_rate"] = round(res[k]["GB_per_s"] / res["copy_of_output_size"]["GB_per_s"], 3)
else:
    from PIL import Image
    rng = np.random.default_rng(416)
    protos = []
    for k in range(6):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / (29.0 + k)) * np.cos(yy / 23.0), 128 + 90 * np.cos(xx / 11.0 + yy / (41.0 + 3 * k)), (xx * 255 / w + yy * 255 / h) / 2], axis=2)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        bio = io.BytesIO()
        Image.fromarray(img).save(bio, "JPEG", quality=85, subsampling={(2, 2): 2, (1, 1): 0}[(hs, vs)])
        protos.append(bio.getvalue())
    files = [protos[k] for k in rng.integers(0, len(protos), n)]
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    ptrs, lens = (vp * n)(*[b.ctypes.data for b in bufs]), (sz * n)(*[b.size for b in bufs])
    outs, pitches, status = (vp * n)(*[d_out + i * pitch * ch for i in range(n)]), (C.c_int64 * n)(*([pitch] * n)), (ci * n)()

    def timer(call):
        L.ffhip_stream_sync(None)
        t0 = time.perf_counter()
        rc = call()
        L.ffhip_stream_sync(None)
        if rc:
            sys.exit(f"call failed: {rc}")
        return (time.perf_counter() - t0) * 1e3

    calls = {"reference_files": lambda: L.ffhip_jpeg_decode_files_mixed_device_ex(ptrs, lens, n, args.threads, outs, pitches, None, 0, None, status, None)}
    if have_new:
        calls["libjpeg_files"] = lambda: L.ffhip_jpeg_decode_files_mixed_device_ex(ptrs, lens, n, args.threads, outs, pitches, None, 0x10, None, status, None)
    res["files_MB"] = round(sum(len(f) for f in files) / 1e6, 1)
    res.update(alternate(calls, timer))
print(json.dumps(res))
