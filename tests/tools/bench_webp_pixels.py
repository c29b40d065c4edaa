"""What pixels='libwebp' costs: the default rule and the libwebp rule measured ALTERNATELY in one session, three rounds
each, median / min / max of the rounds' figures (a round's figure is the median of `--reps` calls after one warm-up call).

  file call   ffhip_webp_decode_files_device against ffhip_webp_decode_files_device_ex with FFHIP_WEBP_PIXELS_LIBWEBP on copies of
              tests/golden/file_1080p_q75.webp: 256 with 16 host threads (FFHIP_WEBP_GPU_ENTROPY=0), 1 024 with the kernels (=1).  Wall clock
              around the synchronising call.  The bar: the libwebp median within 3 % of the default's, or within the default's own spread
              over its rounds ((max - min) / median) where that is wider.
  back half   ffhip_vp8_decode_items against the rule's residual + frames + colour launches on the same pre-parsed frames (no bar: a ratio)
  colour      ffhip_yuv420_to_bgra against k_vp8_upsample_color on the same planes: GB/s of both (1.5 bytes in, 4 out per pixel) and the ratio

    python tests/tools/bench_webp_pixels.py [--file-sets 256:0,1024:1] [--back 256,1024] [--colour 256] [--rounds 3] [--reps 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ffpic_amd import capi, ops  # noqa: E402

LIBWEBP = capi.FFHIP_WEBP_PIXELS_LIBWEBP


def median_of_calls(call, reps):
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:] or times)) * 1e3


def alternate(calls, rounds, reps):
    """calls: {label: callable}; -> {label: [a figure per round]}, the labels taking turns inside every round"""
    out = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            out[k].append(median_of_calls(call, reps))
    return out


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))


def file_calls(L, big, copies, threads):
    files = [big] * copies
    w, h, c, r = ops.webp_probe(big, pixels="libwebp")
    assert (c, r) == ops.webp_probe(big)[2:]
    dout = ops.DeviceBuffer(nbytes=copies * 64 * c * 16 * r)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * copies)(*[dout.ptr + i * 64 * c * 16 * r for i in range(copies)])
    pitch = (C.c_int64 * copies)(*[64 * c] * copies)
    status = (C.c_int * copies)()
    keep = (dout, bufs)
    return {"reference": lambda: capi.check(L.ffhip_webp_decode_files_device(ptrs, lens, copies, threads, outs, pitch, None, status, None), "decode"),
            "libwebp": lambda: capi.check(L.ffhip_webp_decode_files_device_ex(ptrs, lens, copies, threads, outs, pitch, None, LIBWEBP, None, status, None), "decode_ex")}, keep


def back_half_calls(L, big, copies):
    calls, keep = {}, []
    for rule in ("reference", "libwebp"):
        p = ops.webp_parse(big, pixels=rule)
        n_mb = p["mbcols"] * p["mbrows"]
        d = {k: ops.DeviceBuffer(np.ascontiguousarray(p[k])) for k in ("levels", "mbinfo", "resmap")}
        modes = ops.DeviceBuffer(np.ascontiguousarray(np.tile(p["modes"], (copies, 1))))       # the rule writes byte [19]: a copy per frame
        dout = ops.DeviceBuffer(nbytes=copies * 64 * p["mbcols"] * 16 * p["mbrows"])
        items = (capi.Vp8Item * copies)()
        for i in range(copies):
            it = items[i]
            it.mbcols, it.mbrows = p["mbcols"], p["mbrows"]
            it.d_modes, it.d_levels, it.d_mbinfo = modes.ptr + i * 20 * n_mb, d["levels"].ptr, d["mbinfo"].ptr
            it.d_resmap = d["resmap"].ptr if rule == "reference" else None
            for s in range(4):
                for k in range(8):
                    it.quant[s][k] = int(p["quant"][s, k])
            it.filter_type = p["filter_type"]
            for k, v in enumerate(p["filters"].reshape(-1)):
                it.filters[k] = int(v)
            it.d_bgra, it.pitch = dout.ptr + i * 64 * p["mbcols"] * 16 * p["mbrows"], 64 * p["mbcols"]
        display = (capi.Size * copies)(*[capi.Size(p["width"], p["height"])] * copies)
        keep.append((d, modes, dout, items, display))
        if rule == "reference":
            calls[rule] = lambda items=items: (capi.check(L.ffhip_vp8_decode_items(items, copies, None), "items"), capi.sync(None))
        else:
            calls[rule] = lambda items=items, display=display: (capi.check(L.ffhip_debug_vp8_decode_items_libwebp(items, copies, display, None), "items, libwebp"),
                                                                capi.sync(None))
    return calls, keep


def colour_calls(L, copies, cols=120, rows=68):
    rng = np.random.default_rng(1)
    n_mb = cols * rows
    y, u, v = (ops.DeviceBuffer(rng.integers(0, 256, copies * k * n_mb, dtype=np.uint8)) for k in (256, 64, 64))
    dout = ops.DeviceBuffer(nbytes=copies * 1024 * n_mb)
    pitch, stride = 64 * cols, 1024 * n_mb
    keep = (y, u, v, dout)
    return {"reference": lambda: (capi.check(L.ffhip_yuv420_to_bgra(dout.ptr, pitch, y.ptr, u.ptr, v.ptr, 16 * cols, 8 * cols, rows, cols, copies, 256 * n_mb, 64 * n_mb, stride,
                                                                    None), "yuv420"), capi.sync(None)),
            "libwebp": lambda: (capi.check(L.ffhip_debug_vp8_upsample_color(y.ptr, u.ptr, v.ptr, 16 * cols, 8 * cols, 16 * cols, 16 * rows, copies, 256 * n_mb, 64 * n_mb,
                                                                            dout.ptr, pitch, stride, None), "upsample"), capi.sync(None))}, keep, copies * 256 * n_mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file-sets", default="256:0,1024:1", help="copies:FFHIP_WEBP_GPU_ENTROPY, ...")
    ap.add_argument("--back", default="256,1024")
    ap.add_argument("--colour", default="256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.require_device(0)
    big = open(os.path.join(ROOT, "tests", "golden", "file_1080p_q75.webp"), "rb").read()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for spec in [s for s in a.file_sets.split(",") if s]:
        copies, entropy = (int(x) for x in spec.split(":"))
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
        calls, keep = file_calls(L, big, copies, a.threads)
        r = alternate(calls, a.rounds, a.reps)
        ref, lw = stats(r["reference"]), stats(r["libwebp"])
        bar = max(0.03, (ref["max"] - ref["min"]) / ref["median"])
        emit(what=f"file call, 1080p x{copies}", front_end="kernels" if entropy else f"{a.threads} host threads", ms_reference=ref, ms_libwebp=lw,
             ratio=round(lw["median"] / ref["median"], 4), bar=round(1 + bar, 4), within_bar=bool(lw["median"] <= ref["median"] * (1 + bar)))
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", None)
        del calls, keep
    for copies in [int(x) for x in a.back.split(",") if x]:
        calls, keep = back_half_calls(L, big, copies)
        r = alternate(calls, a.rounds, a.reps)
        ref, lw = stats(r["reference"]), stats(r["libwebp"])
        emit(what=f"back half alone, 1080p x{copies}", ms_reference=ref, ms_libwebp=lw, ratio=round(lw["median"] / ref["median"], 4))
        del calls, keep
    for copies in [int(x) for x in a.colour.split(",") if x]:
        calls, keep, pixels = colour_calls(L, copies)
        r = alternate(calls, a.rounds, a.reps)
        ref, lw = stats(r["reference"]), stats(r["libwebp"])
        gbs = lambda ms: round(pixels * 5.5 / (ms * 1e-3) / 1e9, 1)
        emit(what=f"colour alone, 1920x1088 x{copies}", ms_yuv420_to_bgra=ref, ms_upsample_color=lw, gb_per_s_yuv420_to_bgra=gbs(ref["median"]),
             gb_per_s_upsample_color=gbs(lw["median"]), ratio=round(lw["median"] / ref["median"], 4))
        del calls, keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
