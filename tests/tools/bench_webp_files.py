"""Files -> device pixels for lossy WebP: the large real-encoder stream (tests/golden/file_1080p_q75.webp) at 1, 16, 256 and 1024
copies and the mixed fixture set.  Per set, in the same run: the device front end (FFHIP_WEBP_GPU_ENTROPY=1), the host-thread front
end (=0), the unforced call (it should match the faster of the two), and the BACK HALF ALONE -- the same files parsed once on the host,
their arrays uploaded, then only ffhip_vp8_decode_items timed.  Once per run: the host parser on one core and the reference's own
WEBP_load on one core for the 1080p frame (through oracle/_ref in a child process, as the fixture generator calls it; the row says so
when oracle/_ref has not been built).  Each figure is the median of `--reps` calls after one warm-up call, wall clock around the
synchronising call; one JSON line each.

    python tests/tools/bench_webp_files.py [--copies 1,16,256,1024] [--reps 5] [--threads 16] [--front device,host_threads,unforced,back_half] [--no-mixed] [--out FILE]"""
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

GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed_call(L, files, n_threads, reps):
    n = len(files)
    probes = [ops.webp_probe(f) for f in files]
    offs, total = [], 0
    for w, h, c, r in probes:
        offs.append(total)
        total += 64 * c * 16 * r
    dout = ops.DeviceBuffer(nbytes=total)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * n)(*[dout.ptr + o for o in offs])
    pitch = (C.c_int64 * n)(*[64 * p[2] for p in probes])
    status = (C.c_int * n)()
    times = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        capi.check(L.ffhip_webp_decode_files_device(ptrs, lens, n, n_threads, outs, pitch, None, status, None), "decode")
        times.append(time.perf_counter() - t0)
    pixels = sum(256 * p[2] * p[3] for p in probes)
    t = float(np.median(times[1:] or times))   # --reps 0: the one (cold) call, for a kernel trace
    return t, pixels


def back_half(L, files, n_threads, reps):
    """ffhip_vp8_decode_items alone on the pre-parsed arrays of `files` (distinct files are parsed once, every copy gets its own output)"""
    parsed = {}
    for f in files:
        if id(f) not in parsed:
            p = ops.webp_parse(f)
            parsed[id(f)] = (p, {k: ops.DeviceBuffer(np.ascontiguousarray(p[k])) for k in ("modes", "levels", "mbinfo", "resmap")})
    total = sum(64 * parsed[id(f)][0]["mbcols"] * 16 * parsed[id(f)][0]["mbrows"] for f in files)
    dout = ops.DeviceBuffer(nbytes=total)
    items, off, pixels = [], 0, 0
    for f in files:
        p, d = parsed[id(f)]
        it = capi.Vp8Item()
        it.mbcols, it.mbrows = p["mbcols"], p["mbrows"]
        it.d_modes, it.d_levels, it.d_mbinfo, it.d_resmap = d["modes"].ptr, d["levels"].ptr, d["mbinfo"].ptr, d["resmap"].ptr
        for s in range(4):
            for k in range(8):
                it.quant[s][k] = int(p["quant"][s, k])
        it.filter_type = p["filter_type"]
        for k, v in enumerate(p["filters"].reshape(-1)):
            it.filters[k] = int(v)
        it.d_bgra, it.pitch = dout.ptr + off, 64 * p["mbcols"]
        off += 64 * p["mbcols"] * 16 * p["mbrows"]
        pixels += 256 * p["mbcols"] * p["mbrows"]
        items.append(it)
    arr = (capi.Vp8Item * len(items))(*items)
    times = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        capi.check(L.ffhip_vp8_decode_items(arr, len(items), None), "items")
        capi.sync(None)
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:] or times)), pixels


REF_CHILD = r"""
import ctypes as C, sys, time, os
R = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
R.file_ops_init.restype = None
R.file_probe.restype = C.c_void_p
R.file_probe.argtypes = [C.c_char_p]
R.file_load.restype = C.c_void_p
R.file_load.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
R.file_ops_init()
path = sys.argv[2].encode()
ops = R.file_probe(path)
ts = []
for k in range(4):
    t0 = time.perf_counter()
    assert R.file_load(ops, path, 0)
    ts.append(time.perf_counter() - t0)
print(sorted(ts[1:])[1] * 1e3, flush=True)
os._exit(0)
"""


def reference_ms(path):
    """the reference's file_load -> WEBP_load on one core, median of 3 after a warm-up, in a child process; None + reason when it cannot run"""
    import subprocess
    so = os.path.join(ROOT, "oracle", "_ref", "libffpic_ref.so")
    if not os.path.exists(so):
        return None, "oracle/_ref is not built here"
    r = subprocess.run([sys.executable, "-c", REF_CHILD, so, path], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or not r.stdout.strip():
        return None, f"the reference's loader ended with status {r.returncode}"
    return float(r.stdout.split()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--front", default="device,host_threads,unforced,back_half")
    ap.add_argument("--no-mixed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.require_device(0)
    big = open(os.path.join(GOLDEN, "file_1080p_q75.webp"), "rb").read()
    front = np.load(os.path.join(GOLDEN, "webp_front.npz"))
    mixed = [open(os.path.join(GOLDEN, str(n) + ".webp"), "rb").read() for n in front["names"]]
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    t0 = time.perf_counter()
    for _ in range(3):
        ops.webp_parse(big)
    emit(what="host parser, one core, one 1080p frame", ms=round((time.perf_counter() - t0) / 3 * 1e3, 3))
    ms, why = reference_ms(os.path.join(GOLDEN, "file_1080p_q75.webp"))
    emit(what="reference WEBP_load, one core, one 1080p frame", ms=None if ms is None else round(ms, 3), **({"not_measured": why} if why else {}))
    sets = [(f"1080p x{c}", [big] * c) for c in [int(x) for x in a.copies.split(",")]] + ([] if a.no_mixed else [("mixed fixtures x8", mixed * 8)])
    fronts = a.front.split(",")
    for label, files in sets:
        for front_end, val in (("device", "1"), ("host_threads", "0"), ("unforced", None)):
            if front_end not in fronts:
                continue
            capi.setenv("FFHIP_WEBP_GPU_ENTROPY", val)
            t, pixels = timed_call(L, files, a.threads, a.reps)
            emit(what=label, front_end=front_end, files=len(files), ms=round(t * 1e3, 3), gpixel_per_s=round(pixels / t / 1e9, 3), threads=a.threads,
                 parts_device_host=list(ops.webp_last_parts()))
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", None)
        if "back_half" in fronts:
            t, pixels = back_half(L, files, a.threads, a.reps)
            emit(what=label, front_end="none: ffhip_vp8_decode_items on pre-parsed arrays", files=len(files), ms=round(t * 1e3, 3), gpixel_per_s=round(pixels / t / 1e9, 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
