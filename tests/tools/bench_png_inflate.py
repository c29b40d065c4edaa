#!/usr/bin/env python3
"""bench_png.py, unedited, over the device inflate, with ffhip_debug_png_inflate read beside every
ffhip_debug_png_times the tool reads: run it with FFHIP_PNG_INFLATE_GPU=1, arguments as bench_png.py's.  Prints bench_png.py's JSON line,
then one of its own: per timed file call, in the tool's order (set by set, round by round, rep by rep), [files inflated on the device,
files inflated on the host, compressed bytes uploaded, milliseconds of k_inflate and its copy back]."""
import json, os, runpy, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ffpic_amd import ops

seen = []
times = ops.png_times


def both():
    seen.append(ops.png_inflate_last())
    return times()


ops.png_times = both
sys.argv = [os.path.join(HERE, "bench_png.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
finally:
    print(json.dumps({"tool": "bench_png_inflate", "inflate_last_per_timed_call": [list(s) for s in seen]}))
