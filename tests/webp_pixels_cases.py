"""What the tests of pixels='libwebp' share (tests/test_webp_pixels_libwebp*.py): the files -- the 81 of tests/golden/webp_libwebp.npz and
those of tests/golden/webp_libwebp_more.npz, each with PIL's RGB -- and ONE witness decode of each, tests/vp8_spec.py with rules=SPEC,
computed once and left unchanged."""
import functools
import json
import os

import numpy as np

import vp8_spec as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SETS = [np.load(os.path.join(GOLDEN, f)) for f in ("webp_libwebp.npz", "webp_libwebp_more.npz")]
NAMES = [str(n) for s in _SETS for n in s["names"]]
CORPUS = [str(n) for n in _SETS[0]["names"]]
REAL = json.load(open(os.path.join(GOLDEN, "webp_libwebp_real.json")))["files"]
assert len(CORPUS) == 81 and len(set(NAMES)) == len(NAMES)


def _set(name):
    return _SETS[0] if name in CORPUS else _SETS[1]


def data_of(name):
    return _set(name)[name + "_bytes"].tobytes()


def pil_rgb(name):
    return _set(name)[name + "_rgb"]


@functools.lru_cache(maxsize=None)
def witness(name):
    return S.decode(data_of(name), S.SPEC)


def real_bytes(name):
    return open(os.path.join(GOLDEN, name + ".webp"), "rb").read()


def first_plane_difference(got, want, names="yuv"):
    """'plane y, macroblock (x, y), sample (col, row): got g, want w' for the first plane that differs, or None"""
    for k, g, w in zip(names, got, want):
        if g.shape != w.shape:
            return f"plane {k}: shape {g.shape}, want {w.shape}"
        if not np.array_equal(g, w):
            r, c = (int(v) for v in np.argwhere(g != w)[0])
            sz = 16 if k == "y" else 8
            return f"plane {k}, macroblock ({c // sz}, {r // sz}), sample ({c}, {r}): got {int(g[r, c])}, want {int(w[r, c])}; {int((g != w).sum())} differ"
    return None
