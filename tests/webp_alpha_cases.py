"""The shared list of lossy WebP files with an alpha plane (webp_alpha_writer.py writes them from known planes around a carrier's colour).
Small pictures: the code goes wrong at edges -- a band's last row and the next band's first, a row's last partial chunk of 16 samples, a
merge group of four that the width cuts, column 0 and row 0 under every filter -- and not in the middle.  A list, no cross product:
build() gives the same files in the same order every time."""
import functools
from collections import namedtuple

import numpy as np

import vp8_writer
import vp8l_writer as W
import webp_alpha_writer as A
import webp_pixels_cases

# plane: the answer key, uint8 [h][w]; None: the file stays opaque.  kind: what the lossless stream holds ('' for a raw plane)
Case = namedtuple("Case", "name data plane compression filter pre kind")
Damaged = namedtuple("Damaged", "name data")
EINVAL = -22
CHUNK = 16                                                        # k_webp_alpha_unfilter's samples a step
WIDTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 50)
HEIGHTS = (1, 2, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def carrier(w, h):
    return vp8_writer.keyframe(w, h, 7 + w + 3 * h, valid=True)


def noise(rng, h, w):
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def ramps(h, w):
    """slow ramps that reach 0 and 255, so that the gradient's clip matters both ways"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return np.clip(np.where((x // 3 + y // 5) % 2 == 0, x * 40 + y * 9 - 30, 290 - y * 7 - x * 25), 0, 255).astype(np.uint8)


def levels4(rng, h, w):
    return (rng.integers(0, 4, (h, w)) * 85).astype(np.uint8)


def predictor(rng, h, w):
    return {"type": W.PREDICTOR, "bits": 2, "image": rng.integers(0, 14, (W.sub(h, 2), W.sub(w, 2))).astype(np.uint32) << 8}


PALETTE4 = [0xff000000 | (v << 8) for v in (0, 85, 170, 255)]


def indexing(plane, f):
    """colour indexing over the values the STORED plane has: four to a word without a filter, two with one (up to seven values)"""
    return {"type": W.COLOR_INDEXING, "palette": [0xff000000 | (int(v) << 8) for v in np.unique(A.filter_plane(plane, f))]}


ONE_SYMBOL = {(0, 1): {"simple": (0,)}, (0, 2): {"simple": (0,)}, (0, 3): {"simple": (255,)}, (0, 4): {"simple": (0,)}}


def build():
    rng = np.random.default_rng(20260)
    cases = []

    def add(name, w, h, plane, compression=A.RAW, filter=A.NONE, pre=0, kind="", key=True, car=None, **how):
        data = A.wrap(car or carrier(w, h), plane, compression, filter, pre, **how)
        cases.append(Case(name, data, plane if key else None, compression, filter, pre, kind))

    # every width meets every filter, raw and lossless; the heights take turns
    for k, w in enumerate(WIDTHS):
        for f in range(4):
            h = (3, 2, 5, 1)[(k + f) % 4]
            add(f"w{w}-h{h}-raw-f{f}", w, h, noise(rng, h, w), A.RAW, f)
            add(f"w{w}-h{h}-lossless-f{f}", w, h, ramps(h, w) if f == 3 else noise(rng, h, w), A.LOSSLESS, f, kind="plain")
    # every height boundary meets every filter: one, two and three band levels
    for h in HEIGHTS:
        for f in range(4):
            w = 5 if f != 2 else 17
            add(f"h{h}-w{w}-raw-f{f}", w, h, ramps(h, w) if f == 3 else noise(rng, h, w), A.RAW, f)
            add(f"h{h}-w{w}-lossless-f{f}", w, h, noise(rng, h, w), A.LOSSLESS, f, kind="plain")
    # what a lossless stream may hold, each under each filter
    for f in range(4):
        w, h = 17 + f, 9
        add(f"predictor-f{f}", w, h, noise(rng, h, w), A.LOSSLESS, f, kind="predictor", transforms=[predictor(rng, h, w)])
        a = levels4(rng, h, w)
        add(f"palette-f{f}", w, h, a, A.LOSSLESS, f, kind="palette", transforms=[indexing(a, f)])
        add(f"cache-f{f}", w, h, levels4(rng, h, w), A.LOSSLESS, f, kind="cache", cache_bits=3)
    add("predictor-three-levels", 33, 130, noise(rng, 130, 33), A.LOSSLESS, A.GRADIENT, kind="predictor", transforms=[predictor(rng, 130, 33)])
    a = levels4(rng, 5, 9)
    add("palette-one-symbol-codes", 9, 5, a, A.LOSSLESS, A.HORIZONTAL, kind="palette", transforms=[indexing(a, A.HORIZONTAL)], codes=ONE_SYMBOL)
    add("pre-processing-1-raw", 6, 4, (noise(rng, 4, 6) >> 4) * 17, A.RAW, A.VERTICAL, pre=1)
    add("pre-processing-1-lossless", 6, 4, (noise(rng, 4, 6) >> 4) * 17, A.LOSSLESS, A.NONE, pre=1, kind="plain")
    # the container: a chunk of odd size and its padding byte, a raw plane longer than the picture, an unknown chunk in front
    add("odd-chunk-size", 4, 3, noise(rng, 3, 4), A.RAW, A.GRADIENT)
    add("raw-longer", 5, 3, noise(rng, 3, 5), A.RAW, A.HORIZONTAL, trailing=b"abc")
    add("unknown-chunk-in-front", 5, 3, noise(rng, 3, 5), A.RAW, A.VERTICAL, extra=[(b"XMP ", b"odd")])
    # colour from real encoders' streams
    for name in ("pil_50x37_q30", "pil_17x16_q50"):
        car = webp_pixels_cases.real_bytes(name)
        w, h = A.frame_size(A.vp8_chunk(car))
        add(f"{name}-gradient", w, h, ramps(h, w), A.LOSSLESS, A.GRADIENT, kind="plain", car=car)
    # files that stay opaque
    add("flag-clear", 5, 3, noise(rng, 3, 5), A.RAW, A.HORIZONTAL, key=False, vp8x_alpha=False)
    add("no-alph", 5, 3, None, key=False)
    add("no-vp8x", 5, 3, noise(rng, 3, 5), A.RAW, key=False, vp8x=False)              # PIL refuses these two; named deviations
    add("alph-behind-vp8", 5, 3, noise(rng, 3, 5), A.RAW, key=False, alph_behind=True)
    cases.append(Case("plain-carrier", carrier(17, 5), None, 0, 0, 0, ""))
    return cases


PIL_REFUSES = ("no-vp8x", "alph-behind-vp8")                      # opaque here, refused there


def lenient_end():
    """(file, None): colour indexing alone, one-symbol red, blue and alpha codes, the chunk cut inside the LAST token -- accepted, the
    missing bits read as 0; the witness and PIL say what the plane is"""
    rng = np.random.default_rng(11)
    payload = A.alph_payload(levels4(rng, 5, 9), A.LOSSLESS, A.NONE, transforms=[{"type": W.COLOR_INDEXING, "palette": PALETTE4}], codes=ONE_SYMBOL)
    return A.wrap(carrier(9, 5), payload=payload[:-1])


def damaged():
    rng = np.random.default_rng(8)
    w, h = 7, 5
    car, a = carrier(w, h), noise(rng, h, w)
    out = []

    def add(name, **how):
        out.append(Damaged(name, A.wrap(car, a, **how)))

    add("raw-short", payload=A.alph_payload(a)[:-1])
    add("payload-empty", payload=b"")
    add("compression-2", header=2)
    add("compression-3", header=3)
    add("pre-processing-2", header=0x20)
    add("reserved-bit-6", header=0x40)
    add("reserved-bit-7", header=0x80)
    good = A.alph_payload(a, A.LOSSLESS, A.HORIZONTAL)
    add("lossless-truncated", payload=good[:len(good) // 2])
    add("lossless-last-byte-cut", payload=good[:-1])
    add("lossless-stream-empty", payload=good[:1])
    add("lossless-over-subscribed", compression=A.LOSSLESS, codes={(0, 1): {"lengths": [7] * 256}})
    add("lossless-transform-twice", payload=good[:1] + bytes([0b1101101]) + good[1:])   # add-green, add-green
    pal = A.alph_payload(levels4(rng, h, w), A.LOSSLESS, A.NONE, transforms=[{"type": W.COLOR_INDEXING, "palette": PALETTE4}], codes=ONE_SYMBOL)
    add("one-symbol-codes-cut-two-bytes", payload=pal[:-2])
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(build())


@functools.lru_cache(maxsize=None)
def damaged_cases():
    return tuple(damaged())


def levels_of(c):
    """launches of k_webp_alpha_unfilter a lone case takes"""
    return (c.plane.shape[0] + 63) // 64 if c.plane is not None and c.filter else 0


def mangled(sources):
    """[(name, file)]: of each (name, file) its ALPH payload cut short by 1..6 bytes and to a half, and with one bit flipped at 24 places
    spread over it, the header byte included; the container stays whole"""
    out = []
    for name, data in sources:
        payload = dict(A.chunks_of(data))[b"ALPH"]
        for cut in (1, 2, 3, 4, 5, 6, len(payload) // 2):
            if cut < len(payload):
                out.append((f"{name}-cut{cut}", A.with_alph(data, lambda p: p[:-cut])))
        rng = np.random.default_rng(len(payload))
        for bit in sorted({0, 3, 5, 7} | {int(v) for v in rng.integers(8, 8 * len(payload), 20)} if len(payload) > 1 else {0, 3, 5, 7}):
            out.append((f"{name}-bit{bit}", A.with_alph(data, lambda p: p[:bit >> 3] + bytes([p[bit >> 3] ^ 1 << (bit & 7)]) + p[(bit >> 3) + 1:])))
    return out
