"""The shared list of lossless WebP test files (vp8l_writer.py writes them from known pixels).  Small pictures: the code goes wrong at
edges -- a band's last row and the next band's first, a row's last partial chunk of four, the last pixel's TR, a block that the width cuts,
a bundle the width cuts -- and not in the middle.  A list, no cross product: build() gives the same files in the same order every time."""
import functools
from collections import namedtuple

import numpy as np

import vp8l_writer as W
from exif_cases import tiff

P, X, G, I = W.PREDICTOR, W.CROSS_COLOR, W.ADD_GREEN, W.COLOR_INDEXING
# types: the transform types in the file's order; host: inverted by the host threads (colour indexing present and not first)
Case = namedtuple("Case", "name data argb alpha types host orientation cache_bits meta")
Damaged = namedtuple("Damaged", "name data code")
EINVAL, EANIMATION = -22, -1002


def noise(rng, h, w):
    return rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)


def smooth(h, w):
    """slow ramps that reach 0 and 255, so that the clamps of modes 12 and 13 and Select's choice matter"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    r = np.clip(x * 40 - 60, 0, 255)
    g = np.clip(300 - y * 45 - x * 7, 0, 255)
    b = np.clip((x + y) * 23 - 40, 0, 255)
    a = np.clip(255 - x * y * 9, 0, 255)
    return (a << 24 | r << 16 | g << 8 | b).astype(np.uint32)


def modes_image(rng, h, w, bits, modes=None):
    """a mode per block in the green byte, noise in the other three"""
    shape = (W.sub(h, bits), W.sub(w, bits))
    m = rng.integers(0, 14, shape) if modes is None else np.resize(np.asarray(modes), shape)
    return (noise(rng, *shape) & np.uint32(0xffff00ff)) | (m.astype(np.uint32) << 8)


def predictor(rng, h, w, bits=2, modes=None):
    return {"type": P, "bits": bits, "image": modes_image(rng, h, w, bits, modes)}


def cross(rng, h, w, bits=2):
    return {"type": X, "bits": bits, "image": noise(rng, W.sub(h, bits), W.sub(w, bits))}   # half of the multipliers are negative


def palette_picture(rng, h, w, n):
    pal = np.unique(noise(rng, 1, 4 * n))[:n]
    rng.shuffle(pal)
    idx = rng.integers(0, n, (h, w))
    idx.reshape(-1)[:min(n, h * w)] = np.arange(n)[:min(n, h * w)]
    return pal, idx, pal[idx]


def build():
    rng = np.random.default_rng(20259)
    cases = []

    def add(name, argb, transforms=(), alpha=True, host=False, orientation=1, **how):
        data = W.write(argb, transforms, alpha=alpha, **how)
        cases.append(Case(name, data, np.asarray(argb, dtype=np.uint32), bool(alpha), tuple(t["type"] for t in transforms), host, orientation,
                          how.get("cache_bits", 0), how.get("meta") is not None))

    # sizes: one pixel, one column, one row, chunk ends (4k - 1, 4k, 4k + 1), three and two band levels
    for w, h in ((1, 1), (1, 7), (7, 1), (5, 7), (4, 4), (33, 17), (7, 3), (8, 3), (9, 3), (65, 130), (130, 65)):
        a = noise(rng, h, w)
        add(f"size-{w}x{h}", a, [{"type": G}, predictor(rng, h, w), cross(rng, h, w)])
    # every mode alone, on ramps and on noise; 13 x 9: the last block is cut both ways
    for mode in range(14):
        add(f"mode-{mode}-smooth", smooth(9, 13), [predictor(rng, 9, 13, 2, [mode])])
        add(f"mode-{mode}-noise", noise(rng, 9, 13), [predictor(rng, 9, 13, 2, [mode])])
    add("modes-bits2", noise(rng, 19, 21), [predictor(rng, 19, 21, 2)])
    add("modes-bits3", smooth(19, 21), [predictor(rng, 19, 21, 3)])
    add("modes-bits9", noise(rng, 6, 9), [predictor(rng, 6, 9, 9, [11])])
    add("modes-raw-bytes", noise(rng, 8, 16), [predictor(rng, 8, 16, 2, [14, 15, 0x13, 0xfb, 0xfb, 0x13, 15, 14])])
    add("cross-alone", noise(rng, 9, 13), [cross(rng, 9, 13)])
    add("cross-bits5", noise(rng, 40, 37), [cross(rng, 40, 37, 5)])
    add("green-alone", noise(rng, 5, 6), [{"type": G}])
    add("no-transform", noise(rng, 3, 5))
    # the orders libwebp's encoder writes ...
    for types in ((G, P), (G, P, X), (P, X), (P,)):
        add("order-" + "".join(map(str, types)), noise(rng, 11, 10),
            [predictor(rng, 11, 10) if t == P else cross(rng, 11, 10) if t == X else {"type": G} for t in types])
    # ... and orders it does not: on the device while colour indexing is absent or first, else on the host
    add("order-120", noise(rng, 11, 10), [cross(rng, 11, 10), {"type": G}, predictor(rng, 11, 10)])
    add("order-012", smooth(11, 10), [predictor(rng, 11, 10), cross(rng, 11, 10), {"type": G}])
    two = np.where(rng.integers(0, 2, (6, 9)) > 0, np.uint32(0xff102030), np.uint32(0x80f0e0d0))
    for name, first in (("order-03-host", predictor(rng, 6, 9, 2, [1])), ("order-23-host", {"type": G})):
        res = W.forward(two.reshape(-1), 9, 6, first)
        add(name, two, [first, {"type": I, "palette": sorted(set(res))}], host=True)
    # colour indexing: 8, 4, 4, 2, 2, 1, 1 pixels per word; widths that cut a bundle
    for n, w in ((2, 17), (2, 1), (3, 7), (4, 8), (5, 9), (16, 17), (17, 9), (256, 8), (2, 8), (16, 1)):
        pal, idx, pic = palette_picture(rng, 5, w, n)
        add(f"palette-{n}-w{w}", pic, [{"type": I, "palette": pal}])
    for n, w, h in ((2, 17, 5), (4, 33, 6), (16, 17, 70), (256, 9, 5)):
        pal, idx, pic = palette_picture(rng, h, w, n)
        pw = W.sub(w, W.bundle_bits(n))
        add(f"palette-{n}-w{w}-predictor", pic, [{"type": I, "palette": pal}, predictor(rng, h, pw)])
    pal, idx, pic = palette_picture(rng, 4, 9, 16)
    add("palette-16-all-steps", pic, [{"type": I, "palette": pal}, {"type": G}, predictor(rng, 4, 5), cross(rng, 4, 5)])
    for n, bad in ((3, 3), (5, 15), (17, 200)):                   # an index beyond the palette is 0x00000000
        pal, idx, pic = palette_picture(rng, 4, 9, n)
        idx[1, 2] = idx[3, 8] = bad
        pic = np.where(idx >= n, np.uint32(0), pal[np.minimum(idx, n - 1)])
        add(f"palette-{n}-index-beyond", pic, [{"type": I, "palette": pal, "indices": idx}])
    # each of the 120 short distance codes at width 19, one pixel each, a literal between them
    toks = [("lit", int(v)) for v in noise(rng, 1, 8 * 19).reshape(-1)]
    for code in range(1, 121):
        toks += [("copy", 1, code), ("lit", int(noise(rng, 1, 1)[0, 0]))]
    toks += [("lit", int(v)) for v in noise(rng, 1, -len(W.run_tokens(toks, 19)) % 19).reshape(-1)]
    words = W.run_tokens(toks, 19)
    add("distance-codes-w19", np.array(words, dtype=np.uint32).reshape(-1, 19), tokens=toks)
    for w in (1, 2, 3):                                           # where dx + dy * xsize < 1 is 1
        toks = [("lit", int(v)) for v in noise(rng, 1, 2 * w + 1).reshape(-1)]
        for code in range(1, 9):
            toks += [("copy", 2, code), ("lit", int(noise(rng, 1, 1)[0, 0]))]
        toks += [("lit", int(v)) for v in noise(rng, 1, -len(W.run_tokens(toks, w)) % w).reshape(-1)]
        add(f"distance-codes-w{w}", np.array(W.run_tokens(toks, w), dtype=np.uint32).reshape(-1, w), tokens=toks)
    # copies: a run (distance 1, length 64), one that crosses row ends, a long distance by its plain code
    toks = [("lit", 0xff123456), ("copy", 64, 121), ("lit", 0x01020304), ("lit", 0x7f8090a0), ("copy", 30, 122), ("copy", 9, 120 + 60)]
    toks += [("lit", int(v)) for v in noise(rng, 1, -len(W.run_tokens(toks, 7)) % 7).reshape(-1)]
    add("copies", np.array(W.run_tokens(toks, 7), dtype=np.uint32).reshape(-1, 7), tokens=toks)
    # the colour cache: hits directly behind a copy, and of pixels a copy has brought in
    for bits in (1, 4, 11):
        lits = [int(v) for v in noise(rng, 1, 6).reshape(-1)]
        toks = [("lit", v) for v in lits] + [("copy", 3, 120 + 5), ("hit", lits[3]), ("auto", lits[5]), ("lit", lits[0] ^ 0x55), ("auto", lits[3])]
        toks += [("copy", 4, 2), ("hit", lits[3]), ("auto", lits[1])]
        toks += [("lit", int(v)) for v in noise(rng, 1, -len(W.run_tokens(toks, 5)) % 5).reshape(-1)]
        add(f"cache-{bits}", np.array(W.run_tokens(toks, 5), dtype=np.uint32).reshape(-1, 5), tokens=toks, cache_bits=bits)
    few = (rng.integers(0, 4, (12, 15)) * 0x01410a55 | 0xff000000).astype(np.uint32)
    add("cache-4-auto", few, [predictor(rng, 12, 15, 2, [0])], cache_bits=4)
    # a meta prefix image: three groups, their codes written three ways
    gmap = rng.integers(0, 3, (W.sub(10, 2), W.sub(13, 2)))
    gmap.reshape(-1)[:3] = (0, 1, 2)
    codes = {(1, 0): {"repeats": True}, (1, 1): {"repeats": True, "max_symbol": True, "lengths": [8] * 128 + [7] * 64},
             (2, 2): {"max_symbol": True, "lengths": W.complete_lengths(200)}, (2, 4): {"simple": (0,)}, (0, 4): {"simple": (3, 39)}}
    pic = noise(rng, 10, 13)
    red_small = ((pic >> 16) & 255) % 192
    blue_small = (pic & 255) % 200
    pic = (pic & np.uint32(0xff00ff00)) | (red_small << 16).astype(np.uint32) | blue_small.astype(np.uint32)
    add("meta-three-groups", pic, meta=(2, gmap), codes=codes, cache_bits=3)
    # the simple codes: one symbol (no bits), two symbols, a 1-bit symbol field; lengths that start with a repeat of the initial 8
    pic = (np.uint32(0xff000000) | (np.where(rng.integers(0, 2, (6, 7)) > 0, 200, 3) << 16).astype(np.uint32)
           | (rng.integers(0, 256, (6, 7)) << 8).astype(np.uint32) | rng.integers(0, 2, (6, 7)).astype(np.uint32))
    add("simple-codes", pic, codes={(0, 3): {"simple": (255,)}, (0, 1): {"simple": (3, 200)}, (0, 2): {"simple": (0, 1)}, (0, 4): {"simple": (1,), "wide": True},
                                    (0, 0): {"repeats": True, "lengths": [8] * 256}})
    add("one-colour", np.full((5, 9), 0x80112233, dtype=np.uint32),
        codes={(0, 0): {"simple": (0x22,)}, (0, 1): {"simple": (0x11,)}, (0, 2): {"simple": (0x33,)}, (0, 3): {"simple": (0x80,)}, (0, 4): {"simple": (0,)}})
    # alpha: the VP8L bit decides
    a = noise(rng, 5, 6)
    a[2, 3] &= np.uint32(0x00ffffff)                              # colour under alpha 0 is kept
    add("alpha-bit-off", a, alpha=False)
    add("alpha-on-vp8x-flag-clear", a, [{"type": G}], vp8x={"alpha": False})
    add("alpha-off-vp8x-flag-set", a, alpha=False, vp8x={"alpha": True})
    add("exif-6", noise(rng, 6, 10), [predictor(rng, 6, 10)], vp8x={"alpha": True}, exif=tiff(6), orientation=6)
    add("trailing-in-chunk", noise(rng, 3, 3), trailing=b"\x00\xff\x12")
    c = cases[-1]
    cases.append(c._replace(name="trailing-behind-riff", data=W.write(c.argb) + b"junk"))
    return cases


def damaged():
    """files the rule refuses, and every prefix of two small files"""
    rng = np.random.default_rng(7)
    a = noise(rng, 4, 5)
    out = []

    def add(name, data, code=EINVAL):
        out.append(Damaged(name, data, code))

    good = W.write(a, [{"type": G}, predictor(rng, 4, 5)])
    add("signature", W.write(a, signature=0x2e))
    add("version", W.write(a, version=1))
    add("over-subscribed", W.write(a, codes={(0, 1): {"lengths": [7] * 256}}))
    add("incomplete", W.write(a, codes={(0, 1): {"lengths": [9] * 256}}))
    add("two-lengths-incomplete", W.write(a, codes={(0, 4): {"lengths": [1, 2]}}))
    add("empty-code", W.write(a, codes={(0, 4): {"simple": (200,)}}))
    add("code-length-code-incomplete", W.write(a, codes={(0, 2): {"cl_lengths": [5] * 19}}))
    add("max-symbol-beyond", W.write(a, codes={(0, 4): {"raw_max_symbol": 41}}))
    add("repeat-beyond", W.write(a, codes={(0, 4): {"repeats": True, "lengths": [6] * 16 + [5] * 24 + [0] * 3}}))
    add("distance-beyond-start", W.write(a, tokens=[("lit", 1), ("copy", 19, 122)]))
    add("copy-at-start", W.write(a, tokens=[("copy", 20, 121)]))
    add("copy-beyond-end", W.write(a, tokens=[("lit", 1), ("copy", 20, 121)]))
    add("transform-twice", W.write(a, [{"type": G}], repeat={"type": G}))
    add("cache-bits-0", _cache_bits(a, 0))
    add("cache-bits-12", _cache_bits(a, 12))
    add("vp8x-canvas-disagrees", W.write(a, vp8x={"alpha": True, "canvas": (6, 4)}))
    add("vp8x-animation", W.write(a, vp8x={"alpha": True, "animation": True}), EANIMATION)
    body = b"WEBP" + W.chunk(b"VP8 ", bytes(20))
    add("lossy", b"RIFF" + len(body).to_bytes(4, "little") + body)
    add("not-riff", b"RIFX" + good[4:])
    add("riff-size-beyond", good[:4] + (len(good)).to_bytes(4, "little") + good[8:])
    add("chunk-size-beyond", good[:16] + (len(good)).to_bytes(4, "little") + good[20:])
    for name, f in (("plain", W.write(a)), ("transforms", good)):
        for n in range(len(f)):
            add(f"prefix-{name}-{n}", f[:n])
    return out


def _cache_bits(a, bits):
    """a colour cache of a size the format does not have: the writer's own stream with the 4-bit field replaced"""
    bw = W.BitWriter()
    bw.put(a.shape[1] - 1, 14)
    bw.put(a.shape[0] - 1, 14)
    bw.put(1, 1)
    bw.put(0, 3)
    bw.put(0, 1)                                                  # no transform
    bw.put(1, 1)
    bw.put(bits, 4)
    bw.put(0, 1)                                                  # no meta prefix image
    for n in (280 + (1 << bits if bits <= 11 else 0), 256, 256, 256, 40):
        W.put_code(bw, None, n)
    for v in a.reshape(-1):
        bw.put(0, 32)
    return W.riff(b"\x2f" + bw.bytes(), size=a.shape[::-1])


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(build())


@functools.lru_cache(maxsize=None)
def expected():
    """the answer key: each case's BGRA picture"""
    return tuple(W.expected_bgra(c.argb, c.alpha) for c in cases())


@functools.lru_cache(maxsize=None)
def damaged_cases():
    return tuple(damaged())


def levels_of(c):
    """launches of k_vp8l_predict a lone case takes: bands of 64 rows, where a predictor is undone on the device"""
    return (c.argb.shape[0] + 63) // 64 if W.PREDICTOR in c.types and not c.host else 0
