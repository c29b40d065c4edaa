"""The pictures the JPEG encoder's tests run on: every layout; the sizes 1x1, 8x8, 16x16, 17x13, 33x9, 9x33, 100x75, 40x24 (a
height that is even and no multiple of 16: the case the chroma rows' rule was found on), 2100x9 (a block row longer than a workgroup, an odd
block count) and one 1024x768 (prefix sums over more than one pass of a workgroup); the qualities 1, 50, 75, 100; restart intervals of 0, 1 and 3
MCUs; noise, a smooth ramp, 0/255 pixels (DC size 11 and AC size 10 at quality 100) and a flat picture (every block an EOB).  Not the full
product of these -- every value of every axis with every layout, and the combinations named above.  The witness's answers (tests/jpeg_encode_spec.py)
are computed once and kept."""
import zlib

import numpy as np

import jpeg_encode_spec as spec

SIZES = [(1, 1), (8, 8), (16, 16), (17, 13), (33, 9), (9, 33), (100, 75), (40, 24), (2100, 9)]
QUALITIES = [1, 50, 75, 100]
RESTARTS = [0, 1, 3]
CONTENTS = ["noise", "ramp", "binary", "flat"]
LAYOUTS = ["4:4:4", "4:2:2", "4:2:0", "grey"]


def picture(width, height, content, grey, seed):
    """-> uint8 [H][W][3] RGB, or [H][W]"""
    rng = np.random.default_rng(seed)
    shape = (height, width) if grey else (height, width, 3)
    if content == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "binary":
        return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)
    if content == "flat":
        return np.full(shape, 93, np.uint8) if grey else np.broadcast_to(np.array([200, 93, 31], np.uint8), shape).copy()
    yy, xx = np.mgrid[0:height, 0:width]
    ramp = ((xx * 3 + yy * 2) % 256).astype(np.uint8)
    return ramp if grey else np.stack([ramp, (255 - ramp // 2).astype(np.uint8), ((xx + 2 * yy) // 3 % 256).astype(np.uint8)], axis=-1)


class Case:
    def __init__(self, width, height, layout, quality, restart, content):
        self.width, self.height, self.layout, self.quality, self.restart, self.content = width, height, layout, quality, restart, content
        self.id = f"{width}x{height}-{layout}-q{quality}-r{restart}-{content}"
        self._key = None

    @property
    def pixels(self):
        return picture(self.width, self.height, self.content, self.layout == "grey", zlib.crc32(self.id.encode()))

    @property
    def key(self):
        """(coef [3], quant [4][64], file bytes) by the witness, computed once"""
        if self._key is None:
            coef, quant = spec.coefficients(self.pixels, self.layout, self.quality)
            self._key = (coef, quant, spec.file_from_coefficients(self.width, self.height, self.layout, coef, quant, self.restart))
        return self._key

    def __repr__(self):
        return self.id


def _cases():
    out, seen = [], set()

    def add(size, layout, quality, restart, content):
        c = Case(size[0], size[1], layout, quality, restart, content)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    k = 0
    for layout in LAYOUTS:
        for size in SIZES:                       # every size with every layout; the other axes rotate
            add(size, layout, QUALITIES[k % 4], RESTARTS[k % 3], CONTENTS[k % 4])
            k += 1
        for quality in QUALITIES:                # every quality, restart and content with every layout, on sizes with partial MCUs
            for content in CONTENTS:
                add((17, 13), layout, quality, RESTARTS[k % 3], content)
                k += 1
        for restart in RESTARTS:
            add((40, 24), layout, 75, restart, "noise")
            add((33, 9), layout, 100, restart, "binary")
        add((100, 75), layout, 100, 0, "binary")
    add((100, 75), "4:4:4", 100, 0, "noise")      # ~34 KB, ~200 stuffed bytes: larger than its pixels
    add((1024, 768), "4:2:0", 75, 3, "noise")
    return out


CASES = _cases()
LARGE = [c for c in CASES if c.width * c.height > 100000]
SMALL = [c for c in CASES if c.width * c.height <= 100000]
