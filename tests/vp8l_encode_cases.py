"""The cases of the lossless WebP encoder's tests (CPU and GPU): the smallest pictures at which each part of the rule of include/ffpic_hip.h
("Lossless WebP encoding") can go wrong.  Nothing here comes from the library.  A tile is 16 x 16 pixels, a chunk 4096 pixels."""
import numpy as np

BOTH, GREEN, PREDICT = 3, 1, 2


class Case:
    def __init__(self, id, samples, flags=BOTH):
        self.id, self.samples, self.flags = id, np.ascontiguousarray(samples, dtype=np.uint8), flags
        self.height, self.width, self.channels = self.samples.shape


def scene(w, h, c, seed):
    """smooth gradients with an edge, a textured corner and a little noise, so that tiles differ in their best predictor"""
    rng = np.random.default_rng(seed)
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    v = 3 * x + 2 * y * (k + 1) + 37 * k
    v = np.where(x + y > (w + h) // 2, 255 - v // 2, v)
    v = v + np.where((x < w // 3) & (y > h // 2), 40 * ((x // 2 + y) % 2), 0)
    v = v + rng.integers(0, 3, (h, w, c))
    return (v % 256).astype(np.uint8)


def fibonacci_green(seed=4):
    """110 x 161 = 17 710 pixels: the sum of the first 20 Fibonacci numbers, which are the counts of 20 green values.  A Huffman tree over
    them is 19 deep, so the limit of 15 binds.  Blue is noise: no three neighbouring words are equal, every pixel is a literal"""
    rng = np.random.default_rng(seed)
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 110 * 161
    green = np.repeat(np.arange(20) * 11 + 3, fib)
    rng.shuffle(green)
    px = np.zeros((161, 110, 3), np.uint8)
    px[..., 1] = green.reshape(161, 110)
    px[..., 2] = rng.integers(0, 256, (161, 110))
    return px


def _cases():
    rng = np.random.default_rng(99)
    out = []
    for k, (w, h) in enumerate([(1, 1), (1, 70), (70, 1), (16, 16), (17, 17), (32, 32), (33, 33), (64, 65), (100, 50)]):     # 64 x 65: two chunks; 100 x 50: the boundary inside a row
        for c in (1, 2, 3, 4):
            if (k + c) % 2 == 0 or (w, h) in ((17, 17), (33, 33), (64, 65)):
                out.append(Case(f"{w}x{h}x{c}-scene", scene(w, h, c, 10 * k + c)))
    out.append(Case("70x70x4-flat", np.full((70, 70, 4), 9)))                    # single-symbol alphabets; a run to the chunk's end; "above" into the earlier chunk
    out.append(Case("70x70x4-flat-plain", np.full((70, 70, 4), 9), 0))
    out.append(Case("70x70x1-flat", np.full((70, 70, 1), 200)))
    stripes = np.zeros((66, 67, 3), np.uint8)
    stripes[:, ::2], stripes[:, 1::2] = (200, 10, 60), (20, 130, 250)
    out.append(Case("67x66x3-stripes-plain", stripes, 0))                        # two-symbol simple codes, matches from above
    out.append(Case("67x66x3-stripes", stripes))
    rows = np.zeros((65, 64, 4), np.uint8)
    rows[::2], rows[1::2] = (1, 2, 3, 255), (9, 8, 7, 0)
    out.append(Case("64x65x4-rows-plain", rows, 0))                              # runs to the left, row by row
    noise = rng.integers(0, 256, (48, 48, 4), dtype=np.uint8)
    out.append(Case("48x48x4-noise", noise))                                     # all 256 symbols
    out.append(Case("48x48x4-noise-plain", noise, 0))
    out.append(Case("48x48x3-noise4", (rng.integers(0, 4, (48, 48, 3)) * 85).astype(np.uint8), GREEN))
    out.append(Case("110x161x3-fibonacci-plain", fibonacci_green(), 0))         # the 15-bit limit and the halving rule
    under = scene(40, 36, 4, 5)
    under[4:30, 5:33, 3] = 0                                                     # colour under alpha 0 stays
    under[10:20, 10:20, :3] = rng.integers(0, 256, (10, 10, 3))
    out.append(Case("40x36x4-colour-under-alpha-0", under))
    for flags, name in ((GREEN, "green"), (PREDICT, "predict"), (0, "plain")):   # each flag alone, and none
        out.append(Case(f"45x40x3-scene-{name}", scene(45, 40, 3, 7), flags))
        out.append(Case(f"45x40x2-scene-{name}", scene(45, 40, 2, 8), flags))
    out.append(Case("300x300x3-scene", scene(300, 300, 3, 12)))                  # 22 chunks and 361 tiles
    return out


CASES = _cases()
SMALL = [c for c in CASES if c.samples.size <= 70 * 70 * 4]
LARGE = [c for c in CASES if c.samples.size > 70 * 70 * 4]
