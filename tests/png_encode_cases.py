"""The cases of the PNG encoder's tests (CPU and GPU): pictures -- every channel count, the sizes at which the kernels take another path,
contents on which each filter wins -- and raw byte strings for deflate.  Nothing here comes from the library; CHUNK is the rule's
FFHIP_DEFLATE_CHUNK, stated in include/ffpic_hip.h."""
import numpy as np

import png_encode_spec as spec

CHUNK = 16384
SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (17, 33), (100, 64), (1100, 3)]          # width x height; 1100: a row longer than one wave pass
CONTENTS = ["noise", "ramp", "flat", "noise4", "vstripes", "hstripes"]


class Case:
    def __init__(self, id, samples, filter=spec.ADAPTIVE):
        self.id, self.samples, self.filter = id, np.ascontiguousarray(samples), filter
        self.height, self.width, self.channels = self.samples.shape


def content(kind, w, h, c, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "noise4":
        return (rng.integers(0, 4, (h, w, c)) * 85).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, c), 9, np.uint8)
    if kind == "ramp":
        y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        return ((3 * x + 5 * y + 40 * k) % 256).astype(np.uint8)
    if kind == "vstripes":                                                # every row the same: Up wins below the first row
        row = rng.integers(0, 256, (1, w, c), dtype=np.uint8)
        return np.repeat(row, h, axis=0)
    if kind == "hstripes":                                                # every pixel of a row the same: Sub wins
        col = rng.integers(0, 256, (h, 1, c), dtype=np.uint8)
        return np.repeat(col, w, axis=1)
    raise ValueError(kind)


def all_five(c=1, w=40):
    """six rows on which None, Sub, Up, Average, (whichever), Paeth have the smallest sum"""
    rng = np.random.default_rng(55)
    n = w * c
    rows = np.zeros((6, n), np.int32)
    rows[0] = np.where(np.arange(n) % 2 == 0, 1, 255)                     # +-1 as signed bytes: every difference is larger
    rows[1] = (100 + np.arange(n) // c) % 256                             # a ramp far from the row above: the left neighbour predicts it
    rows[2] = rows[1]                                                     # the row above predicts it
    for x in range(n):                                                    # the mean of left and above predicts it
        rows[3, x] = ((rows[3, x - c] if x >= c else 0) + rows[2, x]) // 2
    half = (w // 2) * c
    rows[4, :half], rows[4, half:] = 10, rng.integers(0, 256, n - half)   # flat, then noise
    rows[5, :half], rows[5, half:] = 200, rows[4, half:]                  # left predicts the first half, above the second: Paeth follows both
    return rows.astype(np.uint8).reshape(6, w, c)


def _cases():
    out, seed = [], 0
    for c in (1, 2, 3, 4):
        for k, (w, h) in enumerate(SIZES):
            kind = CONTENTS[(k + c) % len(CONTENTS)]
            seed += 1
            out.append(Case(f"{w}x{h}x{c}-{kind}", content(kind, w, h, c, seed)))
    for k, kind in enumerate(CONTENTS):                                   # every content at a size of several rows, all channel counts between them
        c = 1 + k % 4
        seed += 1
        out.append(Case(f"17x33x{c}-{kind}-b", content(kind, 17, 33, c, seed)))
        out.append(Case(f"100x64x3-{kind}-b", content(kind, 100, 64, 3, seed + 100)))
    out.append(Case("tie", content("flat", 12, 5, 3, 0)))
    out.append(Case("all-five-1", all_five(1)))
    out.append(Case("all-five-3", all_five(3)))
    big = content("noise4", 910, 9, 4, 77)                                # 9 x (1 + 910 x 4) = 2 x CHUNK + 1 filtered bytes: three chunks, the last of one byte
    assert 9 * (1 + 910 * 4) == 2 * CHUNK + 1
    out.append(Case("910x9x4-noise4-three-chunks", big))
    for f in range(5):                                                    # fixed filters
        out.append(Case(f"17x33x3-ramp-filter{f}", content("ramp", 17, 33, 3, 5), f))
        out.append(Case(f"7x1x{1 + f % 4}-noise-filter{f}", content("noise", 7, 1, 1 + f % 4, 6 + f), f))
    out.append(Case("100x64x4-noise-filter4", content("noise", 100, 64, 4, 9), 4))
    return out


CASES = _cases()
SMALL = [c for c in CASES if c.samples.size <= 17 * 33 * 4]
LARGE = [c for c in CASES if c.samples.size > 17 * 33 * 4]


def _deflate_cases():
    rng = np.random.default_rng(2024)
    out = []
    text = (rng.integers(0, 16, 3 * CHUNK, dtype=np.uint8) + 97).tobytes()
    for n in (0, 1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 300):
        out.append((f"len{n}", text[:n]))
    out.append(("zeros", bytes(2 * CHUNK + 300)))                          # matches of 258 across steps and chunks
    for period in (3, 4, 7):
        unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        out.append((f"period{period}", (unit * (CHUNK // period + 200))[:CHUNK + 100 + period]))
    out.append(("noise16", rng.integers(0, 16, 65536, dtype=np.uint8).tobytes()))
    out.append(("noise", rng.integers(0, 256, 2 * CHUNK + 5, dtype=np.uint8).tobytes()))     # the stored form
    block = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    for d in (32768, 32769):                                              # a block again at the largest distance, and one beyond it
        out.append((f"repeat{d}", block + rng.integers(0, 256, d - 1000, dtype=np.uint8).tobytes() + block))
    out.append(("one-value", b"\x41" * 1000))
    out.append(("all-values", bytes(range(256))))
    return out


DEFLATE_CASES = _deflate_cases()

FORMS = ["HWC", "CHW", "reversed", "BGRA", "bottom-up", "padded"]


def source_form(samples, form):
    """the samples [H][W][C] laid out in one of the source forms -> (host uint8 array, offset of `pixels` in it, row_stride, pixel_stride,
    chan offsets in file order).  Bytes that are not the picture's are 0x5A."""
    h, w, c = samples.shape
    if form == "HWC":
        return samples.reshape(-1).copy(), 0, w * c, c, tuple(range(c))
    if form == "CHW":
        return np.ascontiguousarray(samples.transpose(2, 0, 1)).reshape(-1), 0, w, 1, tuple(k * w * h for k in range(c))
    if form == "reversed":                                                # BGR for three channels: the channels stored last to first
        return np.ascontiguousarray(samples[..., ::-1]).reshape(-1), 0, w * c, c, tuple(c - 1 - k for k in range(c))
    if form == "BGRA":                                                    # four bytes a pixel with a padded pitch, as the decoders leave it
        pitch = (4 * w + 15) & ~15
        host = np.full((h, pitch), 0x5A, np.uint8)
        px = np.full((h, w, 4), 0x5A, np.uint8)
        chan = {1: (1,), 2: (1, 3), 3: (2, 1, 0), 4: (2, 1, 0, 3)}[c]
        for k in range(c):
            px[..., chan[k]] = samples[..., k]
        host[:, :4 * w] = px.reshape(h, 4 * w)
        return host.reshape(-1), 0, pitch, 4, chan
    if form == "bottom-up":                                               # a negative row_stride: pixels points at the last stored row
        host = np.ascontiguousarray(samples[::-1]).reshape(-1)
        return host, (h - 1) * w * c, -w * c, c, tuple(range(c))
    if form == "padded":
        pitch = w * c + 5
        host = np.full((h, pitch), 0x5A, np.uint8)
        host[:, :w * c] = samples.reshape(h, w * c)
        return host.reshape(-1), 0, pitch, c, tuple(range(c))
    raise ValueError(form)
