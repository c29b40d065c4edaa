"""Pictures for the lossy WebP encoder's tests: small, because the Python bool coder and the numpy witness are slow.
A case is (id, pixels, quality, filter): pixels uint8 [H][W][3] RGB or [H][W] grey; filter 0..63 or -1 for the rule's own level.
  sizes      1 x 1, 16 x 16, 17 x 16 and 33 x 47 (odd chroma, padded edges), 16 x 130 (nine macroblock rows: 8 partitions), 48 x 24 (2 rows:
             2 partitions)
  content    a flat picture whose planes are 128 (every macroblock skipped), checkerboard noise at quality 100 (large levels, cat6 tokens), a
             grey source
  settings   qualities 0, 30, 75, 100; filter 0, -1, 63"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "id pixels quality filter")


def picture(w, h, seed):
    """a smooth picture with an edge and some noise: all four prediction modes win somewhere"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([40 + 3 * xx + yy, 200 - 2 * yy + (xx > w // 2) * 30, 90 + ((xx + yy) % 23) * 4], -1)
    return np.clip(base + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def _cases():
    rng = np.random.default_rng(7)
    out = [Case("1x1", picture(1, 1, 1), 75, -1),
           Case("16x16", picture(16, 16, 2), 75, 0),
           Case("17x16", picture(17, 16, 3), 75, 0),
           Case("33x47", picture(33, 47, 4), 75, -1),
           Case("16x130-8-partitions", picture(16, 130, 5), 75, 0),
           Case("48x24-2-partitions", picture(48, 24, 6), 75, 63),
           Case("flat-all-skipped", np.full((32, 48, 3), 130, np.uint8), 75, 0),
           Case("checkerboard-noise-q100", (rng.integers(0, 2, (32, 32, 1), dtype=np.uint8) * 255).repeat(3, 2) ^ rng.integers(0, 2, (32, 32, 3), dtype=np.uint8) * 255, 100, 0),
           Case("grey-20x20", picture(20, 20, 8)[..., 1].copy(), 50, 0)]
    for q in (0, 30, 100):
        out.append(Case(f"33x47-q{q}", picture(33, 47, 4), q, 0))
    out.append(Case("40x24-q30-filter-auto", picture(40, 24, 9), 30, -1))
    return out


CASES = _cases()
