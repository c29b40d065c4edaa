"""Writes tests/golden/webp_alpha_libwebp.npz: lossy WebP files with an alpha plane as PIL's encoder (libwebp) writes them, and PIL's decoded
pixels for them, so that the GPU tests need no PIL.  The settings are those at which the encoder wrote each kind of ALPH chunk it writes:
raw and lossless, filters none, horizontal, vertical and gradient, with and without pre-processing.  files(): the list, made again by
whoever has PIL (tests/test_webp_alpha_spec.py holds the stored copy against it).  Run from the repository root:
python tests/golden/make_golden_webp_alpha.py"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "webp_alpha_libwebp.npz")

# (width, height, alpha kind, method, alpha_quality)
LIST = [
    (3, 5, "grad", 0, 100), (3, 5, "noise", 4, 50), (17, 9, "noise", 6, 100), (1, 1, "noise", 4, 100),          # raw planes
    (3, 5, "mask", 0, 100), (17, 9, "mask", 4, 100), (3, 5, "vstripe", 0, 50), (64, 64, "mask", 6, 50),          # lossless, no filter
    (17, 9, "grad", 0, 100), (17, 9, "vstripe", 4, 100), (50, 37, "grad", 6, 100), (50, 37, "vstripe", 0, 100),  # horizontal
    (64, 64, "grad", 0, 100), (64, 64, "vstripe", 0, 100), (33, 130, "grad", 4, 100),
    (50, 37, "soft", 0, 100), (50, 37, "soft", 4, 100), (50, 37, "soft", 6, 100),                                # gradient
    (130, 70, "vstripe", 0, 100), (130, 70, "vstripe", 4, 100), (130, 70, "vstripe", 6, 100),                    # vertical
    (33, 130, "soft", 4, 100), (33, 130, "mask", 4, 0), (33, 130, "hstripe", 6, 100), (130, 70, "soft", 4, 50),
    (130, 70, "mask", 0, 0), (64, 64, "soft", 6, 100), (64, 64, "noise", 4, 0), (50, 37, "hstripe", 4, 100), (17, 9, "soft", 6, 0),
]


def picture(w, h, kind):
    """RGBA uint8 [h][w][4]: noise for colour, the named plane for alpha"""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:h, 0:w]
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = {"grad": lambda: (x * 3 + y * 5) % 256,
         "noise": lambda: rng.integers(0, 256, (h, w)),
         "mask": lambda: (((x - w / 2) ** 2 + (y - h / 2) ** 2) < (min(w, h) / 3) ** 2) * 255,
         "hstripe": lambda: (y * 7) % 256 + 0 * x,
         "vstripe": lambda: (x * 7) % 256 + 0 * y,
         "soft": lambda: np.clip(255 - ((x - w / 2) ** 2 + (y - h / 2) ** 2) * 1020 / (min(w, h) ** 2), 0, 255)}[kind]()
    return np.dstack([rgb, a.astype(np.uint8)])


def files():
    """[(name, file bytes)] -- needs PIL"""
    from PIL import Image
    out = []
    for w, h, kind, method, aq in LIST:
        b = io.BytesIO()
        Image.fromarray(picture(w, h, kind), "RGBA").save(b, "WEBP", quality=40, method=method, alpha_quality=aq)
        out.append((f"{kind}-{w}x{h}-m{method}-a{aq}", b.getvalue()))
    return out


def decoded(data):
    """PIL's pixels as BGRA [h][w][4]"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))[..., [2, 1, 0, 3]])


def load():
    """-> [(name, file bytes, BGRA pixels)] from the stored copy"""
    z = np.load(PATH)
    return [(str(n), z[f"file_{k}"].tobytes(), z[f"bgra_{k}"]) for k, n in enumerate(z["names"])]


if __name__ == "__main__":
    fs = files()
    arrays = {"names": np.array([n for n, _ in fs])}
    for k, (_, d) in enumerate(fs):
        arrays[f"file_{k}"] = np.frombuffer(d, np.uint8)
        arrays[f"bgra_{k}"] = decoded(d)
    np.savez_compressed(PATH, **arrays)
    print(len(fs), "files", sum(len(d) for _, d in fs), "bytes ->", os.path.getsize(PATH))
