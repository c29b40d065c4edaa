"""Writes tests/golden/vp8l_libwebp.npz: lossless WebP files as PIL's encoder (libwebp) writes them, and PIL's decoded pixels for them, so
that the GPU tests need no PIL.  files(): the list, made again by whoever has PIL (tests/test_vp8l_spec.py holds the stored copy against
it).  Run from the repository root: python tests/golden/make_golden_vp8l.py"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "vp8l_libwebp.npz")


def pictures():
    """name -> RGBA or RGB uint8 [h][w][c]"""
    rng = np.random.default_rng(2026)
    out = {}
    out["noise-rgba-41x30"] = rng.integers(0, 256, (30, 41, 4), dtype=np.uint8)
    out["noise-rgb-40x31"] = rng.integers(0, 256, (31, 40, 3), dtype=np.uint8)
    y, x = np.mgrid[0:112, 0:201]
    out["gradient-201x112"] = np.stack([(x * 255) // 200, (y * 255) // 111, ((x + y) * 255) // 311], -1).astype(np.uint8)
    y, x = np.mgrid[0:48, 0:67]
    flat = np.full((48, 67, 3), 240, np.uint8)
    flat[8:40, 5:60] = (30, 60, 200)
    for k in range(6):                                            # text-like: thin strokes with hard edges
        flat[12 + 4 * k, 8:56:2] = (0, 0, 0)
        flat[10:38, 9 + 9 * k] = (255, 255, 255)
    out["flat-text-67x48"] = flat
    y, x = np.mgrid[0:30, 0:43]
    alpha = np.stack([(x * 3) % 256, (y * 5) % 256, (x * y) % 256, np.where((x // 8 + y // 8) % 3 == 0, 0, (x * 4) % 256)], -1).astype(np.uint8)
    out["alpha-zeros-43x30"] = alpha                              # without `exact` the encoder rewrites colour under alpha 0
    for n in (2, 4, 16, 17, 256):
        pal = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        out[f"palette-{n}-37x21"] = pal[rng.integers(0, n, (21, 37))]
    out["one-pixel"] = np.array([[[1, 2, 3, 4]]], np.uint8)
    return out


def extra():
    """pictures with the settings at which the encoder writes what the others do not: a palette with a predictor on the packed image,
    and a meta prefix image"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:40, 0:64]
    pal = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    return [("bands16-64x40", np.ascontiguousarray(pal[(x // 5 + y // 3) % 16]), dict(method=6, quality=100, exact=False)),
            ("noise-rgba-61x40", np.random.default_rng(2026).integers(0, 256, (40, 61, 4), dtype=np.uint8), dict(method=6, quality=0, exact=False))]


def how():
    """the encoder settings, taken in turn and then all on the gradient"""
    return [dict(method=m, quality=q, exact=e) for m in (0, 3, 6) for q in (0, 100) for e in (False, True)]


def files():
    """[(name, file bytes)] -- needs PIL"""
    from PIL import Image
    out = []

    def enc(name, a, kw):
        b = io.BytesIO()
        Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB").save(b, "WEBP", lossless=True, **kw)
        out.append((f"{name}-m{kw['method']}-q{kw['quality']}-{'exact' if kw['exact'] else 'plain'}", b.getvalue()))

    settings = how()
    for k, (name, a) in enumerate(pictures().items()):
        for kw in (settings[k % len(settings)], settings[(k + 5) % len(settings)], settings[(2 * k + 3) % len(settings)]):
            enc(name, a, kw)
    for kw in settings:
        enc("alpha-zeros-43x30-all", pictures()["alpha-zeros-43x30"], kw)
    for name, a, kw in extra():
        enc(name, a, kw)
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
