"""Pictures for the tests of libjpeg's pixel rule (include/ffpic_hip.h, "JPEG pictures with libjpeg's pixels"): files written
from known small coefficients by tests/jpeg_writer.py in every layout, files PIL writes, and what PIL (libjpeg-turbo) makes of them.
Seeded, built once per process."""
import collections
import functools
import io

import numpy as np

import jpeg_writer as W
from ffpic_amd import capi

Picture = collections.namedtuple("Picture", "name geom width height coef quant data")   # coef: (cy, cu, cv), cu / cv None for grey

# (width, height, luma h, luma v): every layout; chroma grids of at most 2 samples across and around it; single rows and columns
WRITER_SIZES = [(41, 23, 2, 2), (40, 24, 2, 1), (37, 19, 1, 2), (33, 17, 1, 1), (40, 8, 4, 1), (9, 40, 1, 4),
                (3, 5, 2, 2), (4, 4, 2, 2), (6, 5, 2, 2), (7, 5, 2, 2), (5, 3, 2, 1), (3, 3, 2, 1), (6, 3, 2, 1), (5, 9, 2, 1),
                (17, 1, 2, 2), (1, 17, 1, 2)]
# for the device: 4 x 3 MCUs of 4:2:0 (an interior MCU has all eight neighbours), 3 MCU rows of 4:2:2, grey
EXTRA_SIZES = [(56, 40, 2, 2), (30, 24, 2, 1), (21, 13, 0, 0)]


def _small_blocks(rng, n, ac):
    """DC in +-40, 12 % of the ACs non-zero within +-ac: coefficients as 8-bit samples give them, on which libjpeg's builds agree"""
    b = np.where(rng.random((n, 64)) < 0.12, rng.integers(-ac, ac + 1, (n, 64)), 0).astype(np.int16)
    b[:, 0] = rng.integers(-40, 41, n)
    return b


def _full_blocks(rng, n):
    return rng.integers(-32768, 32768, (n, 64)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def writer_picture(width, height, h, v, full_range=False):
    """h = v = 0: grey.  full_range: every coefficient over int16 and every quantiser over uint16 -- no file, the rule is the definition"""
    grey = h == 0
    h, v = (1, 1) if grey else (h, v)
    rng = np.random.default_rng([width, height, h, v, int(grey), int(full_range)])
    mc, mr = -(-width // (8 * h)), -(-height // (8 * v))
    n = mc * mr
    quant = np.ones((4, 64), np.uint16)
    if full_range:
        quant[:] = rng.integers(0, 65536, (4, 64))
        planes = [_full_blocks(rng, n * h * v)] + ([] if grey else [_full_blocks(rng, n), _full_blocks(rng, n)])
    else:
        quant[:2] = rng.integers(1, 30, (2, 64))
        planes = [_small_blocks(rng, n * h * v, 6)] + ([] if grey else [_small_blocks(rng, n, 8), _small_blocks(rng, n, 8)])
    coef = planes + [None] * (3 - len(planes))
    data = None if full_range else W.encode(width, height, h, v, coef, quant)
    geom = capi.jpeg_geom(mc, mr, 1 if grey else 3, h, v)
    flat = tuple(np.ascontiguousarray(p.reshape(-1)) if p is not None else None for p in coef)
    name = f"{'full' if full_range else 'writer'}_{width}x{height}_{'grey' if grey else f'h{h}v{v}'}"
    return Picture(name, geom, width, height, flat, quant, data)


def synthetic_rgb(width, height, seed=0):
    """a noisy photo-like picture with a flat saturated patch"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    img = np.clip(base + rng.normal(0, 12, (height, width, 3)), 0, 255).astype(np.uint8)
    img[height // 4:height // 2 + 1, width // 4:width // 2 + 1] = (250, 20, 30)
    return img


def pil_write(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def pil_files():
    """{name: bytes}: quality 90; 61x45 4:2:0 (and its progressive twin), 61x45 4:2:2, 50x33 4:4:4, 3x2 4:2:0, a grey one"""
    a, b = synthetic_rgb(61, 45, 1), synthetic_rgb(50, 33, 2)
    from PIL import Image
    grey = io.BytesIO()
    Image.fromarray(synthetic_rgb(45, 29, 3)[..., 1]).save(grey, "JPEG", quality=90)
    return {"420": pil_write(a, quality=90, subsampling=2), "422": pil_write(a, quality=90, subsampling=1),
            "444": pil_write(b, quality=90, subsampling=0), "420_3x2": pil_write(synthetic_rgb(3, 2, 4), quality=90, subsampling=2),
            "grey": grey.getvalue(), "420_progressive": pil_write(a, quality=90, subsampling=2, progressive=True)}


def pil_rgb(data):
    """what PIL decodes: uint8 [h][w][3]"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
