"""The progressive JPEG files of tests/test_jpeg_progressive.py and tests/test_jpeg_progressive_gpu.py, built once per process.

pil_pairs():    PIL-made pairs, the same picture saved with progressive=True and progressive=False under otherwise the same arguments:
                libjpeg writes the same quantised coefficients either way, so the baseline twin through the existing decoder is the oracle.
writer_cases(): files of tests/jpeg_progressive.py from known coefficients, the smallest shapes where each path can go wrong, each with
                the planes a decoder must deliver and a baseline twin of those planes (tests/jpeg_writer.py).
"""
import functools
import io

import numpy as np

import jpeg_progressive as P
import jpeg_writer

PIL_CASES = [  # (tag, width, height, mode, save arguments)
    ("420_40x24", 40, 24, "RGB", dict(subsampling=2)),
    ("420_41x23", 41, 23, "RGB", dict(subsampling=2)),
    ("422_24x8", 24, 8, "RGB", dict(subsampling=1)),
    ("444_33x17", 33, 17, "RGB", dict(subsampling=0)),
    ("420_40x24_dri2", 40, 24, "RGB", dict(subsampling=2, restart_marker_blocks=2)),
    ("grey_37x19", 37, 19, "L", dict()),
    ("420_8x40_q100", 8, 40, "RGB", dict(subsampling=2, quality=100)),
]


def picture(width, height, mode, seed):
    """smooth plus noise, so that some blocks end early and EOBRUNs occur"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = np.stack([128 + 100 * np.sin(xx / 9.0), 128 + 90 * np.cos(yy / 7.0), (5 * xx + 3 * yy) % 256], axis=2)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    return img[:, :, 0] if mode == "L" else img


def pil_pair(img, **kw):
    from PIL import Image
    out = []
    for progressive in (True, False):
        bio = io.BytesIO()
        Image.fromarray(img).save(bio, "JPEG", progressive=progressive, **kw)
        out.append(bio.getvalue())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pil_pairs():
    """[(tag, progressive file, baseline twin)]"""
    out = []
    for n, (tag, w, h, mode, kw) in enumerate(PIL_CASES):
        kw = dict(kw)
        kw.setdefault("quality", 85)
        out.append((tag,) + pil_pair(picture(w, h, mode, n), **kw))
    return out


QUANT = np.ones((4, 64), np.uint16)
QUANT[0] = 3
QUANT[1] = 5

SPECTRAL = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), ss, se, 0, 0) for c in (0, 1, 2) for ss, se in ((1, 5), (6, 63))]
DEEP = ([((0, 1, 2), 0, 0, 0, 3), ((0, 1, 2), 0, 0, 3, 2), ((0, 1, 2), 0, 0, 2, 1), ((0, 1, 2), 0, 0, 1, 0)] +
        [((c,), 1, 63, ah, al) for c in (0, 1, 2) for ah, al in ((0, 3), (3, 2), (2, 1), (1, 0))])
SPLIT_DC = [((c,), 0, 0, 0, 1) for c in (0, 1, 2)] + [((c,), 1, 63, 0, 0) for c in (0, 1, 2)] + [((c,), 0, 0, 1, 0) for c in (2, 0, 1)]
GREY_EMPTY = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]
INCOMPLETE = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((1,), 1, 63, 0, 1), ((0,), 1, 5, 2, 1)]


def _late_ones(rng, width, height, h, v):
    """coefficients of magnitude 1 only: nothing of them is seen before the last (Al = 0) pass"""
    coef = P.random_coef(rng, width, height, h, v, density=0.2, amp=1)
    return coef


def _zrl_in_refinement(rng):
    """a grey block whose refinement needs ZRL over a run that holds coefficients already non-zero: history at k = 3, 9, 20 and 30 (large), the
    first new coefficient (magnitude 1) at k = 45, so 41 still-zero coefficients precede it: two ZRL, each stepping over history"""
    coef = [np.zeros((4, 64), np.int16)]
    for b in range(4):
        for k, val in ((3, 37), (9, -22), (20, 14 + b), (30, -9), (45, 1 if b % 2 else -1), (63, -1)):
            coef[0][b, P.ZZ[k]] = val
        coef[0][b, 0] = 100 * b - 150
    return coef


@functools.lru_cache(maxsize=None)
def writer_cases():
    """[dict(tag, file, planes, twin, width, height, h, v, ncomp, script, restart)]"""
    rng = np.random.default_rng(2024)
    specs = [  # tag, width, height, h, v, ncomp, script, restart, coefficients
        ("spectral_only", 16, 16, 2, 2, 3, SPECTRAL, 0, None),
        ("deep_3_bits", 17, 9, 1, 1, 3, DEEP, 0, None),
        ("dc_not_interleaved", 40, 24, 2, 2, 3, SPLIT_DC, 0, None),
        ("late_ones", 24, 16, 2, 1, 3, P.pil_script(3), 0, "ones"),
        ("zrl_in_refinement", 16, 16, 1, 1, 1, P.pil_script(1), 0, "zrl"),
        ("restart_cuts_eobrun", 40, 24, 2, 2, 3, P.pil_script(3), 7, "sparse"),
        ("one_mcu_420", 8, 8, 2, 2, 3, P.pil_script(3), 0, None),
        ("420_40x24", 40, 24, 2, 2, 3, P.pil_script(3), 0, None),
        ("h4v1_40x8", 40, 8, 4, 1, 3, P.pil_script(3), 0, None),
        ("grey_2048x1024_empty_band", 2048, 1024, 1, 1, 1, GREY_EMPTY, 0, "empty"),
        ("incomplete", 24, 16, 2, 2, 3, INCOMPLETE, 0, None),
    ]
    out = []
    for tag, w, hh, h, v, ncomp, script, restart, kind in specs:
        if kind == "ones":
            coef = _late_ones(rng, w, hh, h, v)
        elif kind == "zrl":
            coef = _zrl_in_refinement(rng)
        elif kind == "sparse":
            coef = P.random_coef(rng, w, hh, h, v, ncomp, density=0.02)
        elif kind == "empty":
            coef = [np.zeros((2048 * 1024 // 64, 64), np.int16)]
            coef[0][:, 0] = rng.integers(-300, 300, size=len(coef[0]))
        else:
            coef = P.random_coef(rng, w, hh, h, v, ncomp)
        data = P.encode_progressive(w, hh, h, v, coef, QUANT[:2], script, restart=restart)
        planes = P.expected_planes(coef, w, hh, h, v, script)
        hv = (h, v) if ncomp > 1 else (1, 1)
        twin = jpeg_writer.encode(w, hh, hv[0], hv[1], planes + [None] * (3 - ncomp), QUANT)
        out.append(dict(tag=tag, file=data, planes=planes, twin=twin, width=w, height=hh, h=hv[0], v=hv[1], ncomp=ncomp, script=script,
                        restart=restart))
    return out
