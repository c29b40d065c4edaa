"""Writes tests/golden/webp_libwebp.npz: the corpus of tests/test_webp_libwebp.py and tests/test_webp_libwebp_gpu.py.  Lossy WebP
files as byte arrays INSIDE the npz (no .webp file is added to the tree), each with the RGB that PIL (libwebp) decodes it to, and
PIL's and libwebp's version strings.  Needs PIL with WebP support; the tests need neither PIL nor this script.

  pil_*   written by PIL: sizes 1x1 .. 72x56, flat grey, flat colour, a ramp, noise, a smooth picture plus noise, qualities 5 .. 100,
          methods 0, 4 and 6.  Flat and tiny files are the ones whose first partition ends right behind the last macroblock header.
  wr_*    written by tests/vp8_writer.py with valid=True (RIFF padding, no segment ids without segmentation, 255 for an unset
          segment probability), one for each thing PIL cannot be asked for.  Segmentation is ON with all three tree probabilities
          given wherever a file is not about segmentation itself: then libwebp and the reference read the same modes and levels.

Run from the repository root:  python tests/golden/make_golden_libwebp.py"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vp8_writer as W  # noqa: E402

SIZES = [(1, 1), (2, 3), (16, 16), (17, 33), (50, 37), (64, 48), (72, 56)]
KINDS = ["grey", "colour", "ramp", "noise", "smooth"]
QUALITIES = [5, 30, 60, 80, 95, 100]
METHODS = [0, 4, 6]
SEG = dict(update_map=1, feature_mode=1, probs=(128, 128, 128))   # with absolute quantisers and filter levels: read alike by both rule sets


def picture(kind, w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "grey":
        a = np.full((h, w, 3), 128.0)
    elif kind == "colour":
        a = np.zeros((h, w, 3)) + (200, 60, 30)
    elif kind == "ramp":
        a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], -1)
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w, 3))
    else:
        a = np.stack([128 + 100 * np.sin(xx / 9.0), 128 + 100 * np.cos(yy / 7.0), 128 + 60 * np.sin((xx + yy) / 11.0)], -1) + rng.normal(0, 12, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def pil_files():
    from PIL import Image
    out, k = {}, 0
    combos = [(q, m) for m in METHODS for q in QUALITIES]
    rng = np.random.default_rng(2024)
    for w, h in SIZES:
        for kind in KINDS:
            q, m = combos[(5 * k) % len(combos)]
            k += 1
            b = io.BytesIO()
            Image.fromarray(picture(kind, w, h, rng)).save(b, "WEBP", quality=q, method=m)
            out[f"pil_{kind}_{w}x{h}_q{q}_m{m}"] = b.getvalue()
    for q, m, kind in ((5, 0, "smooth"), (30, 6, "noise"), (80, 0, "ramp"), (100, 6, "smooth"), (95, 4, "grey"), (60, 0, "colour"), (100, 0, "noise")):
        b = io.BytesIO()
        Image.fromarray(picture(kind, 64, 48, rng)).save(b, "WEBP", quality=q, method=m)
        out[f"pil_{kind}_64x48_q{q}_m{m}_b"] = b.getvalue()
    return out


def macroblocks(rng, n, *, ymode=None, bmode=None, uvmode=None, segs=1, skip=0.0, amp=5, big=None):
    """n macroblocks with sparse random levels.  ymode / bmode / uvmode: one mode for all, or None for random ones; segs: segment ids
    below this; skip: the share of skipped macroblocks; big: a level put into some Y2 / luma DC positions (cat6)."""
    ym = np.full(n, ymode) if ymode is not None else rng.integers(0, 5, n)
    bm = np.full((n, 16), bmode) if bmode is not None else rng.integers(0, 10, (n, 16))
    uv = np.full(n, uvmode) if uvmode is not None else rng.integers(0, 4, n)
    lv = np.zeros((n, 25, 16), np.int64)
    sk = (rng.random(n) < skip).astype(np.int64)
    sk[0] = 0
    for i in range(n):
        if sk[i]:
            continue
        for b in range(25):
            if b == 24 and ym[i] == 4:
                continue
            r = rng.random()
            if r < 0.3:
                continue
            if r < 0.4 and b < 16:
                lv[i, b, 1] = rng.integers(1, amp + 1)                    # one AC token, nothing else
                continue
            for pos in rng.integers(0, 16, rng.integers(1, 4)):
                lv[i, b, pos] = rng.integers(-amp, amp + 1)
            if big and b in (24, 3, 17) and rng.random() < 0.7:
                lv[i, b, 0 if b == 24 or ym[i] == 4 else 5] = big * (1 if rng.random() < 0.5 else -1)
        if ym[i] != 4:
            lv[i, :16, 0] = 0                                             # the DC of a 16x16 macroblock's luma is the Y2 block's
    return dict(ymode=ym, bmodes=bm, uvmode=uv, seg=rng.integers(0, segs, n), skip=sk, levels=lv)


def n_mb(w, h):
    return ((w + 15) >> 4) * ((h + 15) >> 4)


def writer_files():
    out = {}
    rng = np.random.default_rng(77)

    def put(name, w, h, mbs_args, **header):
        header.setdefault("y_ac_qi", 30)
        header.setdefault("segmentation", dict(SEG, quant=(header["y_ac_qi"],) * 4, lf=(header.get("level", 0),) * 4))
        if mbs_args.get("skip"):
            header.setdefault("prob_skip", 150)
        out["wr_" + name] = W.keyframe_from(w, h, macroblocks(rng, n_mb(w, h), **mbs_args), valid=True, **header)

    # every predictor on the top row, the left column and the right-most column: 3 x 3 macroblocks, one mode each
    for m, nm in enumerate(("dc", "tm", "v", "h")):
        put(f"border_i16_{nm}", 48, 48, dict(ymode=m, uvmode=m), level=0)
    for m in range(10):
        put(f"border_b{m}", 48, 48, dict(ymode=4, bmode=m, uvmode=m & 3), level=0)
    put("border_mixed", 44, 41, dict(), level=0)
    # segment quantisers and filter levels, as deltas and absolute; a negative sum; a map that is kept; a probability left unset
    put("seg_delta", 48, 32, dict(segs=4), y_ac_qi=50, level=20,
        segmentation=dict(update_map=1, feature_mode=0, quant=(5, -10, 20, -30), lf=(3, -5, 10, -20), probs=(120, 90, 200)))
    put("seg_abs", 48, 32, dict(segs=4), y_ac_qi=50, level=20,
        segmentation=dict(update_map=1, feature_mode=1, quant=(20, 40, 60, 90), lf=(0, 10, 30, 63), probs=(120, 90, 200)))
    put("seg_negative", 48, 32, dict(segs=4), y_ac_qi=10, level=12,
        segmentation=dict(update_map=1, feature_mode=0, quant=(-30, 4, -11, 0), lf=(0, 0, 0, 0), probs=(100, 128, 60)))
    put("seg_map_kept", 32, 32, dict(), y_ac_qi=35, level=9, segmentation=dict(update_map=0, feature_mode=1, quant=(60, 1, 2, 3), lf=(25, 1, 2, 3)))
    put("seg_prob_unset", 32, 32, dict(segs=2), level=15,
        segmentation=dict(update_map=1, feature_mode=1, quant=(30, 50, 0, 0), lf=(15, 25, 0, 0), probs=(None, 100, None)))
    put("seg_off", 32, 16, dict(), level=10, segmentation=None)
    # token partitions
    for lg in (1, 2, 3):
        put(f"parts{1 << lg}", 32, 56, dict(), log2_parts=lg, level=18)
    # the loop filter: simple, every sharpness, the deltas, a level that leaves 0..63 before the deltas bring it back
    put("simple", 48, 48, dict(skip=0.3), filter_type=1, level=24)
    for sh in range(1, 8):
        put(f"sharp{sh}", 32, 32, dict(amp=9), level=(12, 30, 45, 63, 20, 37, 50)[sh - 1], sharpness=sh)
    put("lf_deltas", 48, 32, dict(), level=30, lf_adj=((8, 0, 0, 0), (-12, 0, 0, 0)))
    put("lf_clamp", 48, 32, dict(segs=4), level=60, lf_adj=((-50, 0, 0, 0), (4, 0, 0, 0)),
        segmentation=dict(update_map=1, feature_mode=0, quant=(0, 0, 0, 0), lf=(10, -63, 0, 5), probs=(128, 128, 128)))
    # a height that is no multiple of 16; cat6 tokens with extra bits of 256 and above; skipped macroblocks; an odd chunk in front
    put("h37", 40, 37, dict(), level=14)
    put("cat6", 32, 32, dict(big=67 + 700), y_ac_qi=0, level=0)      # small factors: no sum leaves int16, where libwebp itself is not defined
    put("cat6_small_q", 32, 32, dict(big=67 + 260), y_ac_qi=2, level=5)
    put("skips", 64, 32, dict(skip=0.5), level=22)
    out["wr_iccp_odd"] = W.keyframe_from(32, 16, macroblocks(rng, 2), valid=True, segmentation=dict(SEG, quant=(30,) * 4, lf=(8,) * 4), y_ac_qi=30, level=8, vp8x=(31, 15, 0x20),
                                         leading_chunk=b"ICCP" + struct.pack("<I", 3) + b"abc\x00")
    return out


def main():
    import PIL
    from PIL import Image, features
    files = pil_files()
    files.update(writer_files())
    arrays = dict(names=np.array(sorted(files)), pil_version=np.array(PIL.__version__), libwebp_version=np.array(str(features.version("webp"))))
    for name, data in files.items():
        im = Image.open(io.BytesIO(data))          # a file libwebp refuses stops the script here
        rgb = np.asarray(im.convert("RGB"))
        assert rgb.shape[0] <= 56 and rgb.shape[1] <= 72
        arrays[name + "_bytes"] = np.frombuffer(data, np.uint8)
        arrays[name + "_rgb"] = rgb
    path = os.path.join(HERE, "webp_libwebp.npz")
    np.savez_compressed(path, **arrays)
    print(len(files), "files,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
