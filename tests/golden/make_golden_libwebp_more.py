"""Writes tests/golden/webp_libwebp_more.npz and tests/golden/webp_libwebp_real.json: what the tests of pixels='libwebp'
(tests/test_webp_pixels_libwebp*.py) need beyond the corpus of make_golden_libwebp.py.

webp_libwebp_more.npz, in the corpus's format (files as byte arrays inside the npz, each with PIL's RGB): files named wm_* from
vp8_writer.keyframe_from(..., valid=True) for what the 81 corpus files cover thinly --
  lfs_* / lfn_*   the simple and the normal loop filter, each over: coded 16x16 macroblocks with coefficients; coded ones whose tokens are
                  all explicit zeros (nothing to add; these two files are FINDINGS, below, and left out); skipped ones; B_PRED
  wrap0           a level x quantiser product of 65536, which the int16 store makes 0: that block has nothing to add
  ar_*            B_PRED macroblocks whose above-right neighbour's bottom row holds distinct values, in inner columns and the last one,
                  in row 0 and below (3 x 3 macroblocks of noisy B_PRED, once with the modes that read above-right only); the script
                  asserts the distinct values on the reconstruction (assert_above_right_is_told_apart)
  parts2/4/8      token partitions over four macroblock rows
  size_*          display sizes 16k + 1 and 16k + 15 on both axes
Nothing above 5 x 4 macroblocks.  For every file the script asserts that PIL accepts it and that vp8_spec.decode(SPEC)["rgb"] is PIL's RGB.

webp_libwebp_real.json: for the four real-encoder fixtures (file_lf_q40, file_lf_q55, file_q100, file_1080p_q75) the sha256 of PIL's RGB,
whole and per band of 16 rows, so that the 1080p check is a hash and not 17 s of Python.

Needs PIL with WebP support (libwebp 1.6.0 wrote the committed files); the tests need neither PIL nor this script.
Run from the repository root:  python tests/golden/make_golden_libwebp_more.py"""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vp8_spec as S  # noqa: E402
import vp8_writer as W  # noqa: E402
from make_golden_libwebp import SEG, macroblocks, n_mb  # noqa: E402

REAL = ["file_lf_q40", "file_lf_q55", "file_q100", "file_1080p_q75"]
# FINDINGS: files for which the witness does NOT give PIL's picture.  They are written, asserted to still differ, and left
# out of the npz.  libwebp switches a macroblock's inner edges on when some block of it had TOKENS read beyond its first position, the
# witness (and RFC 6386 section 15's wording) when some block has a non-zero coefficient: a coded macroblock whose tokens are all explicit
# zeros separates the two.  No encoder of pictures writes such a macroblock.
FINDINGS = ["wm_lfs_zeros", "wm_lfn_zeros"]


def writer_files():
    out = {}
    rng = np.random.default_rng(4021)

    def put(name, w, h, mbs, zeros16=None, **header):
        header.setdefault("y_ac_qi", 30)
        header.setdefault("segmentation", dict(SEG, quant=(header["y_ac_qi"],) * 4, lf=(header.get("level", 0),) * 4))
        if np.asarray(mbs["skip"]).any():
            header.setdefault("prob_skip", 150)
        out["wm_" + name] = W.keyframe_from(w, h, mbs, zeros16=zeros16, valid=True, **header)

    for tag, ftype in (("lfs", 1), ("lfn", 0)):
        n = n_mb(48, 32)
        put(f"{tag}_coded", 48, 32, macroblocks(rng, n, ymode=None, amp=9), filter_type=ftype, level=28)
        # coded, every token an explicit zero: count 16 and nothing non-zero in every block of half the macroblocks, the others noisy
        m = macroblocks(rng, n, amp=9)
        m["ymode"] = np.where(m["ymode"] == 4, 1, m["ymode"])          # 16x16 everywhere: B_PRED would switch the inner edges on by itself
        m["levels"][:, :16, 0] = 0                                      # (the DC of a 16x16 macroblock's luma is the Y2 block's)
        z = np.zeros((n, 25), bool)
        for i in range(0, n, 2):
            m["levels"][i] = 0
            z[i] = True
        put(f"{tag}_zeros", 48, 32, m, zeros16=z, filter_type=ftype, level=28)
        m = macroblocks(rng, n, amp=9, skip=0.6)
        m["ymode"] = np.where(m["ymode"] == 4, 0, m["ymode"])
        m["levels"][:, :16, 0] = 0
        put(f"{tag}_skipped", 48, 32, m, filter_type=ftype, level=28)
        put(f"{tag}_bpred", 48, 32, macroblocks(rng, n, ymode=4, amp=9, skip=0.4), filter_type=ftype, level=28)
    # 512 x 128 = 65536: AC_Q[q] = 128 at q = 99
    q = S.AC_Q.index(128)
    m = macroblocks(rng, 4, ymode=4, amp=3)
    m["levels"][1] = 0
    m["levels"][1, 5, 3] = 512
    m["levels"][2, 0, 1] = -512
    put("wrap0", 32, 32, m, y_ac_qi=q, level=20)
    # above-right: noisy B_PRED on 3 x 3 macroblocks, all ten modes and the two that read nothing but the row above and above-right.  Noise alone
    # does not promise distinct samples where they are needed (levels of this size saturate whole rows): the first seed whose reconstruction
    # passes assert_above_right_is_told_apart is taken, and main() asserts it again on the file as written
    for name, only in (("ar_mixed", None), ("ar_ld_vl", (6, 7))):
        for seed in range(1000):
            r2 = np.random.default_rng(9000 + seed)
            m = macroblocks(r2, 9, ymode=4, amp=25)
            if only:
                m["bmodes"] = r2.choice(only, (9, 16))                   # LD, VL
            put(name, 48, 48, m, level=0)
            try:
                assert_above_right_is_told_apart("wm_" + name, S.decode(out["wm_" + name], S.SPEC))
            except AssertionError:
                continue
            break
        else:
            raise AssertionError(name + ": no seed gives distinct above-right samples")
        if only:
            put(name + "_filtered", 48, 48, dict(m), level=35)
    for lg in (1, 2, 3):
        put(f"parts{1 << lg}", 32, 64, macroblocks(rng, n_mb(32, 64), amp=7, skip=0.2), log2_parts=lg, level=18)
    for w, h in ((17, 17), (31, 31), (17, 31), (31, 17), (65, 49), (79, 63), (33, 15)):
        put(f"size_{w}x{h}", w, h, macroblocks(rng, n_mb(w, h), amp=9), level=22)
    return out


def assert_above_right_is_told_apart(name, w):
    """an ar_* file without a loop filter (the witness's planes are the reconstruction): below row 0 EVERY B_PRED macroblock of an inner column has
    an above-right neighbour whose bottom row holds four distinct values -- so the macroblock's above-right samples differ from 127 four times and
    from any one sample repeated -- and the last column one whose last sample above is not 127"""
    assert w["filter_type"] == 0 and (w["modes"][:, 0] == 4).all(), name
    cols, rows, y = w["mbcols"], w["mbrows"], w["y"]
    assert cols >= 3 and rows >= 3, name
    for x in range(cols - 1):
        distinct = [len(set(y[16 * r - 1, 16 * x + 16:16 * x + 20].tolist())) for r in range(1, rows)]
        assert min(distinct) == 4, (name, "column", x, distinct)
    assert all(int(y[16 * r - 1, 16 * cols - 1]) != 127 for r in range(1, rows)), (name, "last column")


def main():
    import PIL
    from PIL import Image, features
    files = writer_files()
    arrays = dict(names=np.array(sorted(files)), pil_version=np.array(PIL.__version__), libwebp_version=np.array(str(features.version("webp"))))
    for name in FINDINGS:
        data = files.pop(name)
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert not np.array_equal(S.decode(data, S.SPEC)["rgb"], rgb), f"{name}: the witness gives PIL's picture now"
    arrays["names"] = np.array(sorted(files))
    for name, data in files.items():
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))        # a file libwebp refuses stops the script here
        w = S.decode(data, S.SPEC)
        assert not w["refused"], name
        assert w["mbcols"] <= 5 and w["mbrows"] <= 4, name
        assert w["rgb"].shape == rgb.shape and np.array_equal(w["rgb"], rgb), f"{name}: the witness differs from PIL"
        if name in ("wm_ar_mixed", "wm_ar_ld_vl"):
            assert_above_right_is_told_apart(name, w)
        arrays[name + "_bytes"] = np.frombuffer(data, np.uint8)
        arrays[name + "_rgb"] = rgb
    path = os.path.join(HERE, "webp_libwebp_more.npz")
    np.savez_compressed(path, **arrays)
    print(len(files), "files,", os.path.getsize(path), "bytes")

    real = dict(pil_version=PIL.__version__, libwebp_version=str(features.version("webp")), files={})
    for name in REAL:
        rgb = np.ascontiguousarray(np.asarray(Image.open(os.path.join(HERE, name + ".webp")).convert("RGB")))
        real["files"][name] = dict(width=int(rgb.shape[1]), height=int(rgb.shape[0]), sha256=hashlib.sha256(rgb.tobytes()).hexdigest(),
                                   bands=[hashlib.sha256(rgb[r:r + 16].tobytes()).hexdigest() for r in range(0, rgb.shape[0], 16)])
    with open(os.path.join(HERE, "webp_libwebp_real.json"), "w") as f:
        json.dump(real, f, indent=1)
        f.write("\n")
    print({k: (v["width"], v["height"], len(v["bands"])) for k, v in real["files"].items()})


if __name__ == "__main__":
    main()
