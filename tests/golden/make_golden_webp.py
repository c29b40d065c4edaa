"""Fixtures of the WebP front end (ffhip_webp_probe / _parse / _decode_files_device): every file is decoded by the reference's own
WEBP_load in oracle/_ref (make_golden.ref_decode_webp: its loader with the predictor recorder hooked in), and what it passed on --
mode records with segment ids, the residual its predictors saw, filter header and parameters, BGRA -- is stored next to the file.

  real encoder   file_q100 / file_lf_q40 / file_lf_q55.webp (committed; decoded afresh), file_1080p_q75.webp (regenerated as
                 make_golden.gen_webp_file_1080p makes it, checked against the stored bgra_row_sums), PIL files of other sizes
  synthetic      tests/vp8_writer.py: what PIL cannot ask libwebp for (see there)

Widths that are not multiples of 16 are covered; HEIGHTS are multiples of 16 throughout, because the reference allocates its BGRA
for the height rounded up to 4 and converts 16 * mbrows rows into it (format/webp.c:1819, 1868): any other height overruns its heap
and the loader aborts or not by chance, so there is nothing to record.

Every planned case must decode in the reference (exit status 0): one that runs off a partition is given more bytes, never dropped.
For the quantiser sweep our own parser must find a non-zero DC and AC level in Y1, Y2 and UV for every segment in use.

Run from the repository root with the reference present:  python tests/golden/make_golden_webp.py"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden as M  # noqa: E402
import oracle_lib as O  # noqa: E402
import vp8_writer as W  # noqa: E402

# struct WEBP (format/webp.h:295-311; its members are packed, the struct itself is not): header 12 + vp8x 18 + alpha 9 + vp8 8 + fh 3 +
# fi 7 + k 1098 = 1155, p[4] aligned to 1156, d[4] behind its 32 bytes, filters behind d's 64 (checked against ref_webp_filter_info)
WEBP_D_OFFSET, WEBP_FILTERS_OFFSET = 1188, 1252

HIGH = [8] * 1056   # coefficient probabilities that send most tokens down to cat3..cat6


# segmentation on with the map kept: no segment ids are read and every macroblock is segment 0.  (With segmentation OFF the reference
# still reads a segment id from every macroblock header, with zero probabilities -- nearly always 3 -- and has quantisers for segment 0
# only, webp.c:393, 515: most residuals are then zero.  syn_lf_adj and syn_odd_size keep that path covered.)
SEG0 = dict(update_map=0, feature_mode=1, quant=(1, 0, 0, 0))


def skip_seed():
    """a seed whose first macroblock is coded (a skipped one in front of every coded one is unpinned) and whose skips run across a row end"""
    from ffpic_amd import capi, ops
    for seed in range(300, 1000):
        try:
            p = ops.webp_parse(W.keyframe(width=80, height=64, seed=seed, y_ac_qi=35, prob_skip=60, level=16, segmentation=SEG0, token_bytes=12000))
        except capi.FfhipError:
            continue
        sk = p["resmap"] != np.arange(20)
        if p["mbinfo"][0, :25].sum() > 0 and sk.sum() >= 8 and sk[4] and sk[5] and (~sk).sum() >= 3:
            return seed
    raise AssertionError("no seed")


def synthetic_cases():
    c = {}
    c["syn_parts2"] = dict(width=48, height=96, seed=101, log2_parts=1, y_ac_qi=30, level=12, segmentation=SEG0)
    c["syn_parts4"] = dict(width=40, height=96, seed=102, log2_parts=2, y_ac_qi=55, level=25, sharpness=3, segmentation=SEG0)
    c["syn_simple_filter"] = dict(width=64, height=48, seed=103, filter_type=1, level=30, y_ac_qi=60, segmentation=SEG0)
    c["syn_seg_abs"] = dict(width=64, height=48, seed=104, y_ac_qi=20, level=20,
                            segmentation=dict(update_map=1, feature_mode=1, quant=(10, -5, 127, 64), lf=(5, 40, -3, 63), probs=(120, 100, 160)))
    c["syn_seg_delta_negative"] = dict(width=48, height=48, seed=105, y_ac_qi=5, level=9,
                                       segmentation=dict(update_map=0, feature_mode=0, quant=(-20, 3, 0, 0), lf=(2, 0, 0, 0)))
    c["syn_skips"] = dict(width=80, height=64, seed=skip_seed(), y_ac_qi=35, prob_skip=60, level=16, segmentation=SEG0, token_bytes=12000)
    c["syn_cat6"] = dict(width=48, height=48, seed=108, y_ac_qi=3, coeff_probs=HIGH, token_bytes=60000, segmentation=SEG0)
    c["syn_lf_adj"] = dict(width=48, height=48, seed=109, y_ac_qi=45, level=33, sharpness=5, lf_adj=((7, 0, 0, 0), (-9, 0, 0, 0)))
    c["syn_vp8x"] = dict(width=44, height=32, seed=110, y_ac_qi=25, segmentation=SEG0, vp8x=(40, 30), trailing_chunk=b"EXIF" + (6).to_bytes(4, "little") + b"abcdef")
    c["syn_odd_size"] = dict(width=37, height=32, seed=111, y_ac_qi=70, level=5)
    for k, (qi, deltas) in enumerate([(0, (0, 0, 0, 0, 0)), (1, (-3, 2, -1, 4, -2)), (17, (5, -7, 15, -15, 9)), (64, (0, 3, 0, -4, 1)),
                                      (100, (-15, 15, -8, 7, -1)), (127, (6, 9, 12, 15, 3))]):
        # segmentation on with the map kept: no segment ids are read, every macroblock is segment 0 with index y_ac_qi + update
        c[f"syn_q{k}"] = dict(width=96, height=64, seed=120 + k, y_ac_qi=qi, deltas=deltas, level=7 + k, coeff_probs=[60] * 1056,
                              segmentation=dict(update_map=0, feature_mode=1, quant=((k % 3) - 1, 0, 0, 0)), token_bytes=20000)
    for k, (um, q) in enumerate([(1, (0, 31, 90, 127)), (1, (-1, -64, 5, 77)), (0, (-30, -10, 20, 80))]):
        c[f"syn_qseg{k}"] = dict(width=192, height=128, seed=140 + k, token_bytes=80000, p0_tail=4000, y_ac_qi=24, deltas=(1, -2, 3, -4, 5), coeff_probs=[60] * 1056,
                                 segmentation=dict(update_map=um, feature_mode=1, quant=q, probs=(128, 128, 128) if um else None))
    return c


def pil_cases():
    from PIL import Image
    rng = np.random.default_rng(77)
    out = {}
    for name, (w, h, kw) in {"pil_50x48_q30": (50, 48, dict(quality=30, method=2)), "pil_201x112_q80": (201, 112, dict(quality=80, method=4)),
                             "pil_17x16_q50": (17, 16, dict(quality=50, method=6)), "pil_320x16_q65": (320, 16, dict(quality=65, method=3))}.items():
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 110 * np.sin(xx / 9.0 + yy / 31.0), 127 + 100 * np.cos(xx / 13.0) * np.sin(yy / 5.0), (xx * 3 + yy * 5) % 256], axis=2)
        img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
        path = os.path.join(HERE, name + ".webp")
        Image.fromarray(img).save(path, "WEBP", **kw)
        out[name] = path
    return out


UNPINNED = ("syn_parts8", "syn_h37", "pil_50x37_q30")


def unpinned_synthetic():
    """the writer's arguments of the unpinned files that are its own"""
    return {"syn_parts8": dict(width=48, height=160, seed=150, log2_parts=3, y_ac_qi=33, level=14, segmentation=SEG0, token_bytes=3000),
            "syn_h37": dict(width=50, height=37, seed=151, y_ac_qi=48, level=21, sharpness=2, segmentation=SEG0)}


def unpinned_cases():
    """Files the reference cannot record: 8 token partitions overflow its p[4] / bt[4] arrays (format/webp.h:268, webp.c:437, 1904), a
    height that is not a multiple of 16 its BGRA buffer (see above).  They are committed WITHOUT reference data; the tests hold the host
    parser, the kernels and the oracle chain against each other on them."""
    from PIL import Image
    for name, kw in unpinned_synthetic().items():
        open(os.path.join(HERE, name + ".webp"), "wb").write(W.keyframe(**kw))
    rng = np.random.default_rng(78)
    yy, xx = np.mgrid[0:37, 0:50]
    img = np.stack([127 + 110 * np.sin(xx / 9.0 + yy / 31.0), 127 + 100 * np.cos(xx / 13.0) * np.sin(yy / 5.0), (xx * 3 + yy * 5) % 256], axis=2)
    img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(os.path.join(HERE, "pil_50x37_q30.webp"), "WEBP", quality=30, method=2)


def write_manifest():
    """MANIFEST_webp.sha256: the files written here.  (MANIFEST.sha256 is make_golden.py's: it rewrites that file from its own list.)"""
    lines = {}
    for f in sorted(os.listdir(HERE)):
        if f == "webp_front.npz" or (f.endswith(".webp") and (f.startswith(("syn_", "pil_")) or f == "file_1080p_q75.webp")):
            lines[f] = hashlib.sha256(open(os.path.join(HERE, f), "rb").read()).hexdigest()
    open(os.path.join(HERE, "MANIFEST_webp.sha256"), "w").write("".join(f"{h}  {f}\n" for f, h in sorted(lines.items())))


def ref_decode_with_quant(path):
    """ref_decode_webp plus the reference's w->d[4] (its dequantisation factors), read out of struct WEBP in a child process."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "q.npy")
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--quant", path, out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert rc == 0 and os.path.exists(out), f"reference could not decode {path} (status {rc})"
        return np.load(out)


def _quant_inproc(path, out):
    R = C.CDLL(O.REF_SO, mode=C.RTLD_GLOBAL)

    class Pic(C.Structure):
        _fields_ = [("pixels", C.c_void_p), ("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("depth", C.c_int),
                    ("pitch", C.c_int), ("format", C.c_int), ("refcnt", C.c_int), ("pic", C.c_void_p)]
    R.file_ops_init.restype = None
    R.file_probe.restype = C.c_void_p
    R.file_probe.argtypes = [C.c_char_p]
    R.file_load.restype = C.POINTER(Pic)
    R.file_load.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    R.file_ops_init()
    p = R.file_load(R.file_probe(path.encode()), path.encode(), 0).contents
    raw = np.ctypeslib.as_array(C.cast(p.pic, C.POINTER(C.c_uint8)), shape=(WEBP_FILTERS_OFFSET + 24,)).copy()
    info = (C.c_int * 27)()
    R.ref_webp_filter_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    R.ref_webp_filter_info(p.pic, info)
    assert list(raw[WEBP_FILTERS_OFFSET:]) == list(info)[3:27], "struct WEBP is not laid out as assumed"
    np.save(out, raw[WEBP_D_OFFSET:WEBP_D_OFFSET + 64].view(np.uint16).reshape(4, 8))
    os._exit(0)


def record(path):
    d = M.ref_decode_webp(path)   # raises when the reference does not exit with status 0
    return dict(modes=d["modes"], residual=d["residual"], lf=d["lf"], lf_header=d["lf_header"], dims=d["dims"], bgra=d["bgra"])


def check_sweep_levels(name, data):
    from ffpic_amd import ops
    p = ops.webp_parse(data)
    lv, seg, has_y2 = p["levels"], p["modes"][:, 18], p["modes"][:, 0] != 4
    coded = p["resmap"] == np.arange(len(seg))
    for s in np.unique(seg):
        m = coded & (seg == s)
        y2 = lv[m & has_y2][:, 24]
        y1 = lv[m & ~has_y2][:, :16]
        y1ac = lv[m][:, :16]
        uv = lv[m][:, 16:24]
        ok = [(y1[..., 0] != 0).any(), (y1ac[..., 1:] != 0).any(), (y2[..., 0] != 0).any(), (y2[..., 1:] != 0).any(), (uv[..., 0] != 0).any(), (uv[..., 1:] != 0).any()]
        assert all(ok), f"{name}: segment {s} lacks a non-zero level in (y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac) = {ok}"


def main():
    O.ref()
    res, names, table_in, table_out = {}, [], [], []
    from ffpic_amd import ops
    real = {n: os.path.join(HERE, n + ".webp") for n in ("file_q100", "file_lf_q40", "file_lf_q55")}
    real.update(pil_cases())
    for name, path in real.items():
        r = record(path)
        for k, v in r.items():
            res[f"{name}_{k}"] = v
        names.append(name)
        print(f"  {name}: {os.path.getsize(path)} B, dims {list(r['dims'])}")
    for name, kw in synthetic_cases().items():
        kw = dict(kw)
        path = os.path.join(HERE, name + ".webp")
        for attempt in range(6):   # a case the reference runs off a partition on gets more bytes, never dropped
            data = W.keyframe(**kw)
            open(path, "wb").write(data)
            try:
                r = record(path)
                break
            except RuntimeError:
                kw["token_bytes"] = kw.get("token_bytes", 6000) * 2
                kw["p0_tail"] = kw.get("p0_tail", 600) * 2
        else:
            raise AssertionError(f"the reference did not decode the planned case {name}")
        for k, v in r.items():
            res[f"{name}_{k}"] = v
        names.append(name)
        if name.startswith("syn_q"):
            check_sweep_levels(name, data)
            i = ops.webp_parse(data)["info"].quant_header
            table_in.append([i.y_ac_qi, i.y_dc_delta, i.y2_dc_delta, i.y2_ac_delta, i.uv_dc_delta, i.uv_ac_delta, i.segmentation_enabled,
                             i.update_mb_segmentation_map] + list(i.quantizer_update_value))
            table_out.append(ref_decode_with_quant(path))
        print(f"  {name}: {len(data)} B, dims {list(r['dims'])}, y-modes {np.bincount(r['modes'][:, 0], minlength=5)}, segments {np.bincount(r['modes'][:, 18], minlength=4)}")
    # the 1080p stream of make_golden.gen_webp_file_1080p, kept this time
    from PIL import Image
    from sklearn.datasets import load_sample_images
    imgs = load_sample_images().images
    Wd, Hd = 1920, 1088
    canvas = np.zeros((Hd, Wd, 3), np.uint8)
    k = 0
    for y in range(0, Hd, 427):
        for x in range(0, Wd, 640):
            im = imgs[k % 2]; k += 1
            h, w = min(427, Hd - y), min(640, Wd - x)
            canvas[y:y + h, x:x + w] = im[:h, :w]
    path = os.path.join(HERE, "file_1080p_q75.webp")
    Image.fromarray(canvas).save(path, "WEBP", quality=75, method=4)
    d = M.ref_decode_webp(path)
    rows = d["bgra"][:Hd].reshape(Hd, -1).view(np.uint32).astype(np.uint64)
    row_sums = (rows * (np.arange(rows.shape[1], dtype=np.uint64) + np.uint64(1))).sum(axis=1, dtype=np.uint64)
    stored = np.load(os.path.join(HERE, "webp_file_1080p.npz"))
    assert np.array_equal(row_sums, stored["bgra_row_sums"]), "the regenerated 1080p stream does not decode to the stored row sums"
    assert os.path.getsize(path) < (1 << 20)
    print(f"  file_1080p_q75.webp: {os.path.getsize(path)} B, row sums equal the stored ones")
    res["names"] = np.array(names)
    res["dequant_in"] = np.array(table_in, np.int32)
    res["dequant_out"] = np.array(table_out, np.uint16)
    np.savez_compressed(os.path.join(HERE, "webp_front.npz"), **res)
    unpinned_cases()
    write_manifest()

if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--unpinned":   # only the files without reference data, and the manifest
        unpinned_cases()
        write_manifest()
    elif len(sys.argv) == 4 and sys.argv[1] == "--quant":
        _quant_inproc(sys.argv[2], sys.argv[3])
    else:
        main()
