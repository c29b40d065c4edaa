"""The WebP / VP8 path against a witness that is neither the reference nor this library: tests/vp8_spec.py, a plain decoder written
from RFC 6386, held to libwebp (PIL) on the corpus of tests/golden/make_golden_libwebp.py.

  rules=SPEC       must give PIL's RGB of every corpus file, sample for sample.
  rules=REFERENCE  SPEC plus the named deviations of vp8_spec.FLAGS: must give what the tree produces -- the host parser's arrays and
                   the oracle chain's planes for the corpus, the reference-made pixels for the golden fixtures -- and an independent
                   witness for the three fixtures the reference cannot record.
  every flag is live and minimal; no tolerance anywhere.  No GPU needed; PIL only for the half of one test."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import vp8_spec as S
from ffpic_amd import capi, ops
from test_webp_front_capi import FRONT, GOLDEN, NAMES, UNPINNED, _status, check_modes, file_bytes, oracle_bgra, oracle_residual

CORPUS = np.load(os.path.join(GOLDEN, "webp_libwebp.npz"))
CNAMES = [str(n) for n in CORPUS["names"]]
# Corpus files whose REFERENCE decode differs from the tree in a way no named rule explains yet: at most one in ten, each asserted to
# STILL differ.  None today.
UNEXPLAINED = []
# Flags no corpus file can show, with the reason; their liveness is asserted on the golden fixtures instead.
LIVE_ON_FIXTURES_ONLY = {
    "idct_pass1_int16": "needs sums beyond int16 inside the IDCT, where libwebp's own answer differs between its C and SIMD transforms: "
                        "no such file has ONE libwebp picture to be held to",
}
# the two rules behind every refusal of a valid file
REFUSING = {"segment_id_without_segmentation", "segment_prob_default_0", "chunk_walk_without_padding"}


def data_of(name):
    return CORPUS[name + "_bytes"].tobytes() if name in CNAMES else file_bytes(name)


@functools.lru_cache(maxsize=None)
def _decode(name, rules):
    try:
        return S.decode(data_of(name), rules)
    except S.Refused:
        return None


def witness(name, rules):
    """the witness's decode of a corpus file or golden fixture, or None where it finds no frame at all; shared by every test.  The
    colour flag is applied by picture(), so the decode is the same with and without it"""
    return _decode(name, frozenset(rules) - {"reference_colour"})


def planes_to_bgra(o):
    """the reference's colour step (pinned in test_oracle_golden.py, test_color_gpu.py) on the witness's planes: [16r][16c][4]"""
    c, r = o["mbcols"], o["mbrows"]
    out = np.zeros((16 * r, 64 * c), np.uint8)
    y, u, v = [np.ascontiguousarray(o[k]).reshape(-1) for k in "yuv"]
    O.ffo().ffo_yuv420_to_bgra32(out.reshape(-1), 64 * c, y, u, v, 16 * c, 8 * c, r, c)
    return out.reshape(16 * r, 16 * c, 4)


def picture(o, rules):
    """BGR [h][w][3] of a decode under `rules`: the colour step is the one flag applied outside vp8_spec.decode"""
    if "reference_colour" in rules:
        return planes_to_bgra(o)[:o["height"], :o["width"], :3]
    return o["rgb"][:, :, ::-1]


def moved(a, b):
    """samples that differ between two pictures, those outside their common part included"""
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    return int((a[:h, :w] != b[:h, :w]).sum()) + 3 * (a.shape[0] * a.shape[1] + b.shape[0] * b.shape[1] - 2 * h * w)


def tree_planes(p):
    """the oracle chain on the host parser's arrays (the chain the GPU tests hold the device to): filtered Y, U, V"""
    c, r = p["mbcols"], p["mbrows"]
    y, u, v = [np.ascontiguousarray(a).copy() for a in O.oracle_vp8_frame(c, r, p["modes"], oracle_residual(p))]
    if p["filter_type"]:
        O.ffo().ffo_vp8_loopfilter_frame(c, r, p["filter_type"], np.ascontiguousarray(p["modes"]).reshape(-1), np.ascontiguousarray(p["filters"]).reshape(-1),
                                         y.reshape(-1), u.reshape(-1), v.reshape(-1))
    return y.reshape(16 * r, 16 * c), u.reshape(8 * r, 8 * c), v.reshape(8 * r, 8 * c)


def parse_differences(o, p):
    """names of the parse results in which witness `o` and host parser `p` differ"""
    bad = [k for k in ("width", "height", "mbcols", "mbrows", "nbr_partitions", "filter_type") if o[k] != p[k]]
    bad += [k for k in ("modes", "levels", "resmap") if not np.array_equal(o[k], p[k])]
    if not np.array_equal(o["counts"], p["mbinfo"][:, :25]) or not np.array_equal(p["mbinfo"][:, 25], o["modes"][:, 0] != 4) or \
            not np.array_equal(p["mbinfo"][:, 26], o["modes"][:, 18]):
        bad.append("mbinfo")
    if not np.array_equal(o["quant"], p["quant"][:, :6]):
        bad.append("quant")
    if not np.array_equal(o["filters"], p["filters"]):
        bad.append("filters")
    return bad


def tree_differences(name):
    """where the witness under REFERENCE and the tree differ on a file both accept"""
    o, p = witness(name, S.REFERENCE), ops.webp_parse(data_of(name))
    bad = parse_differences(o, p)
    if "mbcols" not in bad and "mbrows" not in bad:
        for k, plane in zip("yuv", tree_planes(p)):
            if not np.array_equal(o[k], plane):
                at = np.argwhere(o[k] != plane)[0]
                bad.append(f"plane {k}: {int((o[k] != plane).sum())} samples, first at row {at[0]} column {at[1]}")
        if not np.array_equal(planes_to_bgra(o).reshape(16 * p["mbrows"], -1), oracle_bgra(p, oracle_residual(p))):
            bad.append("BGRA")
    return bad


def test_corpus_is_what_the_issue_asks_for():
    assert 60 <= len(CNAMES) <= 90 and os.path.getsize(os.path.join(GOLDEN, "webp_libwebp.npz")) < 1 << 20
    assert all(CORPUS[n + "_rgb"].shape[0] <= 56 and CORPUS[n + "_rgb"].shape[1] <= 72 for n in CNAMES)
    pil = [n for n in CNAMES if n.startswith("pil_")]
    for size in ("1x1", "2x3", "16x16", "17x33", "50x37", "64x48", "72x56"):
        assert any(f"_{size}_" in n for n in pil), size
    for word in ["grey", "colour", "ramp", "noise", "smooth"] + [f"_q{q}_" for q in (5, 30, 60, 80, 95, 100)] + [f"_m{m}" for m in (0, 4, 6)]:
        assert any(word in n for n in pil), word
    assert len(UNEXPLAINED) * 10 <= len(CNAMES) and set(UNEXPLAINED) <= set(CNAMES)


@pytest.mark.parametrize("name", CNAMES)
def test_spec_equals_pil(name):
    """no exceptions: a file the witness cannot match means the witness is wrong"""
    o = witness(name, S.SPEC)
    assert o is not None and not o["refused"]
    want = CORPUS[name + "_rgb"]
    assert o["rgb"].shape == want.shape
    assert np.array_equal(o["rgb"], want), f"{int((o['rgb'] != want).sum())} samples differ"


def test_stored_rgb_is_the_installed_pils():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check("webp"):
        pytest.skip("PIL without WebP")
    import io
    for name in CNAMES:
        got = np.asarray(Image.open(io.BytesIO(data_of(name))).convert("RGB"))
        assert np.array_equal(got, CORPUS[name + "_rgb"]), (name, str(CORPUS["pil_version"]), str(CORPUS["libwebp_version"]))


def test_libwebp_refuses_exactly_the_fixtures_without_riff_padding():
    """why the older syn_* fixtures have no libwebp picture: vp8_writer.py wrote an odd-sized VP8 chunk without the
    padding byte, as the reference walks chunks; with the byte added libwebp takes them (syn_vp8x aside: its canvas fields, 40 and 30,
    name a 41 x 31 canvas around a 44 x 32 frame)"""
    Image = pytest.importorskip("PIL.Image")
    import io
    import struct

    def accepted(data):
        try:
            Image.open(io.BytesIO(data)).load()
            return True
        except Exception:
            return False
    for name in NAMES + UNPINNED:
        data = file_bytes(name)
        at = data.index(b"VP8 ")
        odd = struct.unpack("<I", data[at + 4:at + 8])[0] & 1
        assert accepted(data) == (not odd), name
        if odd and name != "syn_vp8x":
            assert accepted(b"RIFF" + struct.pack("<I", len(data) - 7) + data[8:] + b"\x00"), name


def refused_by_witness(name, rules=S.REFERENCE):
    o = witness(name, rules)
    return o is None or o["refused"]


@pytest.mark.parametrize("name", CNAMES)
def test_reference_equals_the_tree_on_the_corpus(name):
    """probe and host parser refuse exactly the files the witness's REFERENCE rules refuse; on the others the parser's modes, levels,
    counts, residual map, quantisers and filter parameters and the oracle chain's planes are the witness's"""
    rc, prc = _status(data_of(name))
    o = witness(name, S.REFERENCE)
    assert (rc != 0) == (o is None), "probe"
    assert (prc != 0) == refused_by_witness(name), "parser"
    if prc:
        assert prc == capi.FFHIP_EINVAL
        return
    bad = tree_differences(name)
    if name in UNEXPLAINED:
        assert bad, "explained by now: take it off the list"
    else:
        assert not bad, bad


def test_valid_files_are_refused_exactly_where_the_named_rules_say():
    """libwebp decodes every corpus file.  The tree refuses those in which the reference's segment-id read (with segmentation off, or
    with a probability left unset) eats the first partition's last bits, or whose odd chunk is padded: with these rules off, none"""
    refused = [n for n in CNAMES if refused_by_witness(n)]
    assert any("grey" in n for n in refused) and any("colour" in n for n in refused) and any("_1x1_" in n for n in refused)
    assert not any(refused_by_witness(n, S.SPEC) for n in CNAMES)
    for n in refused:
        assert not refused_by_witness(n, S.REFERENCE - REFUSING), n
        alone = [f for f in sorted(REFUSING) if refused_by_witness(n, frozenset([f]))]
        assert alone, n                                # one of the three alone over SPEC refuses it already
    print(f"\n{len(refused)} of {len(CNAMES)} corpus files refused under REFERENCE:", ", ".join(refused))


def test_how_far_the_default_pixels_are_from_libwebp():
    """the measurement of DESIGN.md 4.19: the tree's default pixels (REFERENCE) against PIL's, file by file, over PIL's picture"""
    rows = []
    for n in CNAMES:
        if refused_by_witness(n):
            continue
        want = CORPUS[n + "_rgb"]
        got = picture(witness(n, S.REFERENCE), S.REFERENCE)[:want.shape[0], :want.shape[1], ::-1]
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        planes = witness(n, S.REFERENCE)["rgb"][:want.shape[0], :want.shape[1]]      # libwebp's colour step on the REFERENCE planes
        dp = np.abs(planes.astype(np.int32) - want.astype(np.int32))
        rows.append((n, int((d > 0).sum()), d.size, int(d.max()), int((dp > 0).sum()), int(dp.max())))
    print("\nfile | samples that differ from libwebp | of | largest difference | with libwebp's colour step on the same planes: samples | largest")
    for r in rows:
        print("%-32s %6d %6d %4d %6d %4d" % r)
    same = [r[0] for r in rows if not r[1]]
    print(f"{len(rows)} files accepted, {len(same)} of them equal to libwebp; with libwebp's colour step {sum(not r[4] for r in rows)} equal, "
          f"median {int(np.median([r[4] * 100 // r[2] for r in rows]))} % of the samples off, {sum(r[5] > 64 for r in rows)} files by more than 64 levels")
    assert len(rows) > len(same)        # the day this fails, the default pixels ARE libwebp's and pixels="libwebp" has nothing to add


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_reference_made_fixtures(name):
    o, p = witness(name, S.REFERENCE), ops.webp_parse(file_bytes(name))
    assert not o["refused"] and not parse_differences(o, p)
    w, h, pitch = [int(x) for x in FRONT[f"{name}_dims"]]
    assert (o["width"], o["height"]) == (w, h)
    check_modes(o["modes"], FRONT[f"{name}_modes"])
    ref = FRONT[f"{name}_bgra"]
    rows, cols = min(h, 16 * o["mbrows"]), min(w, 16 * o["mbcols"])
    assert np.array_equal(planes_to_bgra(o)[:rows, :cols].reshape(rows, -1), ref[:rows, :4 * cols])


@pytest.mark.parametrize("name", UNPINNED)
def test_unpinned_fixtures_get_an_independent_witness(name):
    assert not tree_differences(name)


def test_every_deviation_is_live_and_minimal():
    """each flag switched on alone over SPEC moves at least one file, and switched off alone from REFERENCE breaks at least one; the
    table printed here is the one of DESIGN.md 4.19.  A file is decoded again only where its decode asked for the flag."""
    rows = []
    for flag in S.FLAGS:
        names = NAMES if flag in LIVE_ON_FIXTURES_ONLY else CNAMES
        counts = []
        for base, other in ((S.SPEC, frozenset([flag])), (S.REFERENCE, S.REFERENCE - {flag})):
            files = samples = verdicts = 0
            for n in names:
                a = witness(n, base)
                if a is not None and flag not in a["asked"] and flag != "reference_colour":
                    continue
                b = witness(n, other)
                if a is None or b is None or a["refused"] or b["refused"]:
                    changed = (a is None or a["refused"]) != (b is None or b["refused"])
                    verdicts += changed
                    files += changed
                    continue
                m = moved(picture(a, base), picture(b, other))
                parse = any(not np.array_equal(a[k], b[k]) for k in ("modes", "levels", "resmap", "quant", "filters"))
                files += bool(m or parse)
                samples += m
            counts += [files, samples, verdicts]
        rows.append((flag, *counts))
    print("\nflag | on alone over SPEC: files, samples, verdicts | off alone from REFERENCE: files, samples, verdicts")
    for r in rows:
        print("%-32s | %3d %7d %3d | %3d %7d %3d%s" % (*r, "   (golden fixtures)" if r[0] in LIVE_ON_FIXTURES_ONLY else ""))
    dead = [r[0] for r in rows if not r[1] or not r[4]]
    assert not dead, dead


@pytest.mark.parametrize("name", ["pil_noise_1x1_q80_m6", "pil_smooth_16x16_q95_m6", "wr_parts2", "pil_grey_1x1_q5_m0"])
def test_every_truncation_gets_a_code_or_a_parse(name):
    """host parser and witness accept the same cuts of a file and give the same arrays wherever they accept; the last file is one the
    reference's rules refuse whole"""
    base = data_of(name)
    accepted = 0
    for cut in range(len(base) + 1):
        data = base[:cut]
        rc, prc = _status(data)
        assert prc in (0, capi.FFHIP_EINVAL)
        try:
            o = S.decode(data, S.REFERENCE, pixels=False)
        except S.Refused:
            o = None
        assert (prc == 0) == (o is not None and not o["refused"]), cut
        if prc == 0:
            accepted += 1
            assert not parse_differences(o, ops.webp_parse(data)), cut
    assert (accepted >= 1) != refused_by_witness(name)
