"""The corpus behind tests/golden/jpeg_front_pins.json: JPEG files, well-formed and not, and what the library's host front ends say of each.

cases() -> [(tag, data)], deterministic (numpy default_rng, no PIL).  Tags: `b.<seed>...` a baseline seed file and its mutations, `p.<seed>...` a
progressive one, `r.<name>...` one of the parse-time refusal files of test_jpeg_progressive.py, `h.<name>` a hand-made case -- one per difference
between the baseline and the progressive parser, and the malformations around them.
verdict(L, data) -> (digest, probe code, probe_any code, progressive flag): everything the front ends return for the file, through capi.lib() only.

A seed file is taken as it is and under seeded mutations of its header region (a baseline file: up to sixteen bytes behind its SOS segment; a
progressive file: all of it): a byte replaced, a bit flipped, one to three bytes inserted, the file cut, the file cut and an EOI stuck on."""
import ctypes as C
import functools
import hashlib
import os
import struct

import numpy as np

import jpeg_cases
import jpeg_progressive as P
import progressive_cases as PC
from ffpic_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("q80_grey", "q85_114", "q85_411", "q85_420", "q85_420_dri", "q88_422", "q92_444")
MUTATIONS = {"b": 120, "p": 120, "r": 40}
LUT_WORDS = 1536        # of ffhip_huff_gpu.hip
FILL = 0x5A5A           # what the output buffers hold before a call


# ---------------------------------------------------------------- files as lists of parts ----
def seg(marker, payload=b""):
    return ("seg", marker, bytes(payload))


def split(data):
    """SOI, then [("seg", marker, payload) | ("raw", bytes)]: marker segments, and between them whatever is none (entropy-coded bytes with their RSTn,
    an EOI, what follows it).  join(split(f)) == f for the well-formed files this is used on."""
    assert data[:2] == b"\xff\xd8"
    parts, p = [], 2
    while p < len(data):
        if data[p] == 0xFF and p + 3 < len(data) and (0xC0 <= data[p + 1] <= 0xCF or 0xDA <= data[p + 1] <= 0xFE):
            n = int.from_bytes(data[p + 2:p + 4], "big")
            parts.append(("seg", data[p + 1], bytes(data[p + 4:p + 2 + n])))
            p += 2 + n
            continue
        q = p
        while q < len(data) and not (data[q] == 0xFF and q + 1 < len(data) and (0xC0 <= data[q + 1] <= 0xCF or 0xDA <= data[q + 1] <= 0xFE)):
            q += 1
        parts.append(("raw", bytes(data[p:q])))
        p = q
    return parts


def join(parts):
    out = bytearray(b"\xff\xd8")
    for part in parts:
        if part[0] == "seg":
            out += bytes([0xFF, part[1]]) + (len(part[2]) + 2).to_bytes(2, "big") + part[2]
        else:
            out += part[1]
    return bytes(out)


def where(parts, marker, nth=0):
    return [i for i, part in enumerate(parts) if part[0] == "seg" and part[1] == marker][nth]


def edited(data, marker, fn, nth=0):
    """the file with the payload of its nth `marker` segment replaced by fn(payload)"""
    parts = split(data)
    i = where(parts, marker, nth)
    parts[i] = seg(marker, fn(bytearray(parts[i][2])))
    return join(parts)


def inserted(data, marker, new, nth=0, behind=False):
    """the file with the parts `new` put in front of (or behind) its nth `marker` segment"""
    parts = split(data)
    i = where(parts, marker, nth) + (1 if behind else 0)
    return join(parts[:i] + list(new) + parts[i:])


def _set(at, value):
    def fn(payload):
        payload[at] = value
        return payload
    return fn


# ---------------------------------------------------------------- the seed files ----
@functools.lru_cache(maxsize=None)
def baseline_seeds():
    out = [("fix_" + name, open(os.path.join(HERE, "golden", f"file_{name}.jpg"), "rb").read()) for name in FIXTURES]
    for layout, tables, restart in (("420", "annexk", 0), ("444", "deep23", 0), ("422", "ids23", 2), ("grey", "long", 3), ("h4v1", "shared", 0)):
        out.append((f"w_{layout}_{tables}_r{restart}", jpeg_cases.small(layout, tables, restart).data))
    return out


def _progressive(seed, width, height, h, v, ncomp, script, **kw):
    coef = P.random_coef(np.random.default_rng(seed), width, height, h, v, ncomp)
    return P.encode_progressive(width, height, h, v, coef, PC.QUANT[:2], script, **kw)


@functools.lru_cache(maxsize=None)
def progressive_seeds():
    return [("420_16x16", _progressive(11, 16, 16, 2, 2, 3, P.pil_script(3))),
            ("420_24x16_r2", _progressive(5, 24, 16, 2, 2, 3, P.pil_script(3), restart=2)),
            ("grey_16x16", _progressive(7, 16, 16, 1, 1, 1, P.pil_script(1))),
            ("444_17x9_deep", _progressive(9, 17, 9, 1, 1, 3, PC.DEEP))]


@functools.lru_cache(maxsize=None)
def refusal_seeds():
    import test_jpeg_progressive as T
    files = T._parse_time_refusals()
    assert len(files) == 16
    return [("".join(ch if ch.isalnum() else "_" for ch in name), data) for name, data in files.items()]


def header_end(data):
    """a baseline file's header region: up to sixteen bytes behind its SOS segment"""
    k = data.find(b"\xff\xda")
    return min(len(data), k + 2 + int.from_bytes(data[k + 2:k + 4], "big") + 16)


def mutations(data, region, n, rng):
    """n mutations of data[:region], in turn: byte, bit, insertion, cut, cut + EOI"""
    out = []
    for i in range(n):
        at = int(rng.integers(2, region))
        kind = ("byte", "bit", "insert", "cut", "cut_eoi")[i % 5]
        if kind == "byte":
            f = data[:at] + bytes([int(rng.integers(0, 256))]) + data[at + 1:]
        elif kind == "bit":
            f = data[:at] + bytes([data[at] ^ (1 << int(rng.integers(0, 8)))]) + data[at + 1:]
        elif kind == "insert":
            f = data[:at] + bytes(int(x) for x in rng.integers(0, 256, size=int(rng.integers(1, 4)))) + data[at:]
        elif kind == "cut":
            f = data[:at]
        else:
            f = data[:at] + b"\xff\xd9"
        out.append((f"{kind}{i:03d}", f))
    return out


# ---------------------------------------------------------------- the hand-made cases ----
def _exif(orientation):
    tiff = b"II*\0" + struct.pack("<IH", 8, 1) + struct.pack("<HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack("<I", 0)
    return seg(0xE1, b"Exif\0\0" + tiff)


def _dht(tc_th, counts, values):
    return seg(0xC4, bytes([tc_th]) + bytes(counts) + bytes(values))


def _hand_for(kind, good, grey, sof):
    """the cases both kinds of file get: kind `b` (frames are SOF0) or `p` (SOF2)"""
    out = {}
    prec2 = bytes([0x20]) + bytes(range(1, 193))
    out["dqt_precision_2"] = inserted(good, sof, [seg(0xDB, prec2)])
    out["dqt_precision_1"] = inserted(good, sof, [seg(0xDB, bytes([0x11]) + bytes(range(1, 129)))])
    out["dqt_precision_2_short"] = inserted(good, sof, [seg(0xDB, prec2[:130])])
    out["dqt_id_4"] = inserted(good, sof, [seg(0xDB, bytes([4]) + bytes(range(1, 65)))])
    out["dqt_behind_first_sos"] = inserted(good, 0xDA, [seg(0xDB, bytes([0]) + bytes(range(1, 65)))], behind=True)
    for m in (0xC8, 0xCC, 0xC1, 0xC3, 0xC9):
        out[f"segment_{m:02x}_before_sof"] = inserted(good, sof, [seg(m, b"\x00\x10")])
    out["second_sof_same"] = inserted(good, sof, [split(good)[where(split(good), sof)]])
    bad = bytearray(split(good)[where(split(good), sof)][2])
    bad[7] = 0x44                                                           # the first component 4 x 4: a layout both parsers refuse
    out["two_sof_first_refused_layout"] = inserted(good, sof, [seg(sof, bad)])
    out["two_sof_second_refused_layout"] = inserted(good, sof, [seg(sof, bad)], behind=True)
    out["eoi_before_first_sos"] = inserted(good, 0xDA, [("raw", b"\xff\xd9")])
    out["fill_bytes_before_markers"] = inserted(inserted(good, 0xC4, [("raw", b"\xff\xff")]), 0xDA, [("raw", b"\xff")])
    out["tem_and_rst_among_segments"] = inserted(inserted(good, 0xC4, [("raw", b"\xff\x01")]), sof, [("raw", b"\xff\xd3\xff\xd0")])
    for name, marker in (("dht", 0xC4), ("sos", 0xDA), ("sof", sof)):
        k = good.find(bytes([0xFF, marker]))
        for n in (2, 3, 4, 5):
            out[f"ends_{n}_bytes_into_{name}"] = good[:k + n]
        out[f"ends_with_tem_before_{name}"] = good[:k] + b"\xff\x01"
        out[f"ends_with_fill_before_{name}"] = good[:k] + b"\xff\xff\xff"
        out[f"eoi_instead_of_{name}"] = good[:k] + b"\xff\xd9"
        out[f"length_1_{name}"] = good[:k + 2] + b"\x00\x01" + good[k + 4:]
        out[f"length_past_end_{name}"] = good[:k + 2] + b"\xff\xff" + good[k + 4:]
    out["no_soi"] = b"\xff\xd7" + good[2:]
    out["byte_between_segments"] = inserted(good, 0xC4, [("raw", b"\x00")])
    dc = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    out["dht_class_2"] = inserted(good, 0xDA, [_dht(0x20, dc, range(12))])
    out["dht_id_4"] = inserted(good, 0xDA, [_dht(0x04, dc, range(12))])
    out["dht_257_values"] = inserted(good, 0xDA, [_dht(0x13, [0] * 8 + [32] * 7 + [33], range(256))])
    out["dht_256_values_id_3"] = inserted(good, 0xDA, [_dht(0x13, [0] * 8 + [32] * 8, range(256))])
    out["dht_over_subscribed"] = inserted(good, 0xDA, [_dht(0x02, [3] + [0] * 15, range(3))])
    out["dht_more_codes_than_values"] = inserted(good, 0xDA, [_dht(0x02, dc, range(5))])
    out["dht_all_ones_code"] = inserted(good, 0xDA, [_dht(0x12, [2] + [0] * 15, range(2))])
    out["dht_trailing_bytes"] = inserted(good, 0xDA, [seg(0xC4, bytes([0x03]) + bytes(dc) + bytes(range(12)) + b"\x00\x01\x02")])
    out["dri_of_one_byte"] = inserted(good, 0xDA, [seg(0xDD, b"\x02")])
    out["dri_of_three_bytes"] = inserted(good, 0xDA, [seg(0xDD, b"\x00\x00\x07")])
    out["single_component_says_2x2"] = edited(grey, sof, _set(7, 0x22))
    out["single_component_says_4x4"] = edited(grey, sof, _set(7, 0x44))
    out["luma_0x1"] = edited(good, sof, _set(7, 0x01))
    out["luma_3x2"] = edited(good, sof, _set(7, 0x32))
    out["chroma_2x1"] = edited(good, sof, _set(10, 0x21))
    out["tq_of_4"] = edited(good, sof, _set(8, 4))
    out["tq_of_3_undefined"] = edited(good, sof, _set(8, 3))
    out["precision_12"] = edited(good, sof, _set(0, 12))
    out["zero_width"] = edited(good, sof, lambda s: s[:3] + b"\0\0" + s[5:])
    out["zero_height"] = edited(good, sof, lambda s: s[:1] + b"\0\0" + s[3:])
    out["two_components"] = edited(good, sof, lambda s: s[:5] + b"\x02" + s[6:12])
    out["sof_cut_short"] = edited(good, sof, lambda s: s[:11])
    out["sos_component_not_in_frame"] = edited(good, 0xDA, _set(1, 9))
    out["no_sof"] = join([part for part in split(good) if part[:2] != ("seg", sof)])
    out["sos_before_sof"] = inserted(out["no_sof"], 0xDA, [split(good)[where(split(good), sof)]], behind=True)
    out["exif_in_front_of_another_app1"] = inserted(good, 0xDB, [_exif(6), seg(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>")])
    out["exif_behind_another_app1"] = inserted(good, 0xDB, [seg(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>"), _exif(8)])
    out["exif_behind_sos"] = inserted(good, 0xDA, [_exif(3)], behind=True)
    out["exif_behind_a_bad_segment"] = inserted(good, 0xDB, [seg(0xDB, b"\x05"), _exif(5)])
    out["two_exif"] = inserted(good, 0xDB, [_exif(2), _exif(4)])
    return {f"{kind}.{name}": f for name, f in out.items()}


@functools.lru_cache(maxsize=None)
def hand_made():
    """{tag: file}"""
    base = dict(baseline_seeds())
    prog = dict(progressive_seeds())
    good_b, grey_b = base["w_420_annexk_r0"], base["w_grey_long_r3"]
    good_p, grey_p = prog["420_16x16"], prog["grey_16x16"]
    out = {"b.pristine": good_b, "p.pristine_eoi_is_the_last_two_bytes": good_p}
    assert good_p[-2:] == b"\xff\xd9"
    out.update(_hand_for("b", good_b, grey_b, 0xC0))
    out.update(_hand_for("p", good_p, grey_p, 0xC2))
    # baseline only
    out["b.no_eoi"] = good_b[:-2] if good_b[-2:] == b"\xff\xd9" else good_b
    out["b.sof1"] = good_b.replace(b"\xff\xc0", b"\xff\xc1", 1)
    out["b.sos_ns_1_of_3"] = edited(good_b, 0xDA, lambda s: b"\x01" + s[1:3] + s[7:])
    out["b.sos_spectral_1_63"] = edited(good_b, 0xDA, _set(7, 1))
    out["b.sos_table_not_defined"] = edited(good_b, 0xDA, _set(2, 0x22))
    out["b.sos_table_id_4"] = edited(good_b, 0xDA, _set(2, 0x40))
    out["b.marker_in_the_scan"] = good_b[:header_end(good_b)] + b"\xff\xc4" + good_b[header_end(good_b):]
    # progressive only
    out["p.no_eoi"] = good_p[:-2]
    out["p.bytes_behind_eoi"] = good_p + b"\x00\xff\xda"
    out["p.eoi_before_second_sos"] = inserted(good_p, 0xDA, [("raw", b"\xff\xd9")], nth=1)
    out["p.sos_ns_2_of_3"] = edited(good_p, 0xDA, lambda s: b"\x02" + s[1:5] + s[7:])
    out["p.sos_ns_0"] = edited(good_p, 0xDA, lambda s: b"\x00" + s[7:])
    out["p.sos_components_out_of_order"] = edited(good_p, 0xDA, lambda s: s[:1] + s[3:5] + s[1:3] + s[5:])
    out["p.sos_component_twice"] = edited(good_p, 0xDA, lambda s: s[:3] + s[1:3] + s[5:])
    out["p.sos_al_14"] = edited(good_p, 0xDA, _set(-1, 14))
    # a DHT redefined under the same id between scans: what the writer's per-scan optimal tables are already
    heads = [part[2][0] for part in split(good_p) if part[:2] == ("seg", 0xC4)]
    assert len(heads) > len(set(heads))
    out["p.dht_redefined_between_scans"] = good_p
    # a DRI redefined between scans: the first scan of the file without restart markers, a DRI, the other scans of the file with them
    coef = P.random_coef(np.random.default_rng(21), 24, 16, 2, 2, 3)
    plain, marked = (split(P.encode_progressive(24, 16, 2, 2, coef, PC.QUANT[:2], P.pil_script(3), restart=r)) for r in (0, 2))
    cut_a, cut_b = where(plain, 0xDA) + 2, where(marked, 0xDA) + 2
    out["p.dri_redefined_between_scans"] = join(plain[:cut_a] + [seg(0xDD, b"\x00\x02")] + marked[cut_b:])
    out["p.dri_dropped_between_scans"] = join(marked[:cut_b] + [seg(0xDD, b"\x00\x00")] + plain[cut_a:])
    out["p.dri_redefined_data_unchanged"] = inserted(good_p, 0xDA, [seg(0xDD, b"\x00\x01")], nth=1)
    return {"h." + tag: f for tag, f in out.items()}


# where the two parsers' policies stand against each other: (the baseline file, the progressive file) whose codes -- ffhip_jpeg_probe's for the
# first, the progressive leg of ffhip_jpeg_probe_any for the second -- differ
TWINS = {
    "DQT precision": ("h.b.dqt_precision_2", "h.p.dqt_precision_2"),
    "DQT position": ("h.b.dqt_behind_first_sos", "h.p.dqt_behind_first_sos"),
    "repeated SOF": ("h.b.two_sof_first_refused_layout", "h.p.two_sof_first_refused_layout"),
    "other frame markers": ("h.b.segment_c8_before_sof", "h.p.segment_c8_before_sof"),
    "EOI": ("h.b.eoi_before_first_sos", "h.p.eoi_before_second_sos"),
    "where the parsers stop": ("h.b.no_eoi", "h.p.no_eoi"),
}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for kind, seeds in (("b", baseline_seeds()), ("p", progressive_seeds()), ("r", refusal_seeds())):
        for k, (name, data) in enumerate(seeds):
            rng = np.random.default_rng([ord(kind), k])
            out.append((f"{kind}.{name}", data))
            region = header_end(data) if kind == "b" else len(data)
            out += [(f"{kind}.{name}.{tag}", f) for tag, f in mutations(data, region, MUTATIONS[kind], rng)]
    out += sorted(hand_made().items())
    assert len({tag for tag, _ in out}) == len(out)
    return out


# ---------------------------------------------------------------- what the library says of a file ----
def _planes(g):
    return [np.full(max(n, 1) * 64, FILL, np.uint16) for n in (g.y_blocks, g.c_blocks, g.c_blocks)]


def verdict(L, data):
    """-> (digest, ffhip_jpeg_probe's code, ffhip_jpeg_probe_any's code, its progressive flag)"""
    h = hashlib.blake2b(digest_size=8)
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()   # exact size
    ptr, n = buf.ctypes.data, buf.size
    put = lambda *ints: h.update(struct.pack(f"<{len(ints)}i", *ints))
    geom = lambda g: (g.mcu_cols, g.mcu_rows, g.ncomp, g.h, g.v, *g.qt_id)
    tiny = capi.jpeg_geom(1, 1, h=1, v=1, ncomp=1)          # expected where the probe refused: a decode that parses after all writes 64 values

    g, w, hh = capi.JpegGeom(), C.c_int(-1), C.c_int(-1)
    rc_probe = L.ffhip_jpeg_probe(ptr, n, C.byref(g), C.byref(w), C.byref(hh))
    put(rc_probe, *geom(g), w.value, hh.value)
    ga, wa, ha, pg = capi.JpegGeom(), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc_any = L.ffhip_jpeg_probe_any(ptr, n, C.byref(ga), C.byref(wa), C.byref(ha), C.byref(pg))
    put(rc_any, *geom(ga), wa.value, ha.value, pg.value)
    o = C.c_int(-1)
    put(L.ffhip_jpeg_exif_orientation(ptr, n, C.byref(o)), o.value)

    ge = g if rc_probe == 0 else tiny
    planes, q = _planes(ge), np.full(256, FILL, np.uint16)
    rc = L.ffhip_jpeg_entropy_decode(ptr, n, C.byref(ge), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, q.ctypes.data)
    put(rc)
    if rc == 0:
        for a in planes + [q]:
            h.update(a.tobytes())
    gp = ga if rc_any == 0 and pg.value == 1 else tiny
    for k_max in (63, 5):
        planes, q = _planes(gp), np.full(256, FILL, np.uint16)
        rc = L.ffhip_jpeg_progressive_decode(ptr, n, C.byref(gp), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data,
                                             q.ctypes.data, k_max)
        put(rc)
        for a in planes:
            h.update(a.tobytes())
        last = (C.c_int * 5)()
        put(L.ffhip_debug_progressive_last(last), *last)
    L.ffhip_jpeg_lut_test.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ffhip_jpeg_lut_test.restype = C.c_int
    for which in range(8):
        lut =np.full(LUT_WORDS, FILL, np.uint16)
        rc = L.ffhip_jpeg_lut_test(ptr, n, which, lut.ctypes.data)
        put(rc)
        if rc == 0:
            h.update(lut.tobytes())
    return h.hexdigest(), rc_probe, rc_any, pg.value
