"""A small VP8 key-frame WRITER for tests (as jpeg_writer.py is for JPEG), built on a bool encoder (RFC 6386 section 7.3), with two
entry points:

  keyframe()       the frame header bool-coded, seeded random bytes behind it for the macroblock headers and the token partitions.
                   Any bytes are a valid bool-coded stream, so every such file decodes to SOMETHING; what the tests pin on these
                   files is that the library decodes them to what the reference's loader does.  This reaches what PIL cannot ask
                   libwebp for: 2 / 4 / 8 token partitions, the simple filter, segmentation with absolute and delta quantisers
                   (negative sums included), mb_no_skip_coeff with many skips, coefficient probabilities that make cat6 tokens with
                   large extra bits common, quantiser index sweeps, a VP8X chunk.
  Both write what the REFERENCE reads (ffhip_webp.c): a segment id in every macroblock header also without segmentation, no RIFF padding
  byte.  valid=True writes what RFC 6386 and RIFF prescribe instead, so that libwebp takes the file (tests/golden/make_golden_libwebp.py).
  keyframe_from()  the WHOLE frame written from known data: per macroblock the y mode, the sixteen 4x4 modes, the uv mode, the
                   segment id, mb_skip_coeff and the 25 x 16 levels.  The macroblock headers follow the frame header in the SAME
                   encoder (the first partition is one stream); the tokens of row y go to partition y & (nparts - 1).  A decoder
                   is right on such a file when it returns what went in (tests/vp8_cases.py).  Partitions can be cut to the last
                   byte a decoder loads (`tight`), one of them a byte shorter (`short`), unread ones emptied (`empty_parts`).

decode() is a plain Python model of the library's parser (ffb_dec, ffb_mb_header, ffb_mb_tokens of ffhip_vp8_bool.h and the frame
header of ffhip_webp.c): modes, skips, levels, counts, and how many bytes of every partition the decoder loaded.

The trees, the zigzag, the bands and the cat probabilities below are restated from RFC 6386; the three large tables (coefficient
update probabilities, default coefficient probabilities, key-frame 4x4 mode probabilities) are read out of ffhip_vp8_tables.h, so that
there is one copy of them in the tree -- which also means writer and library would be wrong TOGETHER about a typo in them: the tests
that hold written files against the reference are what catches that."""
import collections
import os
import re
import struct

import numpy as np


class BoolEncoder:
    def __init__(self):
        self.out = bytearray()
        self.range, self.bottom, self.bit_count = 255, 0, 24

    def _carry(self):
        i = len(self.out) - 1
        while i >= 0 and self.out[i] == 255:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def put(self, bit, prob=128):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                self._carry()
            self.bottom = (self.bottom << 1) & 0xFFFFFFFF
            self.bit_count -= 1
            if not self.bit_count:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.bit_count = 8

    def bits(self, v, n):
        for k in range(n - 1, -1, -1):
            self.put((v >> k) & 1)

    def sbits(self, v, n):       # magnitude, then sign
        self.bits(abs(v), n)
        self.put(1 if v < 0 else 0)

    def flag_sbits(self, v, n):  # "present" flag, then the value
        self.put(1 if v else 0)
        if v:
            self.sbits(v, n)

    def flush(self):
        c, v = self.bit_count, self.bottom
        if v & (1 << (32 - c)):
            self._carry()
        v = (v << (c & 7)) & 0xFFFFFFFF
        c >>= 3
        while c > 0:
            v = (v << 8) & 0xFFFFFFFF
            c -= 1
        for _ in range(4):
            self.out.append(v >> 24)
            v = (v << 8) & 0xFFFFFFFF
        return bytes(self.out)


def _table(name, size):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ffpic_amd", "csrc", "ffhip_vp8_tables.h")
    txt = open(path).read()
    body = txt[txt.index("#define " + name):].split("{", 1)[1].split("}", 1)[0]
    v = [int(x) for x in re.findall(r"\d+", body)]
    assert len(v) == size
    return v


def coeff_update_probs():
    """RFC 6386 section 13.4, read out of the library's own table header (one copy of the constants in the tree)."""
    return _table("FFB_COEFF_UPDATE_PROBS", 1056)


def default_coeff_probs():
    """section 13.5, [4 types][8 bands][3 contexts][11 nodes] flat"""
    return _table("FFB_DEFAULT_COEFF_PROBS", 1056)


def kf_bmode_probs():
    """section 11.5, [10 above][10 left][9 nodes] flat"""
    return _table("FFB_KF_BMODE_PROBS", 900)


def _frame_header(e, *, y_ac_qi=40, deltas=(0, 0, 0, 0, 0), log2_parts=0, filter_type=0, level=0, sharpness=0, segmentation=None, lf_adj=None,
                  coeff_probs=None, prob_skip=None, valid=False):
    """the frame header into `e`; returns what it leaves for the macroblocks: the 1056 coefficient probabilities in force, whether a
    segment id is coded in every macroblock header and with which probabilities, prob_skip_false or None.  valid: what RFC 6386 has
    where the reference departs from it: no segment ids without segmentation, 255 for a segment probability that is not set"""
    e.put(0)  # color_space
    e.put(0)  # clamp
    seg_probs, ids_coded = (0, 0, 0), not valid   # segmentation off: an id is read all the same, with probabilities 0 (ffhip_vp8_bool.h)
    if segmentation is None:
        e.put(0)
    else:
        s = segmentation
        e.put(1)
        e.put(s.get("update_map", 1))
        data = s.get("quant") is not None or s.get("lf") is not None
        e.put(1 if data else 0)
        if data:
            e.put(s.get("feature_mode", 1))
            for v in (s.get("quant") or (0, 0, 0, 0)):
                e.flag_sbits(v, 7)
            for v in (s.get("lf") or (0, 0, 0, 0)):
                e.flag_sbits(v, 6)
        ids_coded = bool(s.get("update_map", 1))
        if s.get("update_map", 1):
            for p in (s.get("probs") or (None, None, None)):
                e.put(0 if p is None else 1)
                if p is not None:
                    e.bits(p, 8)
            seg_probs = tuple((255 if valid else 0) if p is None else p for p in (s.get("probs") or (None, None, None)))   # unset: 0, not 255 (the reference)
    e.put(filter_type)
    e.bits(level, 6)
    e.bits(sharpness, 3)
    if lf_adj is None:
        e.put(0)
    else:
        e.put(1)
        e.put(1)
        for group in lf_adj:
            for v in group:
                e.flag_sbits(v, 6)
    e.bits(log2_parts, 2)
    e.bits(y_ac_qi, 7)
    for v in deltas:
        e.flag_sbits(v, 4)
    e.put(0)  # refresh_entropy_probs
    upd = coeff_update_probs()
    if isinstance(coeff_probs, dict):
        want = [coeff_probs.get(i) for i in range(1056)]
    else:
        want = coeff_probs or [None] * 1056
    for i in range(1056):
        e.put(0 if want[i] is None else 1, upd[i])
        if want[i] is not None:
            e.bits(want[i], 8)
    e.put(0 if prob_skip is None else 1)
    if prob_skip is not None:
        e.bits(prob_skip, 8)
    probs = [d if w is None else w for d, w in zip(default_coeff_probs(), want)]
    return probs, ids_coded, seg_probs, prob_skip


def _container(width, height, p0, parts, vp8x=None, trailing_chunk=None, leading_chunk=None, riff_pad=False):
    """riff_pad: an odd-sized VP8 chunk gets the padding byte RIFF prescribes (the reference walks chunks without it, and so do the
    files written without this option: libwebp's demuxer refuses those)"""
    assert len(p0) < (1 << 19)
    tag = (len(p0) << 5) | (1 << 4)  # key frame, version 0, show_frame
    frame = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", width, height) + p0
    for p in parts[:-1]:
        frame += struct.pack("<I", len(p))[:3]
    frame += b"".join(parts)
    body = b"WEBP"
    if vp8x is not None:
        body += b"VP8X" + struct.pack("<I", 10) + bytes([vp8x[2] if len(vp8x) > 2 else 0, 0, 0, 0]) + struct.pack("<I", vp8x[0])[:3] + struct.pack("<I", vp8x[1])[:3]
    if leading_chunk:
        body += leading_chunk
    body += b"VP8 " + struct.pack("<I", len(frame)) + frame
    if riff_pad and len(frame) & 1:
        body += b"\x00"
    if trailing_chunk:
        body += trailing_chunk
    return b"RIFF" + struct.pack("<I", len(body)) + body


def keyframe(width, height, seed, *, p0_tail=600, token_bytes=6000, vp8x=None, trailing_chunk=None, valid=False, **header):
    """One lossy WebP file (bytes): the frame header, random bytes behind it.  `header`:
    y_ac_qi, deltas (5), log2_parts, filter_type, level, sharpness
    segmentation: None, or dict(update_map=0/1, feature_mode=0/1, quant=(4 ints)|None, lf=(4 ints)|None, probs=(3 ints or None)|None)
                  -- quant / lf given means update_segment_feature_data = 1
    lf_adj:       None, or (ref_deltas[4], mode_deltas[4])
    coeff_probs:  None (no updates), or {flat index: probability} / a 1056-list of probabilities to set (None = keep)
    prob_skip:    None (mb_no_skip_coeff = 0) or prob_skip_false
    p0_tail / token_bytes: random bytes behind the header in the first partition / in EACH token partition
    vp8x:         None or (canvas_width_field, canvas_height_field) as stored, a third entry being the flags byte
    trailing_chunk: bytes of a whole chunk appended behind the VP8 chunk
    valid:        the file as RFC 6386 and RIFF have it where the reference departs from them (_frame_header, _container)"""
    rng = np.random.default_rng(seed)
    e = BoolEncoder()
    _frame_header(e, valid=valid, **header)
    p0 = e.flush() + rng.integers(0, 256, p0_tail, dtype=np.uint8).tobytes()
    nparts = 1 << header.get("log2_parts", 0)
    parts = [rng.integers(0, 256, token_bytes, dtype=np.uint8).tobytes() for _ in range(nparts)]
    return _container(width, height, p0, parts, vp8x, trailing_chunk, riff_pad=valid)


# ---------------------------------------------------------------------------------------------------- the whole frame from known data
# RFC 6386, restated here and NOT read from the library's sources: a wrong nibble in ffhip_vp8_bool.h then shows as a wrong level
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)            # section 13: raster position of the n-th token
BANDS = (0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7)                   # section 13.3
PCAT = {3: (173, 148, 140), 4: (176, 155, 140, 135), 5: (180, 157, 141, 134, 130), 6: (254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129)}
CAT_BASE = {3: 11, 4: 19, 5: 35, 6: 67}
# the trees as (probability, bit) paths; modes numbered as in the mode records (include/ffpic_hip.h): y / uv 0 DC, 1 TM, 2 V, 3 H, 4 B_PRED
YMODE_PATH = {4: ((145, 0),), 0: ((145, 1), (156, 0), (163, 0)), 2: ((145, 1), (156, 0), (163, 1)), 3: ((145, 1), (156, 1), (128, 0)),
              1: ((145, 1), (156, 1), (128, 1))}                           # kf_ymode_tree, kf_ymode_prob (section 11.2)
UVMODE_PATH = {0: ((142, 0),), 2: ((142, 1), (114, 0)), 3: ((142, 1), (114, 1), (183, 0)), 1: ((142, 1), (114, 1), (183, 1))}
# bmode_tree (section 11.2) as (node, bit) paths; 4x4 modes 0 DC, 1 TM, 2 VE, 3 HE, 4 RD, 5 VR, 6 LD, 7 VL, 8 HD, 9 HU
BMODE_PATH = {0: ((0, 0),), 1: ((0, 1), (1, 0)), 2: ((0, 1), (1, 1), (2, 0)), 3: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 0)),
              4: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)), 5: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)),
              6: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 0)), 7: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)),
              8: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)), 9: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1))}
BLOCK_TYPE_Y_AFTER_Y2, BLOCK_TYPE_Y2, BLOCK_TYPE_UV, BLOCK_TYPE_Y = 0, 1, 2, 3


def token_path(v):
    """the coefficient token tree (section 13.2) below its end-of-block node, for a magnitude v >= 0:
    -> ([(node, bit)], [(probability, bit)] extra bits, token name)"""
    if v == 0:
        return [(1, 0)], [], "0"
    if v == 1:
        return [(1, 1), (2, 0)], [], "1"
    if v <= 4:
        return [(1, 1), (2, 1), (3, 0)] + ([(4, 0)] if v == 2 else [(4, 1), (5, v - 3)]), [], str(v)
    if v <= 6:
        return [(1, 1), (2, 1), (3, 1), (6, 0), (7, 0)], [(159, v - 5)], "cat1"
    if v <= 10:
        return [(1, 1), (2, 1), (3, 1), (6, 0), (7, 1)], [(165, (v - 7) >> 1), (145, (v - 7) & 1)], "cat2"
    cat = 3 if v <= 18 else 4 if v <= 34 else 5 if v <= 66 else 6
    assert v <= 67 + 2047
    nodes = [(1, 1), (2, 1), (3, 1), (6, 1), (8, int(cat >= 5)), (9 + (cat >= 5), 1 - (cat & 1))]
    nb = len(PCAT[cat])
    extra = [(PCAT[cat][k], (v - CAT_BASE[cat]) >> (nb - 1 - k) & 1) for k in range(nb)]
    return nodes, extra, f"cat{cat}"


def decoded_level(v):
    """what the library (and the reference) make of a written level: the eleven extra bits of cat6 are summed modulo 256"""
    a = abs(int(v))
    if a >= 67:
        a = 67 + ((a - 67) & 255)
    return -a if v < 0 else a


def _put_block(e, probs, btype, first, ctx, lv, zeros16, facts):
    """one block's tokens; lv: 16 levels at their raster positions.  Returns the token count as the library reports it: n - first
    at the end-of-block token, 16 when position 15 is coded."""
    c = [int(lv[ZIGZAG[n]]) for n in range(16)]
    assert first == 0 or c[0] == 0
    last = max([n for n in range(first, 16) if c[n]], default=-1)
    prev_zero = False
    for n in range(first, 16):
        base = btype * 264 + BANDS[n] * 33 + ctx * 11

        def put(node, bit):
            e.put(bit, probs[base + node])
            facts["slots"].add((btype, BANDS[n], ctx, node, bit))
        if not prev_zero:
            if n > last and not zeros16:
                put(0, 0)
                facts["tokens"]["EOB"] += 1
                return n - first
            put(0, 1)
        v = abs(c[n])
        nodes, extra, name = token_path(v)
        for node, bit in nodes:
            put(node, bit)
        for p, bit in extra:
            e.put(bit, p)
        facts["tokens"][name] += 1
        facts["positions"].add((btype, n, c[n]))
        if name >= "cat3" and name.startswith("cat"):
            bits = [b for _, b in extra]
            if not any(bits):
                facts["tokens"][name + "_extra_zeros"] += 1
            if all(bits):
                facts["tokens"][name + "_extra_ones"] += 1
        if v == 0:
            prev_zero, ctx = True, 0
            continue
        e.put(1 if c[n] < 0 else 0)
        prev_zero, ctx = False, 1 if v == 1 else 2
    return 16


def _put_mb_tokens(e, probs, has_y2, top, left, lv, z16, facts, mb):
    """ffb_mb_tokens the other way round; top / left: lists of nine 0/1 flags, updated.  -> 25 counts"""
    counts = [0] * 25
    first, ytype = 0, BLOCK_TYPE_Y
    if has_y2:
        facts["y2_ctx"][mb] = top[0] + left[0]
        counts[24] = _put_block(e, probs, BLOCK_TYPE_Y2, 0, top[0] + left[0], lv[24], z16[24], facts)
        top[0] = left[0] = int(counts[24] > 0)
        first, ytype = 1, BLOCK_TYPE_Y_AFTER_Y2
    for y in range(4):
        for x in range(4):
            b = y * 4 + x
            counts[b] = _put_block(e, probs, ytype, first, top[1 + x] + left[1 + y], lv[b], z16[b], facts)
            top[1 + x] = left[1 + y] = int(counts[b] > 0)
    b = 16
    for ch in (5, 7):
        for y in range(2):
            for x in range(2):
                counts[b] = _put_block(e, probs, BLOCK_TYPE_UV, 0, top[ch + x] + left[ch + y], lv[b], z16[b], facts)
                top[ch + x] = left[ch + y] = int(counts[b] > 0)
                b += 1
    return counts


def new_facts():
    return dict(slots=set(), tokens=collections.Counter(), positions=set(), bmode_triples=set(), bmode_kinds=set(), y2_ctx={})


def keyframe_from(width, height, mbs, *, zeros16=None, tight=False, short=None, empty_parts=(), pad=8, facts=None, vp8x=None, trailing_chunk=None,
                  leading_chunk=None, valid=False, **header):
    """One lossy WebP file (bytes) written from known macroblock data.  mbs: dict of arrays over the macroblocks in raster order,
      ymode [n] (0 DC, 1 TM, 2 V, 3 H, 4 B_PRED), bmodes [n][16] (read for B_PRED only), uvmode [n], seg [n], skip [n],
      levels [n][25][16] at their raster positions inside a block, blocks in the library's order (16 Y, 4 U, 4 V, Y2).
    zeros16 [n][25]: a block written WITHOUT an end-of-block token: explicit zero tokens behind its last non-zero level, up to
    position 15.  With all levels zero that gives count 16 and nothing non-zero: legal, though no encoder of pictures writes it.
    tight: every partition, the first included, ends on the last byte decode() loads;  short: "p0" or a token partition's number:
    that partition loses its last byte;  empty_parts: token partitions written with length 0;  pad: zero bytes behind every flushed
    partition otherwise.  `header` and `valid` as for keyframe(); leading_chunk: a whole chunk in front of the VP8 chunk.  facts (a new_facts() dict) receives what the stream visits, the token counts
    [n][25] (`counts`), the levels and the residual map a decoder must return (`levels`, `resmap`) and the bytes of every partition
    (`part_bytes`, the first partition first)."""
    facts = new_facts() if facts is None else facts
    assert not (tight and valid), "decode() below models the reference's reading, which is how `tight` finds the last byte"
    cols, rows = (((width + 3) & ~3) + 15) >> 4, (((height + 3) & ~3) + 15) >> 4
    n_mb = cols * rows
    nparts = 1 << header.get("log2_parts", 0)
    ymode, bmodes, uvmode, seg, skip, levels = [np.asarray(mbs[k]) for k in ("ymode", "bmodes", "uvmode", "seg", "skip", "levels")]
    assert len(ymode) == n_mb and levels.shape == (n_mb, 25, 16)
    z16 = np.zeros((n_mb, 25), bool) if zeros16 is None else np.asarray(zeros16, bool)
    bprobs = kf_bmode_probs()
    e = BoolEncoder()
    probs, ids_coded, seg_probs, prob_skip = _frame_header(e, valid=valid, **header)
    assert ids_coded or not seg.any(), "the map is kept: no ids are coded, every macroblock is segment 0"
    assert prob_skip is not None or not skip.any(), "mb_no_skip_coeff = 0: no macroblock can be skipped"
    te = [BoolEncoder() for _ in range(nparts)]
    top9 = [[0] * 9 for _ in range(cols)]
    bottom4 = [[0] * 4 for _ in range(cols)]      # the 4x4 modes along the bottom edge of the row above; the frame edge stands for DC
    counts = np.zeros((n_mb, 25), np.uint8)
    resmap = np.zeros(n_mb, np.int32)
    last_coded = -1
    for y in range(rows):
        left9, right4 = [0] * 9, [0] * 4
        for x in range(cols):
            mb = y * cols + x
            if ids_coded:
                s = int(seg[mb])
                e.put(s >> 1, seg_probs[0])
                e.put(s & 1, seg_probs[1 + (s >> 1)])
            if prob_skip is not None:
                e.put(int(skip[mb]), prob_skip)
            ym = int(ymode[mb])
            for p, bit in YMODE_PATH[ym]:
                e.put(bit, p)
            if ym == 4:
                im = [int(v) for v in bmodes[mb]]
                for i in range(16):
                    a = bottom4[x][i] if i < 4 else im[i - 4]
                    l = right4[i >> 2] if (i & 3) == 0 else im[i - 1]
                    for node, bit in BMODE_PATH[im[i]]:
                        e.put(bit, bprobs[(a * 10 + l) * 9 + node])
                    facts["bmode_triples"].add((a, l, im[i]))
                    if i < 4:
                        facts["bmode_kinds"].add(("above", "edge" if y == 0 else "bpred" if ymode[mb - cols] == 4 else f"i16_{int(ymode[mb - cols])}"))
                    if (i & 3) == 0:
                        facts["bmode_kinds"].add(("left", "edge" if x == 0 else "bpred" if ymode[mb - 1] == 4 else f"i16_{int(ymode[mb - 1])}"))
                bottom4[x], right4 = im[12:16], [im[3], im[7], im[11], im[15]]
            else:
                bottom4[x], right4 = [ym] * 4, [ym] * 4
            for p, bit in UVMODE_PATH[int(uvmode[mb])]:
                e.put(bit, p)
            has_y2 = ym != 4
            if not skip[mb]:
                counts[mb] = _put_mb_tokens(te[y & (nparts - 1)], probs, has_y2, top9[x], left9, levels[mb], z16[mb], facts, mb)
                last_coded = mb
                resmap[mb] = mb
            else:
                assert not levels[mb].any() and not z16[mb].any()
                for ctx in (top9[x], left9):          # a skipped macroblock clears the eight block flags, and the Y2 flag when it has a Y2 block
                    ctx[1:] = [0] * 8
                    if has_y2:
                        ctx[0] = 0
                resmap[mb] = last_coded if last_coded >= 0 else mb
    p0 = e.flush() + bytes(pad)
    parts = [t.flush() + bytes(pad) for t in te]
    if tight:
        loaded = decode(_container(width, height, p0, parts))["loaded"]
        p0, parts = p0[:loaded[0]], [p[:k] for p, k in zip(parts, loaded[1:])]
    for k in empty_parts:
        parts[k] = b""
    if short == "p0":
        p0 = p0[:-1]
    elif short is not None:
        parts[short] = parts[short][:-1]
    facts["counts"] = counts
    facts["levels"] = np.vectorize(decoded_level, otypes=[np.int16])(levels)
    facts["resmap"] = resmap
    facts["part_bytes"] = [len(p0)] + [len(p) for p in parts]
    return _container(width, height, p0, parts, vp8x, trailing_chunk, leading_chunk, riff_pad=valid)


# ---------------------------------------------------------------------------------------------------- the model decoder
class BoolDecoder:
    """ffb_dec: the range kept as the range, a byte loaded only when `count` is negative (the first one by the first decode), zeros
    and `err` beyond the partition"""

    def __init__(self, data, pos=0):
        self.p, self.pos, self.value, self.range, self.count, self.err = data, pos, 0, 255, -8, 0

    def _load(self):
        byte = 0
        if self.pos < len(self.p):
            byte = self.p[self.pos]
            self.pos += 1
        else:
            self.err = 1
        self.value = byte | (self.value << 8)
        self.count += 8

    def get(self, prob=128):
        if self.count < 0:
            self._load()
        rng, pos = self.range - 1, self.count
        split = (rng * prob) >> 8
        bit = (self.value >> pos) > split
        if bit:
            rng -= split
            self.value -= (split + 1) << pos
        else:
            rng = split + 1
        shift = 7 ^ (rng.bit_length() - 1)
        self.range = rng << shift
        self.count -= shift
        return int(bit)

    def bits(self, n):
        v = 0
        for k in range(n - 1, -1, -1):
            v |= self.get() << k
        return v

    def sbits(self, n):
        v = self.bits(n)
        return -v if self.get() else v

    def flag_sbits(self, n):
        return self.sbits(n) if self.get() else 0


def _walk(path_table, get):
    """decode with a table of (x, bit) paths: get(x) -> bit"""
    live = dict(path_table)
    k = 0
    while len(live) > 1 or k < len(next(iter(live.values()))):
        x = next(iter(live.values()))[k][0]
        bit = get(x)
        live = {m: p for m, p in live.items() if p[k] == (x, bit)}
        k += 1
    return next(iter(live))


def _get_block(d, probs, btype, first, ctx, out):
    prev_zero = False
    for n in range(first, 16):
        p = probs[btype * 264 + BANDS[n] * 33 + ctx * 11:][:11]
        if not prev_zero and not d.get(p[0]):
            return n - first
        if not d.get(p[1]):
            prev_zero, ctx = True, 0
            continue
        prev_zero = False
        if not d.get(p[2]):
            v = 1
        elif not d.get(p[3]):
            v = 2 if not d.get(p[4]) else 3 + d.get(p[5])
        elif not d.get(p[6]):
            if not d.get(p[7]):
                v = 5 + d.get(159)
            else:
                v = 7 + 2 * d.get(165)
                v += d.get(145)
        else:
            b1 = d.get(p[8])
            cat = 3 + 2 * b1 + d.get(p[9 + b1])
            extra = 0
            for q in PCAT[cat]:
                extra = (2 * extra + d.get(q)) & 255
            v = CAT_BASE[cat] + extra
        ctx = 1 if v == 1 else 2
        out[ZIGZAG[n]] = -v if d.get() else v
    return 16


def decode(data):
    """The library's parse restated: dict(modes [n][20], skip [n], levels [n][25][16], mbinfo [n][27], resmap [n], mbcols, mbrows,
    nparts, err, loaded = bytes loaded from the first partition and from every token partition, header_loaded = bytes of the
    first partition loaded by the frame header alone)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP"
    pos = 12
    while data[pos:pos + 4] != b"VP8 ":
        pos += 18 if data[pos:pos + 4] == b"VP8X" else 8 + struct.unpack("<I", data[pos + 4:pos + 8])[0]
    chunk_end = pos + 8 + struct.unpack("<I", data[pos + 4:pos + 8])[0]
    t = data[pos + 8:pos + 18]
    assert not t[0] & 1 and t[3:6] == b"\x9d\x01\x2a"
    p0_size = (t[0] | t[1] << 8 | t[2] << 16) >> 5
    fw, fh = struct.unpack("<HH", t[6:10])
    cols, rows = ((((fw & 0x3fff) + 3) & ~3) + 15) >> 4, ((((fh & 0x3fff) + 3) & ~3) + 15) >> 4
    p0_off = pos + 18
    d = BoolDecoder(data[p0_off:p0_off + p0_size])
    d.get(), d.get()
    seg_probs, ids_coded = [0, 0, 0], True
    if d.get():
        ids_coded = bool(d.get())
        if d.get():
            d.get()
            [d.flag_sbits(7) for _ in range(4)]
            [d.flag_sbits(6) for _ in range(4)]
        if ids_coded:
            for i in range(3):
                if d.get():
                    seg_probs[i] = d.bits(8)
    d.get(), d.bits(6), d.bits(3)
    if d.get() and d.get():
        [d.flag_sbits(6) for _ in range(8)]
    nparts = 1 << d.bits(2)
    sizes_at = p0_off + p0_size
    nxt = sizes_at + 3 * (nparts - 1)
    parts = []
    for i in range(nparts - 1):
        sz = data[sizes_at + 3 * i] | data[sizes_at + 3 * i + 1] << 8 | data[sizes_at + 3 * i + 2] << 16
        parts.append(data[nxt:nxt + sz])
        nxt += sz
    parts.append(data[nxt:min(len(data), chunk_end) if chunk_end >= nxt else len(data)])
    d.bits(7)
    [d.flag_sbits(4) for _ in range(5)]
    d.get()
    upd, probs = coeff_update_probs(), default_coeff_probs()
    for i in range(1056):
        if d.get(upd[i]):
            probs[i] = d.bits(8)
    no_skip = d.get()
    prob_skip = d.bits(8) if no_skip else 0
    header_loaded, header_err = d.pos, d.err
    bprobs = kf_bmode_probs()
    td = [BoolDecoder(p) for p in parts]
    n_mb = cols * rows
    modes, skips = np.zeros((n_mb, 20), np.uint8), np.zeros(n_mb, np.uint8)
    levels, mbinfo, resmap = np.zeros((n_mb, 25, 16), np.int16), np.zeros((n_mb, 27), np.uint8), np.zeros(n_mb, np.int32)
    top9 = [[0] * 9 for _ in range(cols)]
    bottom4 = [[0] * 4 for _ in range(cols)]
    last_coded = -1
    for y in range(rows):
        t = td[y & (nparts - 1)]
        left9, right4 = [0] * 9, [0] * 4
        for x in range(cols):
            mb = y * cols + x
            seg = 0
            if ids_coded:
                seg = d.get(seg_probs[1]) if not d.get(seg_probs[0]) else 2 + d.get(seg_probs[2])
            skip = d.get(prob_skip) if no_skip else 0
            ym = _walk(YMODE_PATH, lambda p: d.get(p))
            modes[mb, 0], modes[mb, 2], modes[mb, 18] = ym, ym, seg
            if ym == 4:
                im = [0] * 16
                for i in range(16):
                    a = bottom4[x][i] if i < 4 else im[i - 4]
                    l = right4[i >> 2] if (i & 3) == 0 else im[i - 1]
                    im[i] = _walk(BMODE_PATH, lambda node: d.get(bprobs[(a * 10 + l) * 9 + node]))
                modes[mb, 2:18] = im
                bottom4[x], right4 = im[12:16], [im[3], im[7], im[11], im[15]]
            else:
                bottom4[x], right4 = [ym] * 4, [ym] * 4
            modes[mb, 1] = _walk(UVMODE_PATH, lambda p: d.get(p))
            skips[mb] = skip
            has_y2 = ym != 4
            top = top9[x]
            if not skip:
                lv, cnt = levels[mb], mbinfo[mb]
                first, ytype = 0, BLOCK_TYPE_Y
                if has_y2:
                    cnt[24] = _get_block(t, probs, BLOCK_TYPE_Y2, 0, top[0] + left9[0], lv[24])
                    top[0] = left9[0] = int(cnt[24] > 0)
                    first, ytype = 1, BLOCK_TYPE_Y_AFTER_Y2
                for by in range(4):
                    for bx in range(4):
                        b = by * 4 + bx
                        cnt[b] = _get_block(t, probs, ytype, first, top[1 + bx] + left9[1 + by], lv[b])
                        top[1 + bx] = left9[1 + by] = int(cnt[b] > 0)
                b = 16
                for ch in (5, 7):
                    for by in range(2):
                        for bx in range(2):
                            cnt[b] = _get_block(t, probs, BLOCK_TYPE_UV, 0, top[ch + bx] + left9[ch + by], lv[b])
                            top[ch + bx] = left9[ch + by] = int(cnt[b] > 0)
                            b += 1
                last_coded = mb
                resmap[mb] = mb
            else:
                for ctx in (top, left9):
                    ctx[1:] = [0] * 8
                    if has_y2:
                        ctx[0] = 0
                resmap[mb] = last_coded if last_coded >= 0 else mb
            mbinfo[mb, 25], mbinfo[mb, 26] = has_y2, seg
    return dict(modes=modes, skip=skips, levels=levels, mbinfo=mbinfo, resmap=resmap, mbcols=cols, mbrows=rows, nparts=nparts,
                err=bool(header_err or d.err or any(t.err for t in td)), header_err=bool(header_err), loaded=[d.pos] + [t.pos for t in td],
                header_loaded=header_loaded, probs=probs)
