"""A small VP8 key-frame WRITER for tests (as jpeg_writer.py is for JPEG): a bool encoder (RFC 6386 section 7.3) for the frame
header, and seeded random bytes behind it -- for the macroblock headers in the rest of the first partition and for the token
partitions.  Any bytes are a valid bool-coded stream, so every such file decodes to SOMETHING; what the tests pin is that the
library decodes it to what the reference's loader does.  This reaches what PIL cannot ask libwebp for: 2 / 4 token partitions,
the simple filter, segmentation with absolute and delta quantisers (negative sums included), mb_no_skip_coeff with many skips,
coefficient probabilities that make cat6 tokens with large extra bits common, quantiser index sweeps, a VP8X chunk."""
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


def coeff_update_probs():
    """RFC 6386 section 13.4, read out of the library's own table header (one copy of the constants in the tree)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ffpic_amd", "csrc", "ffhip_vp8_tables.h")
    txt = open(path).read()
    body = txt[txt.index("#define FFB_COEFF_UPDATE_PROBS"):txt.index("#define FFB_DEFAULT_COEFF_PROBS")]
    v = [int(x) for x in re.findall(r"\d+", body.split("{", 1)[1])]
    assert len(v) == 1056
    return v


def keyframe(width, height, seed, *, y_ac_qi=40, deltas=(0, 0, 0, 0, 0), log2_parts=0, filter_type=0, level=0, sharpness=0,
             segmentation=None, lf_adj=None, coeff_probs=None, prob_skip=None, p0_tail=600, token_bytes=6000, vp8x=None,
             trailing_chunk=None):
    """One lossy WebP file (bytes).
    segmentation: None, or dict(update_map=0/1, feature_mode=0/1, quant=(4 ints)|None, lf=(4 ints)|None, probs=(3 ints or None)|None)
                  -- quant / lf given means update_segment_feature_data = 1
    lf_adj:       None, or (ref_deltas[4], mode_deltas[4])
    coeff_probs:  None (no updates), or {flat index: probability} / a 1056-list of probabilities to set (None = keep)
    prob_skip:    None (mb_no_skip_coeff = 0) or prob_skip_false
    p0_tail / token_bytes: random bytes behind the header in the first partition / in EACH token partition
    vp8x:         None or (canvas_width_field, canvas_height_field) as stored
    trailing_chunk: bytes of a whole chunk appended behind the VP8 chunk"""
    rng = np.random.default_rng(seed)
    e = BoolEncoder()
    e.put(0)  # color_space
    e.put(0)  # clamp
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
        if s.get("update_map", 1):
            for p in (s.get("probs") or (None, None, None)):
                e.put(0 if p is None else 1)
                if p is not None:
                    e.bits(p, 8)
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
    p0 = e.flush() + rng.integers(0, 256, p0_tail, dtype=np.uint8).tobytes()
    nparts = 1 << log2_parts
    parts = [rng.integers(0, 256, token_bytes, dtype=np.uint8).tobytes() for _ in range(nparts)]
    assert len(p0) < (1 << 19)
    tag = (len(p0) << 5) | (1 << 4)  # key frame, version 0, show_frame
    frame = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", width, height) + p0
    for p in parts[:-1]:
        frame += struct.pack("<I", len(p))[:3]
    frame += b"".join(parts)
    body = b"WEBP"
    if vp8x is not None:
        body += b"VP8X" + struct.pack("<I", 10) + bytes(4) + struct.pack("<I", vp8x[0])[:3] + struct.pack("<I", vp8x[1])[:3]
    body += b"VP8 " + struct.pack("<I", len(frame)) + frame
    if trailing_chunk:
        body += trailing_chunk
    return b"RIFF" + struct.pack("<I", len(body)) + body
