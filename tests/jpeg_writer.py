"""Minimal baseline-JPEG WRITER (Huffman, interleaved scan, optional restart intervals) used ONLY to build test fixtures:
it turns quantised coefficient planes in MCU order (what tests/jpeg_entropy.py::decode produces and the reconstruction
stage consumes) plus natural-order quant tables into a .jpg any baseline decoder reads -- the way to get files with
sampling layouts PIL cannot write (4:1:1 = h4v1, h1v4).  Annex K's typical Huffman tables (ITU-T T.81 K.3-K.6) unless the caller
brings tables of its own (deep_tables, long_tables, short_dc_tables, ones_tables below, under any of the ids 0..3): with arbitrary tables and
arbitrary coefficients a file has its answer by construction (tests/jpeg_cases.py).  Written from T.81; test infrastructure, not product code.
"""
import numpy as np

from jpeg_entropy import ZZ

DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
         0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
         0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
         0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
         0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
         0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
         0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
         0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
         0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
         0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
         0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
         0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


# ---- other Huffman tables than Annex K's, for the tests that pin the decoders on written coefficients.  Every builder returns the `tables=` of
# encode(): {(0, 0), (1, 0)} for luma, {(0, 1), (1, 1)} for chroma (with_ids moves them).  Every code is valid: the Kraft sum stays below 1, so no code
# is all ones, and every symbol a baseline scan can hold is there (12 DC sizes; the 162 AC symbols of Annex K).
COMMON_AC = [0x00, 0xF0, 0x01, 0x02, 0x03, 0x11, 0x04, 0x21, 0x12, 0x05, 0xF1, 0xE1, 0x06, 0x31, 0x07, 0x41, 0x08, 0x13, 0x09, 0x22, 0x0A, 0xF2, 0xE2, 0x51]
SHORT_AC = [0xFA, 0xF9, 0xEA, 0xE9]        # run 14 / 15 with a size of 9 / 10: what no test content holds takes the short codes


def kraft(counts):
    """the Kraft sum of a DHT's code counts, in units of 2^-16 (a valid table: below 65 536)"""
    return sum(n << (16 - length) for length, n in enumerate(counts, 1))


def _ac_rest(first):
    return list(first) + [x for x in AC_L[1] if x not in first]


def deep_tables():
    """Long codes under MORE nine-bit prefixes than the device look-up table has groups for (8).  AC: two 3-bit codes, forty 10-bit codes (twenty
    prefixes), twenty codes of every length 11..16 (another ten).  The groups go to the first eight prefixes, in the order of (length, code):
    the first sixteen 10-bit codes, which rare symbols get; EOB, ZRL and the small run/size pairs (COMMON_AC) are dealt out over the codes
    behind them, of every length 10..16 -- all under prefixes WITHOUT a group.  DC: twelve codes of 10..16 bits (a few prefixes: groups).  Luma and
    chroma differ in which symbol gets which code."""
    ac_counts = [0, 0, 2, 0, 0, 0, 0, 0, 0, 40, 20, 20, 20, 20, 20, 20]
    dc_counts = [0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 2, 2, 1, 1, 1, 1]
    out = {}
    for tid in (0, 1):
        common = COMMON_AC[tid:] + COMMON_AC[:tid]
        rare = [x for x in AC_L[1] if x not in common and x not in SHORT_AC[:2]]
        per = {length: [] for length in range(10, 17)}
        for i, sym in enumerate(common):
            per[10 + i % 7].append(sym)
        syms = SHORT_AC[:2] + [rare.pop() for _ in range(16)] + per[10] + [rare.pop() for _ in range(24 - len(per[10]))]
        for length in range(11, 17):
            syms += per[length] + [rare.pop() for _ in range(20 - len(per[length]))]
        assert not rare and sorted(syms) == sorted(AC_L[1])
        out[(1, tid)] = (ac_counts, syms)
        out[(0, tid)] = (dc_counts, [(x + 5 * tid) % 12 for x in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)])   # luma: size 11 has the 16-bit code
    return out


def long_tables():
    """Every DC size and every AC symbol but SHORT_AC has a 16-bit code (DC size 11 then takes 27 bits, an AC coefficient of size 10 takes 26); the four
    of SHORT_AC take one code of 1 bit and three of 8 (the DC tables have no symbol to spare: twelve 16-bit codes)."""
    ac_counts = [1, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 158]
    dc_counts = [0] * 15 + [12]
    out = {}
    for tid in (0, 1):
        rest = [x for x in AC_L[1] if x not in SHORT_AC]
        out[(1, tid)] = (ac_counts, SHORT_AC + (rest if tid == 0 else rest[::-1]))
        out[(0, tid)] = (dc_counts, list(range(12)) if tid == 0 else list(range(11, -1, -1)))
    return out


def short_dc_tables():
    """ONE pair for all components (table_ids = ((0, 0),) * 3): the 12 DC symbols only, in twelve 4-bit codes, beside Annex K's luma AC table"""
    return {(0, 0): ([0, 0, 0, 12] + [0] * 12, list(range(12))), (1, 0): AC_L}


def ones_tables():
    """Annex K's code lengths, their Kraft sum one code short of 1, with the symbols in another order: the frequent ones (COMMON_AC, the large DC sizes)
    get the LAST codes -- 16-bit codes that start with nine to fifteen ones, DC codes of 7..9 bits that are ones but for the last bit.  With magnitudes
    that are all ones behind them the scan is dense in 0xFF, and so in stuffed zeros."""
    out = {}
    for tid, (dcc, acc) in enumerate(((DC_L[0], AC_L[0]), (DC_C[0], AC_C[0]))):
        out[(1, tid)] = (acc, [x for x in AC_L[1] if x not in COMMON_AC] + COMMON_AC[::-1])
        out[(0, tid)] = (dcc, list(range(12)))
    return out


def with_ids(tables, ids):
    """tables of a builder under other ids: ids = {(class, id): new id}"""
    return {(tc, ids.get((tc, th), th)): t for (tc, th), t in tables.items()}


def _codes(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


class _BitOut:
    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        self.bits += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)      # byte stuffing
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)   # pad with ones


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _block(bo, blk, pred, dc, ac, seen=None):
    """one data unit: DC difference then run-length AC in zigzag order (T.81 F.1.2); seen: the symbols as they are emitted, (class, symbol)"""
    d = int(blk[0]) - pred
    t = abs(d).bit_length()
    bo.put(*dc[t])
    if seen is not None:
        seen.append((0, t))
    if t:
        bo.put(d if d > 0 else d + (1 << t) - 1, t)
    run = 0
    zz = blk[ZZ]
    last = int(np.max(np.nonzero(zz)[0])) if np.any(zz[1:]) else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bo.put(*ac[0xF0])
            if seen is not None:
                seen.append((1, 0xF0))
            run -= 16
        t = abs(v).bit_length()
        bo.put(*ac[(run << 4) | t])
        if seen is not None:
            seen.append((1, (run << 4) | t))
        bo.put(v if v > 0 else v + (1 << t) - 1, t)
        run = 0
    if last < 63:
        bo.put(*ac[0x00])
        if seen is not None:
            seen.append((1, 0x00))
    return int(blk[0])


def encode(width, height, h, v, coef, quant, qt_id=(0, 1, 1), restart=0, *, tables=None, table_ids=None, stats=None):
    """coef: per component int16 [blocks][64] natural order, blocks in MCU order (luma h*v per MCU, chroma 1); quant: uint16 [4][64] natural
    order; width / height: picture size in pixels (<= the coded size the MCU counts imply).  Returns the file's bytes.
    tables: {(class, id): (counts[16], symbols)}, class 0 DC / 1 AC, id 0..3 -- the file's DHT segments (Annex K's when None);
    table_ids: per component (dc id, ac id) ((0, 0), (1, 1), (1, 1) when None).
    stats: a dict the writer fills with what it emitted -- "symbols": {(class, id, symbol): times}, "block_bits": bits of every data unit in scan
    order (code and magnitude bits, without padding and stuffing), "dc_diffs": (smallest, largest) DC difference, "zrl_in_a_row": the longest
    run of ZRL symbols."""
    ncomp = len([c for c in coef if c is not None])
    mcu_cols, mcu_rows = -(-width // (8 * h)), -(-height // (8 * v))
    if tables is None:
        tables = {(0, 0): DC_L, (1, 0): AC_L}
        if ncomp == 3:
            tables.update({(0, 1): DC_C, (1, 1): AC_C})
    if table_ids is None:
        table_ids = ((0, 0), (1, 1), (1, 1))
    out = bytearray(b"\xFF\xD8")
    for t in sorted(set(qt_id[:ncomp])):
        out += _seg(0xDB, bytes([t]) + bytes(int(x) for x in np.asarray(quant[t])[ZZ]))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        sof += bytes([c + 1, ((h if c == 0 else 1) << 4) | (v if c == 0 else 1), qt_id[c]])
    out += _seg(0xC0, sof)
    for (tc, th) in sorted(tables, key=lambda k: (k[1], k[0])):
        counts, syms = tables[(tc, th)]
        out += _seg(0xC4, bytes([(tc << 4) | th]) + bytes(counts) + bytes(syms))
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, "big"))
    sos = bytes([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, (table_ids[c][0] << 4) | table_ids[c][1]])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    dc = [_codes(*tables[(0, table_ids[c][0])]) for c in range(ncomp)]
    ac = [_codes(*tables[(1, table_ids[c][1])]) for c in range(ncomp)]
    bo = _BitOut()
    pred = [0, 0, 0]
    nb = [h * v, 1, 1]
    planes = [np.asarray(c).reshape(-1, 64) if c is not None else None for c in coef]
    rst = 0
    seen = [] if stats is not None else None
    if stats is not None:
        stats.update(symbols={}, block_bits=[], dc_diffs=(0, 0), zrl_in_a_row=0)
    done_bits = 0
    for mcu in range(mcu_cols * mcu_rows):
        if restart and mcu and mcu % restart == 0:
            bo.flush()
            out += bo.out + bytes([0xFF, 0xD0 + (rst & 7)])
            bo = _BitOut()
            done_bits = 0
            rst += 1
            pred = [0, 0, 0]
        for c in range(ncomp):
            for k in range(nb[c]):
                before = pred[c]
                pred[c] = _block(bo, planes[c][mcu * nb[c] + k], pred[c], dc[c], ac[c], seen)
                if stats is not None:
                    stats["block_bits"].append(bo.bits - done_bits)
                    done_bits = bo.bits
                    lo, hi = stats["dc_diffs"]
                    stats["dc_diffs"] = (min(lo, pred[c] - before), max(hi, pred[c] - before))
                    zrl = 0
                    for (cls, sym) in seen:
                        key = (cls, table_ids[c][cls], sym)
                        stats["symbols"][key] = stats["symbols"].get(key, 0) + 1
                        zrl = zrl + 1 if (cls, sym) == (1, 0xF0) else 0
                        stats["zrl_in_a_row"] = max(stats["zrl_in_a_row"], zrl)
                    seen.clear()
    bo.flush()
    out += bo.out + b"\xFF\xD9"
    return bytes(out)
