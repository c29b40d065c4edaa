"""zlib streams for the tests of the wave form of inflate (test_inflate_model.py on the host model, test_inflate_gpu.py on k_inflate): the
cases of test_inflate.py, hand-written streams (all through test_inflate.Bits, each checked against what it was written from and against
zlib), and the damaged set -- every proper prefix and every single-bit flip of one stream of about 300 bytes.  Built once, shared."""
import zlib

import numpy as np

from test_inflate import CASES, Bits, deflate, mixed, zwrap

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(n):
    """match length -> (symbol - 257, extra bits' value)"""
    s = 28 if n == 258 else max(k for k in range(28) if LEN_BASE[k] <= n)
    return s, n - LEN_BASE[s]


def distance_symbol(d):
    s = max(k for k in range(30) if DIST_BASE[k] <= d)
    return s, d - DIST_BASE[s]


def canonical(lengths):
    """{symbol: length} -> {symbol: (code, length)}, RFC 1951 3.2.2"""
    code, out = 0, {}
    for bits in range(1, 16):
        for sym in sorted(s for s, l in lengths.items() if l == bits):
            out[sym] = (code, bits)
            code += 1
        code <<= 1
    return out


def copy_match(out, n, d):
    assert 1 <= d <= len(out)
    for _ in range(n):
        out.append(out[-d])


def fixed_match(b, n, d):
    s, extra = length_symbol(n)
    b.fixed_literal(257 + s).field(extra, LEN_EXTRA[s])
    s, extra = distance_symbol(d)
    b.code(s, 5).field(extra, DIST_EXTRA[s])


def long_codes():
    """One dynamic block.  Its literal/length tree has sixteen symbols with code lengths 1 .. 15, 15 -- 256, 257 and 285 among them, 285
    with one of the two 15-bit codes -- and its distance tree the symbols 0 .. 15 with lengths 1 .. 15, 15: every code length there is,
    the ten-bit table look-up and the walk behind it.  The code-length code: symbols 0 .. 15 and 18, fifteen of four bits and two of five"""
    lit_syms = [65, 66, 67, 68, 69, 70, 71, 72, 257, 73, 74, 75, 0, 256, 76, 285]
    lit_len = {s: min(k + 1, 15) for k, s in enumerate(lit_syms)}
    dist_len = {s: min(s + 1, 15) for s in range(16)}
    assert sum(2.0 ** -l for l in lit_len.values()) == 1 and sum(2.0 ** -l for l in dist_len.values()) == 1
    lit, dist = canonical(lit_len), canonical(dist_len)
    clen_len = {s: 4 for s in range(15)}
    clen_len.update({15: 5, 18: 5})
    clen = canonical(clen_len)
    b = Bits().field(1, 1).field(2, 2).field(286 - 257, 5).field(16 - 1, 5).field(19 - 4, 4)
    for s in CLEN_ORDER:
        b.field(clen_len.get(s, 0), 3)
    seq = [lit_len.get(s, 0) for s in range(286)] + [dist_len[s] for s in range(16)]
    k = 0
    while k < len(seq):                                               # lengths as they are, runs of zeros as symbol 18
        run = 0
        while k + run < len(seq) and seq[k + run] == 0 and run < 138:
            run += 1
        if run >= 11:
            b.code(*clen[18]).field(run - 11, 7)
            k += run
        else:
            b.code(*clen[seq[k]])
            k += 1
    out = bytearray()
    for s in (65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 0, 76):     # every literal of the tree
        b.code(*lit[s])
        out.append(s)
    b.code(*lit[257]).code(*dist[0])                                  # length 3 at distance 1
    copy_match(out, 3, 1)
    b.code(*lit[285]).code(*dist[1])                                  # length 258 at distance 2
    copy_match(out, 258, 2)
    for s in range(2, 16):                                            # every other distance code, its extra bits all ones
        b.code(*lit[257]).code(*dist[s]).field((1 << DIST_EXTRA[s]) - 1, DIST_EXTRA[s])
        copy_match(out, 3, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)
    b.code(*lit[256])
    return zwrap(b.done(), bytes(out)), bytes(out)


def distances_and_lengths():
    """one fixed block: 32768 literals, then every pair of the distances 1, 2, 7, 8, 63, 64, 65, 32768 and the lengths 3, 4, 63, 64, 65,
    257, 258, a literal between two matches"""
    out = bytearray(np.random.default_rng(31).integers(0, 256, 32768, dtype=np.uint8).tobytes())
    b = Bits().field(1, 1).field(1, 2)
    for v in out:
        b.fixed_literal(v)
    for d in (1, 2, 7, 8, 63, 64, 65, 32768):
        for n in (3, 4, 63, 64, 65, 257, 258):
            fixed_match(b, n, d)
            copy_match(out, n, d)
            b.fixed_literal((d + n) & 255)
            out.append((d + n) & 255)
    b.fixed_literal(256)
    return zwrap(b.done(), bytes(out)), bytes(out)


def stored_lengths():
    """stored blocks of LEN 0, 1 and 65535, the first behind three bits of a byte, the others at a byte boundary"""
    data = mixed(65536, 32)
    b, at = Bits(), 0
    for k, n in enumerate((0, 1, 65535)):
        b.field(1 if k == 2 else 0, 1).field(0, 2)
        if b.n:
            b.field(0, 8 - b.n)
        b.field(n, 16).field(n ^ 0xffff, 16)
        for v in data[at:at + n]:
            b.field(v, 8)
        at += n
    assert at == 65536
    return zwrap(b.done(), data), data


def two_hundred_blocks():
    """blocks of all three types in turn: raw deflate pieces of zlib at levels 0, 1 and 9 and with Z_FIXED, each ended by Z_FULL_FLUSH
    (an empty stored block), then a last empty fixed block"""
    rng = np.random.default_rng(33)
    raw, data = b"", b""
    hows = (dict(level=0), dict(level=1), dict(level=9), dict(level=6, strategy=zlib.Z_FIXED))
    blocks = 0
    for k in range(100):
        piece = mixed(int(rng.integers(1, 700)), 100 + k)
        how = hows[k % 4]
        co = zlib.compressobj(how["level"], zlib.DEFLATED, -15, 9, how.get("strategy", zlib.Z_DEFAULT_STRATEGY))
        raw += co.compress(piece) + co.flush(zlib.Z_FULL_FLUSH)
        data += piece
        blocks += 2
    raw += Bits().field(1, 1).field(1, 2).fixed_literal(256).done()
    assert blocks >= 200
    return zwrap(raw, data), data


_VALID = None


def valid():
    """{name: (stream, what it holds)}: test_inflate.CASES and the hand-written streams that are good"""
    global _VALID
    if _VALID is None:
        _VALID = {name: (deflate(data, **how), data) for name, (data, how) in CASES.items()}
        _VALID["one_code_distance_tree"] = one_code_distance_tree()
        for make in (long_codes, distances_and_lengths, stored_lengths, two_hundred_blocks):
            _VALID[make.__name__] = make()
        for name, (z, data) in _VALID.items():
            assert zlib.decompress(z) == data, name
    return _VALID


def one_code_distance_tree():
    """test_inflate.test_one_code_distance_tree_is_taken_as_zlib_takes_it's stream"""
    lengths = [0] * 258 + [1]
    lengths[65], lengths[256], lengths[257] = 1, 2, 2
    b = Bits().field(1, 1).field(2, 2).field(1, 5).field(0, 5).field(14, 4)
    clen = {0: 2, 1: 2, 2: 2, 18: 2}
    for k in range(18):
        b.field(clen.get(CLEN_ORDER[k], 0), 3)
    codes = {0: 0, 1: 1, 2: 2, 18: 3}
    for sym, extra in ((18, 65 - 11), (1, None), (18, 138 - 11), (18, 52 - 11), (2, None), (2, None), (1, None)):
        b.code(codes[sym], 2)
        if extra is not None:
            b.field(extra, 7)
    b.code(0, 1).code(0b11, 2).code(0, 1).code(0b10, 2)
    return zwrap(b.done(), b"AAAA"), b"AAAA"


def refused_by_hand():
    """{name: stream}: the hand-written streams of test_inflate.py that every inflate refuses"""
    out = {"block_type_3": zwrap(Bits().field(1, 1).field(3, 2).done(), b"")}
    b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(257).code(1, 5).fixed_literal(256)
    out["distance_beyond_the_start"] = zwrap(b.done(), b"AAAA")
    b = Bits().field(1, 1).field(2, 2).field(0, 5).field(0, 5).field(15, 4)
    for k in range(19):
        b.field(1 if k < 3 else 0, 3)
    out["oversubscribed_code_lengths"] = zwrap(b.done() + b"\x00" * 8, b"")
    for sym in (286, 287):
        b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(sym).code(0, 5).fixed_literal(256)
        out[f"length_symbol_{sym}"] = zwrap(b.done(), b"AAAA")
    for sym in (30, 31):
        b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(257).code(sym, 5).fixed_literal(256)
        out[f"distance_symbol_{sym}"] = zwrap(b.done(), b"AAAA")
    return out


_DAMAGED = None


def damaged():
    """(the good stream, its bytes, [every proper prefix, then every single-bit flip]) of a level-9 stream of mixed(330, 10)"""
    global _DAMAGED
    if _DAMAGED is None:
        data = mixed(330, 10)
        z = deflate(data, 9)
        assert 250 <= len(z) <= 400 and zlib.decompress(z) == data
        bad = [z[:n] for n in range(len(z))]
        for i in range(8 * len(z)):
            s = bytearray(z)
            s[i >> 3] ^= 1 << (i & 7)
            bad.append(bytes(s))
        _DAMAGED = (z, data, bad)
    return _DAMAGED
