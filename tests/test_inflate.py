"""CPU: ffhip_inflate (ops.inflate) against zlib.decompress on every kind of block and distance, and everything it refuses as FFHIP_EINVAL."""
import zlib

import numpy as np
import pytest

from ffpic_amd import capi, ops


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(data) + co.flush()


def mixed(n, seed=1):
    """random bytes with repeats of earlier pieces: literals, matches of many lengths and distances"""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
    while len(out) < n:
        if rng.integers(0, 3):
            back, run = int(rng.integers(1, len(out) + 1)), int(rng.integers(3, 400))
            for _ in range(run):
                out.append(out[-back])
        else:
            out += rng.integers(0, 8, int(rng.integers(1, 200)), dtype=np.uint8).tobytes()
    return bytes(out[:n])


def refused(stream, cap=1 << 16):
    with pytest.raises(capi.FfhipError, match=str(capi.FFHIP_EINVAL)):
        ops.inflate(stream, cap)


def zwrap(deflate_bytes, payload):
    """a raw deflate stream in the zlib wrapper, with payload's Adler-32"""
    return b"\x78\x9c" + deflate_bytes + zlib.adler32(payload).to_bytes(4, "big")


class Bits:
    """deflate's bit order: fields from the least significant bit, Huffman codes from their most significant"""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def field(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, value, bits):
        return self.field(int(format(value, f"0{bits}b")[::-1], 2), bits)

    def fixed_literal(self, sym):
        if sym < 144:
            return self.code(0x30 + sym, 8)
        if sym < 256:
            return self.code(0x190 + sym - 144, 9)
        if sym < 280:
            return self.code(sym - 256, 7)
        return self.code(0xc0 + sym - 280, 8)

    def done(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


CASES = {
    "empty": (b"", {}),
    "stored_blocks": (mixed(200_000, 2), dict(level=0)),
    "fixed": (mixed(5000, 3), dict(strategy=zlib.Z_FIXED)),
    "huffman_only": (mixed(5000, 4), dict(strategy=zlib.Z_HUFFMAN_ONLY)),
    "rle": (mixed(5000, 5), dict(strategy=zlib.Z_RLE)),
    "level_1": (mixed(120_000, 6), dict(level=1)),
    "level_9": (mixed(120_000, 7), dict(level=9)),
    "equal_bytes": (b"\x5a" * 100_000, {}),
    "distance_32768": (np.random.default_rng(8).integers(0, 256, 32768, dtype=np.uint8).tobytes() * 2, dict(level=9)),
}
CASES.update({f"wbits_{w}": (mixed(70_000, 20 + w), dict(wbits=w)) for w in range(9, 16)})


@pytest.mark.parametrize("name", sorted(CASES))
def test_inflate_equals_zlib(name):
    data, how = CASES[name]
    z = deflate(data, **how)
    assert zlib.decompress(z) == data
    assert ops.inflate(z, len(data)) == data
    assert ops.inflate(z, len(data) + 100) == data
    if data:
        refused(z, len(data) - 1)                                    # cap one byte short


def test_every_proper_prefix_is_refused():
    data = mixed(330, 10)
    z = deflate(data, 9)                                              # a stream of about 300 bytes
    assert 250 <= len(z) <= 400 and ops.inflate(z, len(data)) == data
    for n in range(len(z)):
        refused(z[:n])


def test_bad_header_and_check_value():
    data = mixed(1000, 11)
    z = deflate(data)
    refused(z[:-1] + bytes([z[-1] ^ 1]))                              # Adler-32
    refused(bytes([z[0], z[1] | 0x20]) + z[2:])                       # preset dictionary (and the header check no longer holds)
    fdict = bytes([0x78, 0x20 | (31 - (0x7820 % 31))])                # a header with FDICT whose check bits are right
    assert (fdict[0] * 256 + fdict[1]) % 31 == 0
    refused(fdict + z[2:])
    refused(b"\x79" + z[1:])                                          # CM 9
    refused(b"\x88\x1c" + z[2:])                                      # a 64 KiB window


def test_block_type_3():
    refused(zwrap(Bits().field(1, 1).field(3, 2).done(), b""))


def test_distance_beyond_the_start():
    b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(257)      # 'A', then length 3
    b.code(1, 5)                                                                 # distance 2: one byte more than there is
    b.fixed_literal(256)
    refused(zwrap(b.done(), b"AAAA"))
    ok = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(257).code(0, 5).fixed_literal(256)
    assert ops.inflate(zwrap(ok.done(), b"AAAA"), 16) == b"AAAA"                 # the same with distance 1


def test_oversubscribed_code_lengths():
    # a dynamic block whose code-length code has three codes of one bit
    b = Bits().field(1, 1).field(2, 2).field(0, 5).field(0, 5).field(15, 4)
    for k in range(19):
        b.field(1 if k < 3 else 0, 3)
    refused(zwrap(b.done() + b"\x00" * 8, b""))


@pytest.mark.parametrize("sym", [286, 287])
def test_length_symbols_deflate_does_not_have(sym):
    b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(sym).code(0, 5).fixed_literal(256)
    refused(zwrap(b.done(), b"AAAA"))


@pytest.mark.parametrize("sym", [30, 31])
def test_distance_symbols_deflate_does_not_have(sym):
    b = Bits().field(1, 1).field(1, 2).fixed_literal(65).fixed_literal(257).code(sym, 5).fixed_literal(256)
    refused(zwrap(b.done(), b"AAAA"))


def test_one_code_distance_tree_is_taken_as_zlib_takes_it():
    """literal/length codes 'A' (1 bit), 256 and 257 (2 bits each); ONE distance code of one bit: incomplete, and zlib accepts it"""
    lengths = [0] * 258 + [1]
    lengths[65], lengths[256], lengths[257] = 1, 2, 2
    b = Bits().field(1, 1).field(2, 2).field(1, 5).field(0, 5).field(14, 4)          # 258 literal/length codes, 1 distance code, 18 code-length codes
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    clen = {0: 2, 1: 2, 2: 2, 18: 2}                                                 # code-length code: four codes of two bits, complete
    for k in range(18):
        b.field(clen.get(order[k], 0), 3)
    codes = {0: 0, 1: 1, 2: 2, 18: 3}                                                # canonical: symbols in order get 00, 01, 10, 11

    def put(sym, extra=None):
        b.code(codes[sym], 2)
        if extra is not None:
            b.field(extra, 7)

    put(18, 65 - 11)                                                                 # 65 zeros
    put(1)                                                                           # 'A': 1
    put(18, 138 - 11)
    put(18, 52 - 11)                                                                 # 66 .. 255: 190 zeros
    put(2)
    put(2)                                                                           # 256, 257: 2
    put(1)                                                                           # the distance code: 1
    b.code(0, 1).code(0b11, 2).code(0, 1).code(0b10, 2)                              # 'A', length 3 at distance 1, end of block
    stream = zwrap(b.done(), b"AAAA")
    assert zlib.decompress(stream) == b"AAAA"
    assert ops.inflate(stream, 16) == b"AAAA"
