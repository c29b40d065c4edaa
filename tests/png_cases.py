"""The shared list of PNG test files (png_writer.py writes them from known samples).  Small pictures: the kernels go wrong at edges -- the
last row of a band of 64 and the first of the next, a row's last partial chunk, a picture's last partial group of four pixels, a pass
without pixels -- and not in the middle.  A list, no cross product: build() gives the same files in the same order every time."""
import zlib
from collections import namedtuple

import numpy as np

import png_writer as W

Case = namedtuple("Case", "name data samples ctype depth interlace palette trns")

# every filter type follows every filter type (itself included) once per turn of 25 rows: an Euler tour of the five types' pairs
TOUR = [0, 0, 1, 0, 2, 0, 3, 0, 4, 1, 1, 2, 1, 3, 1, 4, 2, 2, 3, 2, 4, 3, 3, 4, 4]
EDGE_ROWS = (0, 63, 64, 128)
# how the zlib stream is made and cut, taken in turn
STREAMS = [dict(), dict(level=9, idat_sizes=[0, 1, 1, 7, 0, 100]), dict(level=0), dict(strategy=zlib.Z_FIXED, idat_sizes=[1]),
           dict(level=1, idat_sizes=[4096]), dict(strategy=zlib.Z_RLE, wbits=9), dict(strategy=zlib.Z_HUFFMAN_ONLY, idat_sizes=[33, 0])]


def tour_from(start):
    return TOUR[start:] + TOUR[:start]


def big_rotations():
    """per (colour type, depth) pair where in TOUR its rows start, so that over the 15 files each of the five types occurs on each of EDGE_ROWS"""
    for step in range(1, 25):
        rot = [(k * step) % 25 for k in range(len(W.PAIRS))]
        if all({TOUR[(r + row) % 25] for r in rot} == {0, 1, 2, 3, 4} for row in EDGE_ROWS):
            return rot
    raise AssertionError("no rotation of the tour covers the edge rows")


def random_samples(rng, h, w, ctype, depth, limit=None):
    top = (1 << depth) if limit is None else limit
    return rng.integers(0, top, (h, w, W.CHANNELS[ctype]), dtype=np.int64)


def random_palette(rng, n):
    return rng.integers(0, 256, (n, 3), dtype=np.int64).astype(np.uint8)


def build():
    rng = np.random.default_rng(20251)
    cases = []

    def add(name, h, w, ctype, depth, filters, interlace=False, palette=None, trns=None, samples=None, **more):
        if ctype == 3 and palette is None:
            palette = random_palette(rng, 1 << depth)
        if samples is None:
            samples = random_samples(rng, h, w, ctype, depth, None if palette is None else len(palette))
        how = dict(STREAMS[len(cases) % len(STREAMS)])
        how.update(more)
        data = W.write(samples, ctype, depth, filters=filters, interlace=interlace, palette=palette, trns=trns, **how)
        cases.append(Case(name, data, samples, ctype, depth, interlace, palette, trns))

    def any_filters(n=256):
        return [int(v) for v in rng.integers(0, 5, n)]

    # every pair at 65 x 130: three bands, a last chunk and a last group that are partial; random bytes give Paeth ties and wrap-around
    for (ctype, depth), rot in zip(W.PAIRS, big_rotations()):
        add(f"c{ctype}d{depth}_65x130", 130, 65, ctype, depth, tour_from(rot))
    # widths at height 3, heights at width 5: RGB 8 (bpp 3) and grey 1 (sub-byte rows, bpp 1)
    for w, kind in ((1, "g"), (2, "c"), (3, "g"), (7, "g"), (8, "g"), (9, "g"), (63, "c"), (64, "g"), (65, "c"), (130, "g"), (4, "c"), (5, "c")):
        add(f"{kind}_w{w}", 3, w, *((2, 8) if kind == "c" else (0, 1)), any_filters())
    for h, kind in ((1, "c"), (2, "g"), (63, "c"), (64, "g"), (65, "c"), (129, "g"), (200, "c")):
        add(f"{kind}_h{h}", h, 5, *((2, 8) if kind == "c" else (0, 1)), any_filters())
    # Adam7: small sizes with passes that have no pixels, then three kinds over several bands
    for w, h in ((1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (8, 8), (9, 9)):
        add(f"adam7_{w}x{h}", h, w, 6, 8, any_filters(), interlace=True)
    add("adam7_pal2_65x130", 130, 65, 3, 2, any_filters(), interlace=True)
    add("adam7_rgb8_65x130", 130, 65, 2, 8, any_filters(), interlace=True)
    add("adam7_rgba16_65x130", 130, 65, 6, 16, any_filters(), interlace=True)
    # tRNS on grey and RGB: the key is a sample the picture has (and, at 16 bits, samples that share its high byte only)
    s = random_samples(rng, 9, 33, 0, 2)
    add("trns_grey2", 9, 33, 0, 2, any_filters(), trns=b"\x00\x02", samples=s)
    s = random_samples(rng, 9, 33, 0, 16)
    s[::2, ::3, 0] = 0x1234
    s[1::2, ::3, 0] = 0x1235
    add("trns_grey16", 9, 33, 0, 16, any_filters(), trns=b"\x12\x34", samples=s)
    s = random_samples(rng, 9, 33, 2, 8)
    s[::2, ::3] = (10, 20, 30)
    s[1::2, ::3] = (10, 20, 31)
    add("trns_rgb8", 9, 33, 2, 8, any_filters(), trns=b"\x00\x0a\x00\x14\x00\x1e", samples=s)
    s = random_samples(rng, 9, 33, 2, 16)
    s[::2, ::3] = (0x0102, 0x0304, 0x0506)
    s[1::2, ::3] = (0x0102, 0x0304, 0x0507)
    add("trns_rgb16", 9, 33, 2, 16, any_filters(), trns=b"\x01\x02\x03\x04\x05\x06", samples=s)
    # a palette shorter than its indices' range, used legally; a tRNS shorter than the palette
    add("pal4_short", 9, 33, 3, 4, any_filters(), palette=random_palette(rng, 5))
    add("pal8_trns_short", 9, 33, 3, 8, any_filters(), palette=random_palette(rng, 200), trns=bytes(int(v) for v in rng.integers(0, 256, 50)))
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build()
    return _CASES


_EXPECTED = None


def expected():
    """the witness's BGRA of every case, computed once and shared: [uint8 [h][w][4]], read-only"""
    global _EXPECTED
    if _EXPECTED is None:
        import png_spec
        _EXPECTED = [png_spec.decode(c.data) for c in cases()]
        for e in _EXPECTED:
            e.setflags(write=False)
    return _EXPECTED


def damaged():
    """[(name, bytes)]: files the rule refuses, one per refusal, made from good ones"""
    import struct
    rng = np.random.default_rng(7)
    s = random_samples(rng, 6, 7, 2, 8)
    pal = random_palette(rng, 5)
    good = W.write(s, 2, 8, filters=[0, 1, 2, 3, 4])
    palfile = W.write(random_samples(rng, 6, 7, 3, 4, 5), 3, 4, palette=pal, trns=b"\x01\x02", filters=4)
    out = []

    def flip(data, kind, name):
        at = data.index(kind)
        body = struct.unpack(">I", data[at - 4:at])[0]
        crc_at = at + 4 + body
        out.append((name, data[:crc_at] + bytes([data[crc_at] ^ 1]) + data[crc_at + 1:]))

    flip(good, b"IHDR", "crc_ihdr")
    flip(palfile, b"PLTE", "crc_plte")
    flip(palfile, b"tRNS", "crc_trns")
    flip(good, b"IDAT", "crc_idat")
    flip(good, b"IEND", "crc_iend")
    raw = W.filtered_stream(s, 2, 8, [0, 1, 2, 3, 4])
    z = zlib.compress(raw)
    head = W.SIGNATURE + W.chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 6, 8, 2, 0, 0, 0))
    out.append(("bad_adler", head + W.chunk(b"IDAT", z[:-1] + bytes([z[-1] ^ 1])) + W.chunk(b"IEND")))
    out.append(("short_stream", head + W.chunk(b"IDAT", zlib.compress(raw[:-1])) + W.chunk(b"IEND")))
    out.append(("truncated_idat", head + W.chunk(b"IDAT", z[:len(z) // 2]) + W.chunk(b"IEND")))
    out.append(("filter_byte_5", W.write(s, 2, 8, stream=raw[:22] + b"\x05" + raw[23:])))
    for name, fields in (("depth_4_rgb", (7, 6, 4, 2, 0, 0, 0)), ("depth_16_palette", (7, 6, 16, 3, 0, 0, 0)), ("colour_type_5", (7, 6, 8, 5, 0, 0, 0)),
                         ("compression_1", (7, 6, 8, 2, 1, 0, 0)), ("filter_method_1", (7, 6, 8, 2, 0, 1, 0)), ("interlace_2", (7, 6, 8, 2, 0, 0, 2)),
                         ("width_0", (0, 6, 8, 2, 0, 0, 0)), ("height_0", (7, 0, 8, 2, 0, 0, 0)), ("width_65536", (65536, 6, 8, 2, 0, 0, 0))):
        out.append((name, W.SIGNATURE + W.chunk(b"IHDR", struct.pack(">IIBBBBB", *fields)) + W.chunk(b"IDAT", z) + W.chunk(b"IEND")))
    out.append(("no_iend", good[:-12]))
    bad_index = random_samples(rng, 6, 7, 3, 4, 5)
    bad_index[5, 6, 0] = 5
    out.append(("index_beyond_plte", W.write(bad_index, 3, 4, palette=pal, filters=[1, 4, 3])))
    return out
