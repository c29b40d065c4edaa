"""The alpha rule of lossy WebP files (include/ffpic_hip.h, "lossy WebP, the alpha plane") a second time, in plain Python and numpy: written
from the rule's lines, not from the C.  find(file) -> None for a file that stays opaque, else what the chunk walk and the ALPH header byte
say; plane(file) -> uint8 [h][w]; Refused for everything the rule refuses.  The headerless VP8L stream goes through vp8l_spec's Bits,
read_image and invert.  Slow on purpose."""
import numpy as np

import vp8l_spec as L
from vp8l_spec import Refused  # noqa: F401  (the witness's one exception type)


def find(file):
    """the libwebp rule's walk: chunks padded to even sizes, up to the `VP8 ` chunk; the first VP8X chunk's flags and the first ALPH chunk
    behind it are remembered"""
    file = bytes(file)
    if len(file) < 12 or file[:4] != b"RIFF" or file[8:12] != b"WEBP":
        raise Refused("not RIFF/WEBP")
    pos, flags, alph = 12, None, None
    while True:
        if pos + 4 > len(file):
            raise Refused("no VP8 chunk")
        tag = file[pos:pos + 4]
        if tag == b"VP8 ":
            break
        if tag in (b"VP8L", b"ANIM", b"ANMF"):
            raise Refused("not a still lossy file")
        if pos + 8 > len(file):
            raise Refused("a chunk header beyond the file")
        size = int.from_bytes(file[pos + 4:pos + 8], "little")
        if tag == b"VP8X":
            if size != 10 or pos + 18 > len(file):
                raise Refused("VP8X")
            if file[pos + 8] & 2:
                raise Refused("animation")
            if flags is None:
                flags = file[pos + 8]
        else:
            if size > len(file) - pos - 8:
                raise Refused("a chunk beyond the file")
            if tag == b"ALPH" and alph is None and flags is not None:
                alph = file[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    tagged = file[pos + 8:pos + 18]
    if len(tagged) < 10 or tagged[0] & 1 or tagged[3:6] != b"\x9d\x01\x2a":
        raise Refused("the frame tag")
    w, h = int.from_bytes(tagged[6:8], "little") & 0x3fff, int.from_bytes(tagged[8:10], "little") & 0x3fff
    if not w or not h:
        raise Refused("an empty frame")
    if alph is None or not flags & 0x10:
        return None
    if not alph:
        raise Refused("an empty ALPH payload")
    head = alph[0]
    out = {"compression": head & 3, "filter": (head >> 2) & 3, "pre": (head >> 4) & 3, "width": w, "height": h, "data": alph[1:]}
    if out["compression"] > 1 or out["pre"] > 1 or head >> 6:
        raise Refused("the ALPH header byte")
    if out["compression"] == 0 and len(out["data"]) < w * h:
        raise Refused("a short raw plane")
    return out


def lossless(data, w, h):
    """a headerless VP8L stream -> the green byte of its w x h pixels"""
    bits = L.Bits(data)
    transforms, seen, xs = [], set(), w
    while bits.read(1):
        t = bits.read(2)
        if t in seen:
            raise Refused("a transform twice")
        seen.add(t)
        tr = {"type": t, "xsize": xs}
        if t in (L.PREDICTOR, L.CROSS_COLOR):
            tr["bits"] = bits.read(3) + 2
            tr["image"] = L.read_image(bits, L.sub(xs, tr["bits"]), L.sub(h, tr["bits"]), False)[0]
        elif t == L.COLOR_INDEXING:
            n = bits.read(8) + 1
            tr["bits"] = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            pal = L.read_image(bits, n, 1, False)[0]
            for k in range(1, n):
                pal[k] = sum((((pal[k] >> s) + (pal[k - 1] >> s)) & 255) << s for s in (0, 8, 16, 24))
            tr["palette"] = pal
            xs = L.sub(xs, tr["bits"])
        transforms.append(tr)
    bits.check()
    px = residual(bits, xs, h, [t["type"] for t in transforms] == [L.COLOR_INDEXING])
    for tr in reversed(transforms):
        px = L.invert(tr, px, h)
    return (np.array(px, dtype=np.uint32).reshape(h, w) >> 8).astype(np.uint8)


class Tail:
    """libwebp's reader at the chunk's end: the last 8 bytes in a 64-bit window and a position in it, 64 at the end.  A fetch takes the
    window from (position mod 64) on, zeros above it.  Extra bits, or a refill at position >= 32, that find the position beyond 64 set
    it to 0 and mark the end; from then on extra bits are 0 and every refill sets the position to 0"""

    def __init__(self, data, at):
        self.win = int.from_bytes(data[-8:], "little")
        self.pos, self.eos = 64 - (8 * len(data) - at), False

    def fetch(self, n):
        return (self.win >> (self.pos & 63)) & ((1 << n) - 1)

    def fill(self):
        if self.pos >= 32 and (self.eos or self.pos > 64):
            self.eos, self.pos = True, 0

    def read(self, n):
        if self.eos:
            self.pos = 0
            return 0
        v = self.fetch(n)
        self.pos += n
        if self.pos > 64:
            self.eos, self.pos = True, 0
        return v

    def symbol(self, code):
        """a whole code word from ONE fetch (two where it is longer than 8 bits: the position moves on by 8 between them)"""
        if code.single is not None:
            return code.single
        for (l, c), s in code.table.items():
            word = int(format(c, f"0{l}b")[::-1], 2)              # MSB first in an LSB-first stream
            if l <= 8:
                if self.fetch(l) == word:
                    self.pos += l
                    return s
            elif self.fetch(8) == word & 255:
                self.pos += 8
                if self.fetch(l - 8) == word >> 8:
                    self.pos += l - 8
                    return s
                self.pos -= 8
        raise Refused("no such code")


def residual(bits, w, h, only_indexing):
    """the picture's own image, with the rule's one exception: where colour indexing is the only transform, the image has no colour cache
    and every group's red, blue and alpha codes have one symbol, the LAST token may run over the chunk's end; it is then what libwebp's
    reader makes of it (a stream of fewer than 8 bytes: zeros)"""
    try:
        return _read_image_marking(bits, w, h)
    except _Over as e:
        if not (only_indexing and e.lenient and e.at <= 8 * len(bits.data)):
            raise Refused("the stream ends early")
        over = e
    if len(bits.data) < 8:
        return over.image
    out, g, t = over.image[:over.done], over.group, Tail(bits.data, over.at)
    t.fill()
    s = t.symbol(g[0])
    if s < 256:
        out.append(g[3].single << 24 | g[1].single << 16 | s << 8 | g[2].single)
    else:
        def value(p):
            return p + 1 if p < 4 else ((2 + (p & 1)) << ((p - 2) >> 1)) + t.read((p - 2) >> 1) + 1
        length = value(s - 256)
        d = t.symbol(g[4])
        t.fill()
        d = value(d)
        if d > 120:
            d -= 120
        else:
            dx, dy = L.DISTANCE_MAP[d - 1]
            d = max(dx + dy * w, 1)
        if d > len(out):
            raise Refused("a copy from before the start")
        for _ in range(length):
            out.append(out[-d])
    if len(out) != w * h:
        raise Refused("the end is marked and the image is not whole")
    return out


class _Over(Exception):
    def __init__(self, image, lenient, at, done, group):
        self.image, self.lenient, self.at, self.done, self.group = image, lenient, at, done, group


def _read_image_marking(bits, w, h):
    """the picture's own image as vp8l_spec.read_image reads it, token by token, remembering where the last token began"""
    cache_bits = 0
    if bits.read(1):
        cache_bits = bits.read(4)
        if not 1 <= cache_bits <= 11:
            raise Refused("colour cache bits")
    meta, meta_bits, groups = None, 0, 1
    if bits.read(1):
        meta_bits = bits.read(3) + 2
        meta = [(v >> 8) & 0xffff for v in L.read_image(bits, L.sub(w, meta_bits), L.sub(h, meta_bits), False)[0]]
        groups = max(meta) + 1
    codes = [[L.read_code(bits, a) for a in (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)] for _ in range(groups)]
    bits.check()
    lenient = not cache_bits and all(g[k].single is not None for g in codes for k in (1, 2, 3))
    cache = [0] * (1 << cache_bits) if cache_bits else None
    out, n, at, done, g = [], w * h, bits.pos, 0, codes[0]

    def emit(v):
        out.append(v)
        if cache is not None:
            cache[((0x1e35a7bd * v) & 0xffffffff) >> (32 - cache_bits)] = v

    while len(out) < n:
        if bits.pos > 8 * len(bits.data):
            raise Refused("the stream ends early")                # over the end with pixels still to come
        x, y = len(out) % w, len(out) // w
        g = codes[meta[(y >> meta_bits) * L.sub(w, meta_bits) + (x >> meta_bits)] if meta else 0]
        at, done = bits.pos, len(out)
        s = g[0].symbol(bits)
        if s < 256:
            r, b, a = g[1].symbol(bits), g[2].symbol(bits), g[3].symbol(bits)
            emit(a << 24 | r << 16 | s << 8 | b)
        elif s < 280:
            length = L.prefix_value(bits, s - 256)
            d = L.prefix_value(bits, g[4].symbol(bits))
            if d > 120:
                d -= 120
            else:
                dx, dy = L.DISTANCE_MAP[d - 1]
                d = max(dx + dy * w, 1)
            if d > len(out) or length > n - len(out):
                raise Refused("a copy from before the start or beyond the end")
            for _ in range(length):
                emit(out[-d])
        else:
            emit(cache[s - 280])
    if bits.pos > 8 * len(bits.data):
        raise _Over(out, lenient, at, done, g)
    return out


def unfilter(stored, f):
    """the table of the rule: sums modulo 256 on the finished plane"""
    h, w = stored.shape
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            if f == 0:
                p = 0
            elif y == 0 or f == 1:
                p = out[y, x - 1] if x > 0 else (out[y - 1, 0] if y > 0 else 0)
            elif f == 2:
                p = out[y - 1, x]
            else:
                p = out[y - 1, 0] if x == 0 else min(255, max(0, out[y, x - 1] + out[y - 1, x] - out[y - 1, x - 1]))
            out[y, x] = (int(stored[y, x]) + p) & 255
    return out.astype(np.uint8)


def plane(file):
    a = find(file)
    if a is None:
        raise Refused("no alpha plane")
    w, h = a["width"], a["height"]
    if a["compression"] == 0:
        stored = np.frombuffer(a["data"][:w * h], np.uint8).reshape(h, w)
    else:
        stored = lossless(a["data"], w, h)
    return unfilter(stored, a["filter"])
