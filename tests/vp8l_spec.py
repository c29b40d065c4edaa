"""The lossless WebP rule (include/ffpic_hip.h, "lossless WebP") a second time, in numpy and plain Python: written from the rule's lines,
not from the C.  parse(file) -> what the header and the transform list say; decode(file) -> BGRA [h][w][4]; Refused for everything the
rule refuses (animation: Animation).  Slow on purpose: one pixel at a time, no tables."""
import numpy as np

CODE_LENGTH_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
PREDICTOR, CROSS_COLOR, ADD_GREEN, COLOR_INDEXING = 0, 1, 2, 3

# the 120 short distance codes, in code order
DISTANCE_MAP = (
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1), (-3, 1),
    (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4),
    (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3),
    (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3),
    (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
    (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7),
    (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7))


class Refused(Exception):
    pass


class Animation(Refused):
    pass


class Bits:
    """LSB first.  Bits behind the end read as 0; a stream that was asked for one is refused once its image is done"""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        v = 0
        for k in range(n):
            byte = self.pos >> 3
            if byte < len(self.data):
                v |= ((self.data[byte] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v

    def check(self):
        if self.pos > 8 * len(self.data):
            raise Refused("the stream ends early")


class Code:
    """A canonical prefix code: shorter codes first, within a length by symbol; written MSB first"""

    def __init__(self, lengths):
        used = [(l, s) for s, l in enumerate(lengths) if l]
        if not used:
            raise Refused("a code without symbols")
        self.single = used[0][1] if len(used) == 1 else None
        if self.single is not None:
            return
        space = sum(1 << (15 - l) for l, _ in used)
        if space != 1 << 15:
            raise Refused("an over-subscribed or incomplete code")
        self.table, code, prev = {}, 0, 0
        for l, s in sorted(used):
            code <<= l - prev
            prev = l
            self.table[(l, code)] = s
            code += 1

    def symbol(self, bits):
        if self.single is not None:
            return self.single                                    # no bits read
        code = 0
        for l in range(1, 16):
            code = code << 1 | bits.read(1)
            if (l, code) in self.table:
                return self.table[(l, code)]
        raise Refused("no such code")


def read_code(bits, alphabet):
    lengths = [0] * max(alphabet, 256)
    if bits.read(1):                                              # the simple form: one or two symbols of length 1
        n = bits.read(1) + 1
        lengths[bits.read(8 if bits.read(1) else 1)] = 1
        if n == 2:
            lengths[bits.read(8)] = 1
    else:
        cl = [0] * 19
        for k in range(bits.read(4) + 4):
            cl[CODE_LENGTH_ORDER[k]] = bits.read(3)
        cl_code = Code(cl)
        limit = alphabet
        if bits.read(1):
            limit = 2 + bits.read(2 + 2 * bits.read(3))
            if limit > alphabet:
                raise Refused("max_symbol beyond the alphabet")
        s, prev = 0, 8
        while s < alphabet and limit > 0:
            limit -= 1
            c = cl_code.symbol(bits)
            if c < 16:
                lengths[s] = c
                s += 1
                prev = c or prev
                continue
            rep = bits.read((2, 3, 7)[c - 16]) + (3, 3, 11)[c - 16]
            if s + rep > alphabet:
                raise Refused("a repeat beyond the alphabet")
            lengths[s:s + rep] = [prev if c == 16 else 0] * rep
            s += rep
    return Code(lengths[:alphabet])                               # a simple code's symbol beyond the alphabet leaves the code empty


def prefix_value(bits, p):
    if p < 4:
        return p + 1
    extra = (p - 2) >> 1
    return ((2 + (p & 1)) << extra) + bits.read(extra) + 1


def sub(n, b):
    return (n + (1 << b) - 1) >> b


def read_image(bits, w, h, top):
    """one entropy-coded image of w x h ARGB words; top: the picture itself, which may have a meta prefix image"""
    cache_bits = 0
    if bits.read(1):
        cache_bits = bits.read(4)
        if not 1 <= cache_bits <= 11:
            raise Refused("colour cache bits")
    meta, meta_bits, groups = None, 0, 1
    if top and bits.read(1):
        meta_bits = bits.read(3) + 2
        meta = read_image(bits, sub(w, meta_bits), sub(h, meta_bits), False)[0]
        meta = [(v >> 8) & 0xffff for v in meta]
        groups = max(meta) + 1
    codes = []
    for _ in range(groups):
        codes.append([read_code(bits, a) for a in (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)])
    bits.check()
    cache = [0] * (1 << cache_bits) if cache_bits else None
    out, n = [], w * h

    def emit(v):
        out.append(v)
        if cache is not None:
            cache[((0x1e35a7bd * v) & 0xffffffff) >> (32 - cache_bits)] = v

    while len(out) < n:
        x, y = len(out) % w, len(out) // w
        g = codes[meta[(y >> meta_bits) * sub(w, meta_bits) + (x >> meta_bits)] if meta else 0]
        s = g[0].symbol(bits)
        if s < 256:
            r = g[1].symbol(bits)
            b = g[2].symbol(bits)
            a = g[3].symbol(bits)
            emit(a << 24 | r << 16 | s << 8 | b)
        elif s < 280:
            length = prefix_value(bits, s - 256)
            d = prefix_value(bits, g[4].symbol(bits))
            if d > 120:
                d -= 120
            else:
                dx, dy = DISTANCE_MAP[d - 1]
                d = max(dx + dy * w, 1)
            if d > len(out) or length > n - len(out):
                raise Refused("a copy from before the start or beyond the end")
            for _ in range(length):
                emit(out[-d])
        else:
            emit(cache[s - 280])                                  # s < 280 + cache size: the alphabet has no more
    bits.check()
    return out, {"cache_bits": cache_bits, "meta": meta is not None}


def container(file):
    """-> (VP8L payload, VP8X canvas or None).  Chunks are padded to even sizes; bytes behind the RIFF size are not looked at"""
    file = bytes(file)
    if len(file) < 12 or file[:4] != b"RIFF" or file[8:12] != b"WEBP":
        raise Refused("not RIFF/WEBP")
    riff = int.from_bytes(file[4:8], "little")
    if riff + 8 > len(file) or riff < 4:
        raise Refused("the RIFF size")
    end, pos, canvas = riff + 8, 12, None
    while pos + 8 <= end:
        tag, size = file[pos:pos + 4], int.from_bytes(file[pos + 4:pos + 8], "little")
        if size > end - pos - 8:
            raise Refused("a chunk beyond the file")
        body = file[pos + 8:pos + 8 + size]
        if tag == b"VP8X":
            if size != 10 or pos != 12:
                raise Refused("VP8X")
            if body[0] & 2:
                raise Animation()
            canvas = (1 + int.from_bytes(body[4:7], "little"), 1 + int.from_bytes(body[7:10], "little"))
        elif tag in (b"ANIM", b"ANMF"):
            raise Animation()
        elif tag == b"VP8 ":
            raise Refused("a lossy file")
        elif tag == b"VP8L":
            return body, canvas
        pos += 8 + size + (size & 1)
    raise Refused("no VP8L chunk")


def parse(file):
    """the header and the transforms, with their sub-images, and the residual image"""
    body, canvas = container(file)
    if len(body) < 5 or body[0] != 0x2f:
        raise Refused("the signature")
    bits = Bits(body[1:])
    w, h = bits.read(14) + 1, bits.read(14) + 1
    alpha = bits.read(1)
    if bits.read(3) != 0:
        raise Refused("the version")
    if canvas is not None and canvas != (w, h):
        raise Refused("the VP8X canvas disagrees")
    transforms, seen, xs = [], set(), w
    while bits.read(1):
        t = bits.read(2)
        if t in seen:
            raise Refused("a transform twice")
        seen.add(t)
        tr = {"type": t, "xsize": xs}
        if t in (PREDICTOR, CROSS_COLOR):
            tr["bits"] = bits.read(3) + 2
            tr["image"] = read_image(bits, sub(xs, tr["bits"]), sub(h, tr["bits"]), False)[0]
        elif t == COLOR_INDEXING:
            n = bits.read(8) + 1
            tr["bits"] = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            pal = read_image(bits, n, 1, False)[0]
            for k in range(1, n):                                 # each entry is stored as its difference to the one before, per byte
                pal[k] = sum((((pal[k] >> s) + (pal[k - 1] >> s)) & 255) << s for s in (0, 8, 16, 24))
            tr["palette"] = pal
            xs = sub(xs, tr["bits"])
        transforms.append(tr)
    residual, extra = read_image(bits, xs, h, True)
    return {"width": w, "height": h, "has_alpha": alpha, "transforms": transforms, "residual": residual, "residual_width": xs, **extra}


def ch(v):
    return [(v >> s) & 255 for s in (0, 8, 16, 24)]


def pack(c):
    return sum((c[k] & 255) << (8 * k) for k in range(4))


def avg2(a, b):
    return pack([(x + y) >> 1 for x, y in zip(ch(a), ch(b))])


def predict(mode, L, T, TR, TL):
    if mode == 0:
        return 0xff000000
    if mode < 5:
        return (L, T, TR, TL)[mode - 1]
    if mode == 5:
        return avg2(avg2(L, TR), T)
    if mode < 10:
        return avg2(*((L, TL), (L, T), (TL, T), (T, TR))[mode - 6])
    if mode == 10:
        return avg2(avg2(L, TL), avg2(T, TR))
    if mode == 11:
        dl = sum(abs(t - tl) for t, tl in zip(ch(T), ch(TL)))
        dt = sum(abs(l - tl) for l, tl in zip(ch(L), ch(TL)))
        return L if dl < dt else T
    if mode == 12:
        return pack([min(max(l + t - tl, 0), 255) for l, t, tl in zip(ch(L), ch(T), ch(TL))])
    if mode == 13:
        return pack([min(max(a + int((a - tl) / 2), 0), 255) for a, tl in zip(ch(avg2(L, T)), ch(TL))])
    return 0xff000000                                             # 14 and 15


def add(a, b):
    return pack([x + y for x, y in zip(ch(a), ch(b))])


def s8(v):
    return v - 256 if v > 127 else v


def invert(tr, px, h):
    """one transform undone: px is h rows of ARGB words; -> the rows at the width before the transform"""
    t, w = tr["type"], tr["xsize"]
    if t == ADD_GREEN:
        return [add(v, ((v >> 8) & 255) * 0x00010001) for v in px]
    if t == CROSS_COLOR:
        bx, out = sub(w, tr["bits"]), []
        for i, v in enumerate(px):
            m = tr["image"][((i // w) >> tr["bits"]) * bx + ((i % w) >> tr["bits"])]
            b, g, r, a = ch(v)
            r = (r + ((s8(m & 255) * s8(g)) >> 5)) & 255
            b = (b + ((s8((m >> 8) & 255) * s8(g)) >> 5) + ((s8((m >> 16) & 255) * s8(r)) >> 5)) & 255
            out.append(pack([b, g, r, a]))
        return out
    if t == COLOR_INDEXING:
        b, pal, out = tr["bits"], tr["palette"], []
        pw, per, depth = sub(w, b), 1 << b, 8 >> b
        for y in range(h):
            for x in range(w):
                idx = (((px[y * pw + (x >> b)] >> 8) & 255) >> (depth * (x & (per - 1)))) & ((1 << depth) - 1)
                out.append(pal[idx] if idx < len(pal) else 0)
        return out
    bx, out = sub(w, tr["bits"]), list(px)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            mode = (tr["image"][(y >> tr["bits"]) * bx + (x >> tr["bits"])] >> 8) & 15
            if y == 0:
                p = out[i - 1] if x else 0xff000000
            elif x == 0:
                p = out[i - w]
            else:
                p = predict(mode, out[i - 1], out[i - w], out[i - w + 1], out[i - w - 1])   # a row's last TR: the next word in memory
            out[i] = add(out[i], p)
    return out


def decode(file):
    p = parse(file)
    px = p["residual"]
    for tr in reversed(p["transforms"]):
        px = invert(tr, px, p["height"])
    a = np.array(px, dtype=np.uint32).reshape(p["height"], p["width"])
    if not p["has_alpha"]:
        a = a | np.uint32(0xff000000)
    return a.view(np.uint8).reshape(p["height"], p["width"], 4).copy()
