"""A lossless WebP (VP8L) writer for tests: files from KNOWN ARGB pixels, everything chosen by the caller -- the transform list in any order
with its block bits, mode and multiplier images, palette and bundling; the colour cache and which pixels go as cache hits; a meta prefix
image with several code groups; backward references as explicit (length, distance code) tokens; the code lengths of every alphabet and
how they are written (plain, with max_symbol, with the repeat symbols 16 / 17 / 18, or the simple one- and two-symbol forms); the alpha
bit; a VP8X / EXIF wrapper.  expected_bgra() is the known picture.  The answer key: it shares no code with tests/vp8l_spec.py.

Pixels are ARGB words (numpy uint32 [h][w]): alpha << 24 | red << 16 | green << 8 | blue."""
import struct

import numpy as np

PREDICTOR, CROSS_COLOR, ADD_GREEN, COLOR_INDEXING = 0, 1, 2, 3
ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):                                      # LSB first
        assert 0 <= value < (1 << n) or n == 0
        self.bits.extend((value >> k) & 1 for k in range(n))

    def code(self, code, n):                                      # a prefix code's word: MSB first
        self.bits.extend((code >> (n - 1 - k)) & 1 for k in range(n))

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def complete_lengths(n):
    """a complete code over n >= 2 symbols: 232 x 8 and 48 x 9 bits for 280"""
    k = n.bit_length() - 1
    m = n - (1 << k)
    return [k] * ((1 << k) - m) + [k + 1] * (2 * m)


def canonical(lengths):
    """symbol -> (word, bits); a code of one symbol has the empty word"""
    used = sorted((l, s) for s, l in enumerate(lengths) if l)
    if len(used) == 1:
        return {used[0][1]: (0, 0)}
    words, code, prev = {}, 0, 0
    for l, s in used:
        code <<= l - prev
        prev = l
        words[s] = (code, l)
        code += 1
    return words


def rle(lengths):
    """the code lengths as tokens of the code-length alphabet: (symbol, extra value)"""
    out, i, prev = [], 0, 8
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((17, take - 3) if take <= 10 else (18, take - 11))
            i += take
        elif v == prev and run >= 3:
            take = min(run, 6)
            out.append((16, take - 3))
            i += take
        else:
            out.append((v, None))
            prev = v or prev
            i += 1
    return out


def put_code(bw, spec, alphabet):
    """spec: a dict -- lengths (default: a complete code over the alphabet); simple=(s0,) or (s0, s1); max_symbol=True; repeats=True;
    raw_max_symbol: the value written whatever the tokens are.  Returns symbol -> (word, bits)."""
    spec = spec or {}
    if "simple" in spec:
        syms = spec["simple"]
        bw.put(1, 1)
        bw.put(len(syms) - 1, 1)
        wide = syms[0] > 1 or spec.get("wide", False)
        bw.put(int(wide), 1)
        bw.put(syms[0], 8 if wide else 1)
        if len(syms) == 2:
            bw.put(syms[1], 8)
        return canonical([1 if s in syms else 0 for s in range(max(alphabet, 256))])
    lengths = list(spec.get("lengths") or complete_lengths(alphabet))
    lengths += [0] * (alphabet - len(lengths))
    bw.put(0, 1)
    tokens = rle(lengths) if spec.get("repeats") else [(v, None) for v in lengths]
    if spec.get("max_symbol"):
        while tokens and tokens[-1][0] in (0, 17, 18):            # the zeros at the end need not be written
            tokens.pop()
    cl = spec.get("cl_lengths") or [4] * 13 + [5] * 6             # complete over the 19 symbols
    bw.put(19 - 4, 4)
    for k in ORDER:
        bw.put(cl[k], 3)
    words = canonical(cl)
    if spec.get("max_symbol") or "raw_max_symbol" in spec:
        count = spec.get("raw_max_symbol", len(tokens))
        nbits = max(2, (max(count - 2, 0)).bit_length() + ((max(count - 2, 0)).bit_length() & 1))
        bw.put(1, 1)
        bw.put((nbits - 2) // 2, 3)
        bw.put(count - 2, nbits)
    else:
        bw.put(0, 1)
    for sym, extra in tokens:
        bw.code(*words[sym])
        if extra is not None:
            bw.put(extra, (2, 3, 7)[sym - 16])
    return canonical(lengths)


def prefix_of(value):
    """a length or distance code -> (prefix symbol, extra bits, extra value)"""
    d = value - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    extra = hb - 1
    return 2 * hb + ((d >> extra) & 1), extra, d & ((1 << extra) - 1)


def cache_key(argb, bits):
    return ((0x1e35a7bd * int(argb)) & 0xffffffff) >> (32 - bits)


def sub(n, b):
    return (n + (1 << b) - 1) >> b


def put_image(bw, tokens, w, h, top, cache_bits=0, meta=None, codes=None):
    """tokens: ("lit", argb) | ("copy", length, distance code) | ("hit", argb) | ("auto", argb), covering w x h words.
    meta: (bits, group index per block [rows][cols]); codes: {(group, alphabet 0..4): spec of put_code}"""
    bw.put(int(cache_bits > 0), 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    groups, gmap, mbits = 1, None, 0
    if top:
        bw.put(int(meta is not None), 1)
        if meta is not None:
            mbits, gmap = meta[0], np.asarray(meta[1])
            assert gmap.shape == (sub(h, mbits), sub(w, mbits))
            bw.put(mbits - 2, 3)
            put_image(bw, [("lit", int(g) << 8) for g in gmap.reshape(-1)], gmap.shape[1], gmap.shape[0], False)
            groups = int(gmap.max()) + 1
    sizes = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    words = [[put_code(bw, (codes or {}).get((g, a)), sizes[a]) for a in range(5)] for g in range(groups)]
    cache, done = {}, []

    def emit(v):
        done.append(v)
        if cache_bits:
            cache[cache_key(v, cache_bits)] = v

    for tok in tokens:
        y, x = divmod(len(done), w)
        g = words[int(gmap[y >> mbits, x >> mbits]) if gmap is not None else 0]
        if tok[0] == "auto":                                      # a hit where the cache holds the word, else a literal
            tok = ("hit" if cache_bits and cache.get(cache_key(tok[1], cache_bits)) == int(tok[1]) else "lit", tok[1])
        if tok[0] == "lit":
            v = int(tok[1])
            for a, s in ((0, (v >> 8) & 255), (1, (v >> 16) & 255), (2, v & 255), (3, v >> 24)):
                bw.code(*g[a][s])
            emit(v)
        elif tok[0] == "hit":
            key = cache_key(tok[1], cache_bits)
            assert cache.get(key) == int(tok[1]), "the cache does not hold that pixel here"
            bw.code(*g[0][280 + key])
            emit(int(tok[1]))
        else:
            _, length, dcode = tok
            sym, nb, val = prefix_of(length)
            bw.code(*g[0][256 + sym])
            bw.put(val, nb)
            sym, nb, val = prefix_of(dcode)
            bw.code(*g[4][sym])
            bw.put(val, nb)
            d = distance_of(dcode, w)
            for _ in range(length):
                emit(done[-d] if d <= len(done) else 0)           # damaged files may point before the start
    return done


# libwebp's order of the 120 short codes
SHORT = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1),
         (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2),
         (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5),
         (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4),
         (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7),
         (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1),
         (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]


def distance_of(dcode, w):
    if dcode > 120:
        return dcode - 120
    dx, dy = SHORT[dcode - 1]
    return max(dx + dy * w, 1)


def run_tokens(tokens, w):
    """the words a token list stands for; ("lit", None) and ("hit", None) are not allowed here"""
    out = []
    for tok in tokens:
        if tok[0] == "copy":
            d = distance_of(tok[2], w)
            for _ in range(tok[1]):
                out.append(out[-d])
        else:
            out.append(int(tok[1]))
    return out


def literal_tokens(words, cache_bits=0, hits=True):
    """every word a literal; with a cache and hits, a word the cache holds goes as a hit"""
    cache, out = {}, []
    for v in (int(v) for v in words):
        key = cache_key(v, cache_bits) if cache_bits else None
        out.append(("hit", v) if cache_bits and hits and cache.get(key) == v else ("lit", v))
        if cache_bits:
            cache[key] = v
    return out


def _ch(v):
    return [(v >> s) & 255 for s in (0, 8, 16, 24)]


def _pack(c):
    return sum((int(c[k]) & 255) << (8 * k) for k in range(4))


def _half(a, b):
    return [(x + y) // 2 for x, y in zip(a, b)]


def _predict(mode, L, T, TR, TL):
    """the format text's 14 predictors on channel lists; 14 and 15 are black"""
    if mode in (0, 14, 15):
        return [0, 0, 0, 255]
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _half(_half(L, TR), T)
    if mode == 6:
        return _half(L, TL)
    if mode == 7:
        return _half(L, T)
    if mode == 8:
        return _half(TL, T)
    if mode == 9:
        return _half(T, TR)
    if mode == 10:
        return _half(_half(L, TL), _half(T, TR))
    if mode == 11:
        est = [l + t - tl for l, t, tl in zip(L, T, TL)]
        dl = sum(abs(e - l) for e, l in zip(est, L))
        dt = sum(abs(e - t) for e, t in zip(est, T))
        return L if dl < dt else T
    if mode == 12:
        return [min(max(l + t - tl, 0), 255) for l, t, tl in zip(L, T, TL)]
    avg = _half(L, T)
    return [min(max(a + (abs(a - tl) // 2) * (1 if a >= tl else -1), 0), 255) for a, tl in zip(avg, TL)]


def _s8(v):
    return v - 256 if v > 127 else v


def forward(words, w, h, tr):
    """one transform applied: words (h rows of tr's width) -> what the decoder has to be given for them"""
    t = tr["type"]
    words = [int(v) for v in words]
    if t == ADD_GREEN:
        return [_pack([c[0] - c[1], c[1], c[2] - c[1], c[3]]) for c in map(_ch, words)]
    if t == CROSS_COLOR:
        b, img = tr["bits"], np.asarray(tr["image"])
        out = []
        for i, v in enumerate(words):
            m = int(img[(i // w) >> b, (i % w) >> b])
            bl, g, r, a = _ch(v)
            nb = bl - ((_s8((m >> 8) & 255) * _s8(g)) >> 5) - ((_s8((m >> 16) & 255) * _s8(r)) >> 5)
            nr = r - ((_s8(m & 255) * _s8(g)) >> 5)
            out.append(_pack([nb, g, nr, a]))
        return out
    if t == COLOR_INDEXING:
        pal = [int(p) for p in tr["palette"]]
        bits = tr["bits"]
        per, depth, out = 1 << bits, 8 >> bits, []
        index = tr.get("indices")                                 # given: the indices themselves (some may lie beyond the palette)
        for y in range(h):
            for x0 in range(0, w, per):
                g = 0
                for k in range(min(per, w - x0)):
                    idx = int(index[y][x0 + k]) if index is not None else pal.index(words[y * w + x0 + k])
                    g |= idx << (depth * k)
                out.append(0xff000000 | g << 8)
        return out
    b, img = tr["bits"], np.asarray(tr["image"])
    px = [_ch(v) for v in words]
    out = []
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                p = px[i - 1] if x else [0, 0, 0, 255]
            elif x == 0:
                p = px[i - w]
            else:
                p = _predict((int(img[y >> b, x >> b]) >> 8) & 15, px[i - 1], px[i - w], px[i - w + 1], px[i - w - 1])
            out.append(_pack([c - q for c, q in zip(px[i], p)]))
    return out


def bundle_bits(n):
    return 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3


def write(argb, transforms=(), alpha=True, cache_bits=0, hits=True, tokens=None, meta=None, codes=None, vp8x=None, exif=None,
          version=0, signature=0x2f, trailing=b"", header_size=None, repeat=None):
    """argb: uint32 [h][w].  transforms, in the file's order: dicts with type and
         PREDICTOR / CROSS_COLOR: bits, image (uint32 [rows][cols] at block resolution: the mode in the green byte / the multipliers)
         COLOR_INDEXING: palette (ARGB words; bundling follows from its length), optionally indices [h][w] in place of a look-up
    tokens: the residual image's token list (default: literals, cache hits where the cache holds the word);
    vp8x: None, or a dict -- alpha (the flag), canvas (w, h) -- for a VP8X chunk in front; exif: the EXIF chunk's payload;
    header_size: (w, h) written into the VP8L header whatever argb's shape is; repeat: a transform dict written once more at the end"""
    argb = np.asarray(argb, dtype=np.uint32)
    h, w = argb.shape
    bw = BitWriter()
    hw, hh = header_size or (w, h)
    bw.put(hw - 1, 14)
    bw.put(hh - 1, 14)
    bw.put(int(bool(alpha)), 1)
    bw.put(version, 3)
    words, xs = [int(v) for v in argb.reshape(-1)], w
    for tr in list(transforms) + ([repeat] if repeat else []):
        t = tr["type"]
        bw.put(1, 1)
        bw.put(t, 2)
        if t == COLOR_INDEXING:
            tr["bits"] = bundle_bits(len(tr["palette"]))
        if tr is not repeat:
            words = forward(words, xs, h, tr)
        if t in (PREDICTOR, CROSS_COLOR):
            img = np.asarray(tr["image"], dtype=np.uint32)
            assert img.shape == (sub(h, tr["bits"]), sub(xs, tr["bits"])), (img.shape, h, xs, tr["bits"])
            bw.put(tr["bits"] - 2, 3)
            put_image(bw, literal_tokens(img.reshape(-1)), img.shape[1], img.shape[0], False)
        elif t == COLOR_INDEXING:
            pal = [int(p) for p in tr["palette"]]
            bw.put(len(pal) - 1, 8)
            diff = [pal[0]] + [_pack([a - b for a, b in zip(_ch(pal[k]), _ch(pal[k - 1]))]) for k in range(1, len(pal))]
            put_image(bw, literal_tokens(diff), len(pal), 1, False)
            if tr is not repeat:
                xs = sub(xs, tr["bits"])
    bw.put(0, 1)
    if tokens is None:
        tokens = literal_tokens(words, cache_bits, hits)
    put_image(bw, tokens, xs, h, True, cache_bits, meta, codes)
    payload = bytes([signature]) + bw.bytes() + trailing
    return riff(payload, vp8x, exif, (w, h))


def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)


def riff(payload, vp8x=None, exif=None, size=(1, 1)):
    body = b"WEBP"
    if vp8x is not None:
        cw, chh = vp8x.get("canvas", size)
        flags = (0x10 if vp8x.get("alpha") else 0) | (0x08 if exif is not None else 0) | (0x02 if vp8x.get("animation") else 0)
        body += chunk(b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", cw - 1)[:3] + struct.pack("<I", chh - 1)[:3])
    body += chunk(b"VP8L", payload)
    if exif is not None:
        body += chunk(b"EXIF", exif)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def expected_bgra(argb, alpha=True):
    """the picture a decoder has to deliver: BGRA bytes [h][w][4]; without the alpha bit every alpha sample is 255"""
    a = np.asarray(argb, dtype=np.uint32)
    if not alpha:
        a = a | np.uint32(0xff000000)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], 4).copy()
