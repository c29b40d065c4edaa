"""The PNG witness: the pixel rule of include/ffpic_hip.h ("PNG") written once more, from the specification, with numpy and Python's zlib
and nothing of the library: parse, unfilter, expand, Adam7.  Slow and plain on purpose; the tests hold the library's host decoder and its
kernels against it byte for byte."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
VALID_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
# Adam7 written as the specification's 8 x 8 pattern: the pass of each pixel of a tile
PATTERN = np.array([[1, 6, 4, 6, 2, 6, 4, 6],
                    [7, 7, 7, 7, 7, 7, 7, 7],
                    [5, 6, 5, 6, 5, 6, 5, 6],
                    [7, 7, 7, 7, 7, 7, 7, 7],
                    [3, 6, 4, 6, 3, 6, 4, 6],
                    [7, 7, 7, 7, 7, 7, 7, 7],
                    [5, 6, 5, 6, 5, 6, 5, 6],
                    [7, 7, 7, 7, 7, 7, 7, 7]])


class Refused(ValueError):
    pass


def parse(data):
    """the chunks -> dict(width, height, depth, ctype, interlace, palette [n][3] or None, trns bytes or None (one that counts), idat bytes)"""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise Refused("signature")
    at, out, seen_idat, done = 8, dict(palette=None, trns=None, idat=b""), False, False
    first = True
    while at < len(data) and not done:
        if len(data) - at < 12:
            raise Refused("chunk cut")
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if n > len(data) - at - 12:
            raise Refused("chunk longer than the file")
        body = data[at + 8:at + 8 + n]
        crc_ok = zlib.crc32(kind + body) == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]
        if kind in (b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND") and not crc_ok:
            raise Refused(f"CRC of {kind}")
        if first != (kind == b"IHDR"):
            raise Refused("IHDR is the first chunk and only that")
        first = False
        if kind == b"IHDR":
            if n != 13:
                raise Refused("IHDR length")
            w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", body)
            if not (1 <= w <= 65535 and 1 <= h <= 65535) or depth not in VALID_DEPTHS.get(ctype, ()) or comp or filt or inter > 1:
                raise Refused("IHDR fields")
            out.update(width=w, height=h, depth=depth, ctype=ctype, interlace=inter)
        elif kind == b"PLTE" and not seen_idat:
            if n == 0 or n % 3 or n > 768 or out["palette"] is not None:
                raise Refused("PLTE")
            out["palette"] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"tRNS" and not seen_idat and out["trns"] is None:
            out["trns"] = body
        elif kind == b"IDAT":
            seen_idat = True
            out["idat"] += body
        elif kind == b"IEND":
            done = True
        elif not (kind[0] & 0x20) and kind not in (b"PLTE",):
            raise Refused(f"critical chunk {kind}")
        at += 12 + n
    if not done or not seen_idat:
        raise Refused("no IEND / no IDAT")
    ctype = out["ctype"]
    if ctype == 3 and out["palette"] is None:
        raise Refused("no PLTE")
    if ctype != 3:
        out["palette"] = None
    t = out["trns"]                                  # counts only with the colour type's length
    ok = t is not None and ((ctype == 3 and 1 <= len(t) <= len(out["palette"])) or (ctype == 0 and len(t) == 2) or (ctype == 2 and len(t) == 6))
    out["trns"] = t if ok else None
    return out


def sub_images(width, height, interlace):
    """[(pass 1..7 or 0, mask of the picture's pixels in it, columns, rows)] of the sub-images that have pixels"""
    if not interlace:
        return [(0, np.ones((height, width), bool), width, height)]
    tile = np.tile(PATTERN, ((height + 7) // 8, (width + 7) // 8))[:height, :width]
    out = []
    for p in range(1, 8):
        m = tile == p
        if m.any():
            out.append((p, m, int(m.any(axis=0).sum()), int(m.any(axis=1).sum())))
    return out


def layout(data):
    """dict of what ffhip_png_probe reports, from parse()"""
    f = parse(data)
    bits = CHANNELS[f["ctype"]] * f["depth"]
    rows, row_bytes = [0] * 7, [0] * 7
    for p, _, pw, ph in sub_images(f["width"], f["height"], f["interlace"]):
        rows[max(p - 1, 0)], row_bytes[max(p - 1, 0)] = ph, (pw * bits + 7) // 8
    return dict(width=f["width"], height=f["height"], bit_depth=f["depth"], color_type=f["ctype"], interlace=f["interlace"],
                has_trns=int(f["trns"] is not None), palette_size=0 if f["palette"] is None else len(f["palette"]),
                n_passes=sum(1 for r in rows if r), filtered_bytes=sum(r * (b + 1) for r, b in zip(rows, row_bytes)),
                pass_rows=rows, pass_row_bytes=row_bytes)


def unfilter(stream, n_rows, row_bytes, bpp):
    """n_rows x (1 + row_bytes) filtered bytes -> uint8 [n_rows][row_bytes]"""
    out = np.zeros((n_rows, row_bytes), np.uint8)
    prev = [0] * row_bytes
    for y in range(n_rows):
        line = stream[y * (row_bytes + 1):(y + 1) * (row_bytes + 1)]
        ft, cur = line[0], list(line[1:])
        if ft > 4:
            raise Refused("filter type")
        for i in range(row_bytes):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 1:
                cur[i] = (cur[i] + a) % 256
            elif ft == 2:
                cur[i] = (cur[i] + b) % 256
            elif ft == 3:
                cur[i] = (cur[i] + (a + b) // 2) % 256
            elif ft == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pr = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (cur[i] + pr) % 256
        out[y] = cur
        prev = cur
    return out


def samples_of(rows, width, channels, depth):
    """unfiltered rows -> the samples at the file's depth, int [n][width][channels]"""
    n = rows.shape[0]
    if depth == 8:
        return rows[:, :width * channels].astype(np.int64).reshape(n, width, channels)
    if depth == 16:
        pairs = rows[:, :2 * width * channels].astype(np.int64).reshape(n, width * channels, 2)
        return (pairs[..., 0] * 256 + pairs[..., 1]).reshape(n, width, channels)
    bits = np.unpackbits(rows, axis=1)[:, :width * depth].astype(np.int64).reshape(n, width, depth)
    return (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=-1).reshape(n, width, 1)


def to_bgra(s, f):
    """samples -> uint8 [n][w][4] by the rule"""
    ctype, depth, trns = f["ctype"], f["depth"], f["trns"]
    n, w, _ = s.shape
    out = np.full((n, w, 4), 255, np.int64)
    eight = (lambda v: v // 256) if depth == 16 else (lambda v: v * (255 // ((1 << depth) - 1)))
    if ctype == 3:
        pal = f["palette"]
        if s.max(initial=0) >= len(pal):
            raise Refused("index beyond PLTE")
        out[..., :3] = pal[s[..., 0]][..., ::-1]
        if trns is not None:
            alpha = np.full(len(pal), 255)
            alpha[:len(trns)] = list(trns)
            out[..., 3] = alpha[s[..., 0]]
    elif ctype in (0, 4):
        out[..., :3] = eight(s[..., :1])
        if ctype == 4:
            out[..., 3] = eight(s[..., 1])
        elif trns is not None:
            key = struct.unpack(">H", trns)[0] & ((1 << depth) - 1)
            out[..., 3] = np.where(s[..., 0] == key, 0, 255)
    else:
        out[..., :3] = eight(s[..., 2::-1] if s.shape[2] == 3 else s[..., [2, 1, 0]])
        if ctype == 6:
            out[..., 3] = eight(s[..., 3])
        elif trns is not None:
            key = np.array(struct.unpack(">HHH", trns)) & ((1 << depth) - 1)
            out[..., 3] = np.where((s[..., :3] == key).all(axis=-1), 0, 255)
    return out.astype(np.uint8)


def decode(data):
    """a PNG file's bytes -> BGRA uint8 [h][w][4]; Refused for what the rule refuses"""
    f = parse(data)
    w, h, depth, channels = f["width"], f["height"], f["depth"], CHANNELS[f["ctype"]]
    d = zlib.decompressobj()
    try:
        stream = d.decompress(f["idat"])
    except zlib.error as e:
        raise Refused(str(e))
    if not d.eof:
        raise Refused("the zlib stream does not end")
    bpp = max(1, channels * depth // 8)
    out = np.zeros((h, w, 4), np.uint8)
    at = 0
    for _, mask, pw, ph in sub_images(w, h, f["interlace"]):
        rb = (pw * channels * depth + 7) // 8
        need = ph * (rb + 1)
        if len(stream) - at < need:
            raise Refused("the stream ends short of the picture")
        rows = unfilter(stream[at:at + need], ph, rb, bpp)
        at += need
        out[mask] = to_bgra(samples_of(rows, pw, channels, depth), f).reshape(-1, 4)   # row-major in both: the pass's pixels in order
    return out
