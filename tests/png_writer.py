"""An answer-key PNG writer: from KNOWN samples it writes any of the 15 (colour type, bit depth) pairs with a chosen filter type per row,
Adam7 or not, PLTE / tRNS / eXIf, the IDAT data cut into chunks of chosen sizes (0 and 1 bytes included) and a chosen zlib level, strategy
and window, through Python's zlib.  What a decoder has to give for such a file is known without any decoder: expected_bgra()."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
PAIRS = [(c, d) for c in (0, 2, 3, 4, 6) for d in DEPTHS[c]]                 # the 15 valid pairs
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]   # x start, y start, x step, y step
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data=b"", crc=None):
    """one chunk; crc: a value to write instead of the right one"""
    crc = zlib.crc32(kind + data) if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc & 0xffffffff)


def bpp_of(ctype, depth):
    return max(1, CHANNELS[ctype] * depth // 8)


def pack_rows(samples, depth):
    """samples [h][w][channels] at the file's depth -> the rows' bytes, uint8 [h][row bytes]"""
    h, w, c = samples.shape
    s = samples.astype(np.uint32)
    if depth == 8:
        return s.astype(np.uint8).reshape(h, w * c)
    if depth == 16:
        return np.stack([s >> 8, s & 255], axis=-1).astype(np.uint8).reshape(h, 2 * w * c)
    bits = ((s.reshape(h, w * c, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, w * c * depth)
    return np.packbits(bits, axis=1)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, types):
    """rows uint8 [n][row bytes] of one sub-image, types[n] -> the filtered stream of it: per row the type byte and the filtered bytes"""
    n, rb = rows.shape
    r = rows.astype(np.int32)
    out = bytearray()
    for y in range(n):
        cur = r[y]
        up = r[y - 1] if y else np.zeros(rb, np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur])[:rb]
        c = np.concatenate([np.zeros(bpp, np.int32), up])[:rb]
        t = types[y]
        pred = {0: np.zeros(rb, np.int32), 1: a, 2: up, 3: (a + up) >> 1, 4: _paeth(a, up, c)}.get(t, np.zeros(rb, np.int32))
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def passes(width, height, interlace):
    """[(x start, y start, x step, y step, columns, rows)] of the sub-images that have pixels"""
    if not interlace:
        return [(0, 0, 1, 1, width, height)]
    out = []
    for xs, ys, dx, dy in ADAM7:
        pw, ph = (width - xs + dx - 1) // dx if width > xs else 0, (height - ys + dy - 1) // dy if height > ys else 0
        if pw and ph:
            out.append((xs, ys, dx, dy, pw, ph))
    return out


def filtered_stream(samples, ctype, depth, filters=0, interlace=False):
    """the bytes the zlib stream holds.  filters: one type, a sequence indexed by the row's number in the STREAM (all passes counted on,
    taken modulo its length), or a callable (pass, row) -> type"""
    h, w, _ = samples.shape
    out, k = b"", 0
    for p, (xs, ys, dx, dy, pw, ph) in enumerate(passes(w, h, interlace)):
        if callable(filters):
            types = [filters(p, y) for y in range(ph)]
        elif isinstance(filters, int):
            types = [filters] * ph
        else:
            types = [filters[(k + y) % len(filters)] for y in range(ph)]
        k += ph
        out += filter_rows(pack_rows(samples[ys::dy, xs::dx], depth), bpp_of(ctype, depth), types)
    return out


def cut(data, sizes):
    """data in pieces of the given sizes, then of the last size (0: the rest in one piece); None: one piece"""
    if sizes is None:
        return [data]
    out, at = [], 0
    for n in sizes:
        out.append(data[at:at + n])
        at += n
    step = sizes[-1] if sizes and sizes[-1] > 0 else len(data) + 1
    while at < len(data):
        out.append(data[at:at + step])
        at += step
    return out


def write(samples, ctype, depth, filters=0, interlace=False, palette=None, trns=None, exif=None, idat_sizes=None, level=6,
          strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, before_idat=(), after_idat=(), stream=None):
    """samples [h][w][channels] (palette files: the indices) -> the file's bytes.  palette [n][3] RGB; trns: bytes of the tRNS chunk;
    exif: the eXIf payload; before_idat / after_idat: ready-made chunks to put there; stream: the filtered bytes to compress instead of the samples' own"""
    samples = np.asarray(samples)
    h, w, c = samples.shape
    assert c == CHANNELS[ctype] and depth in DEPTHS[ctype]
    raw = filtered_stream(samples, ctype, depth, filters, interlace) if stream is None else stream
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    z = co.compress(raw) + co.flush()
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if interlace else 0))
    if exif is not None:
        out += chunk(b"eXIf", exif)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for extra in before_idat:
        out += extra
    for piece in cut(z, idat_sizes):
        out += chunk(b"IDAT", piece)
    for extra in after_idat:
        out += extra
    return out + chunk(b"IEND")


def expected_bgra(samples, ctype, depth, palette=None, trns=None):
    """the answer key: what the pixel rule makes of the known samples, uint8 [h][w][4]"""
    s = np.asarray(samples).astype(np.int64)
    h, w, _ = s.shape
    out = np.zeros((h, w, 4), np.uint8)
    byte = (lambda v: v >> 8) if depth == 16 else (lambda v: v * {1: 255, 2: 85, 4: 17, 8: 1}[depth])
    out[..., 3] = 255
    if ctype == 3:
        pal = np.zeros((256, 4), np.uint8)
        pal[:, 3] = 255
        p = np.asarray(palette, np.uint8)
        pal[:len(p), :3] = p[:, ::-1]
        if trns is not None:
            pal[:len(trns), 3] = np.frombuffer(bytes(trns), np.uint8)
        return pal[s[..., 0]]
    if ctype in (0, 4):
        out[..., 0] = out[..., 1] = out[..., 2] = byte(s[..., 0])
        if ctype == 4:
            out[..., 3] = byte(s[..., 1])
        elif trns is not None:
            out[..., 3] = np.where(s[..., 0] == struct.unpack(">H", bytes(trns))[0], 0, 255)
        return out
    out[..., 0], out[..., 1], out[..., 2] = byte(s[..., 2]), byte(s[..., 1]), byte(s[..., 0])
    if ctype == 6:
        out[..., 3] = byte(s[..., 3])
    elif trns is not None:
        key = np.array(struct.unpack(">HHH", bytes(trns)))
        out[..., 3] = np.where((s[..., :3] == key).all(axis=-1), 0, 255)
    return out


def exif_payload(orientation, big_endian=False):
    """a TIFF structure with the orientation tag alone, as the eXIf chunk holds it"""
    e = ">" if big_endian else "<"
    return (b"MM\x00*" if big_endian else b"II*\x00") + struct.pack(e + "IH", 8, 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
