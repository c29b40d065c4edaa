"""The PNG encoder's witness: the filter rule of include/ffpic_hip.h ("PNG encoding") written once more with numpy, and nothing of the
library -- the five filters, the adaptive choice (the smallest sum of absolute values of the filtered bytes read as signed 8-bit, the lowest
type among equals), the filtered picture -- and the walk over a file's chunks that the tests read the encoder's files with."""
import struct
import zlib

import numpy as np

ADAPTIVE = 5
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def as_hwc(samples):
    """uint8 [H][W] or [H][W][C] -> [H][W][C]"""
    s = np.asarray(samples)
    assert s.dtype == np.uint8 and s.ndim in (2, 3)
    return s[..., None] if s.ndim == 2 else s


def row_filters(row, above, bpp):
    """the five filtered forms of one row of bytes (int arrays in, uint8 [5][n] out); `above` is zeros for the first row"""
    n = row.size
    a = np.concatenate([np.zeros(bpp, np.int32), row[:n - bpp]]) if n > bpp else np.zeros(n, np.int32)
    b = above
    c = np.concatenate([np.zeros(bpp, np.int32), above[:n - bpp]]) if n > bpp else np.zeros(n, np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([row, row - a, row - b, row - (a + b) // 2, row - paeth]).astype(np.int64) % 256


def row_sums(forms):
    """the adaptive rule's five sums of a row's filtered forms"""
    return np.where(forms < 128, forms, 256 - forms).sum(axis=1)


def filtered(samples, filter=ADAPTIVE):
    """-> (the filtered picture's bytes, the rows' types, the rows' five sums [H][5])"""
    s = as_hwc(samples)
    h, w, c = s.shape
    rows = s.reshape(h, w * c).astype(np.int32)
    out, types, sums = bytearray(), [], []
    for y in range(h):
        forms = row_filters(rows[y], rows[y - 1] if y else np.zeros(w * c, np.int32), c)
        sm = row_sums(forms)
        t = int(np.argmin(sm)) if filter == ADAPTIVE else filter          # argmin: the first of equal ones
        types.append(t)
        sums.append(sm)
        out.append(t)
        out += forms[t].astype(np.uint8).tobytes()
    return bytes(out), types, np.array(sums)


def chunks(data):
    """[(type, body)] of a file; asserts the signature, every CRC and that nothing follows IEND"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and zlib.crc32(kind + body) == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0], (kind, at)
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def to_bgra(samples):
    """the samples as the decoders' BGRA picture [H][W][4]"""
    s = as_hwc(samples)
    h, w, c = s.shape
    out = np.full((h, w, 4), 255, np.uint8)
    if c <= 2:
        out[..., :3] = s[..., :1]
    else:
        out[..., :3] = s[..., 2::-1]
    if c in (2, 4):
        out[..., 3] = s[..., c - 1]
    return out
