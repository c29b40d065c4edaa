"""Files with an EXIF orientation tag for the orientation tests, and the eight orientations in numpy (include/ffpic_hip.h, "EXIF
orientation").  A helper, not a test: an APP1 Exif segment in either byte order with the tag as SHORT or LONG among other tags, spliced
behind SOI of a JPEG file; a WebP file's `VP8 ` chunk wrapped into RIFF / VP8X / VP8 / EXIF."""
import struct

import numpy as np

import jpeg_writer
from ffpic_amd import synth

LAYOUTS = {"420": (3, 2, 2), "444": (3, 1, 1), "grey": (1, 1, 1)}
SHORT, LONG = 3, 4

# the table of the header: U = TABLE[o](S), S [h][w][c]
TABLE = {
    1: lambda S: S,
    2: lambda S: S[:, ::-1],
    3: lambda S: S[::-1, ::-1],
    4: lambda S: S[::-1],
    5: lambda S: S.transpose(1, 0, 2),
    6: lambda S: np.rot90(S, -1),
    7: lambda S: S[::-1, ::-1].transpose(1, 0, 2),
    8: lambda S: np.rot90(S, 1),
}
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}


def orient(S, o):
    return np.ascontiguousarray(TABLE[o](S))


def upright_size(w, h, o):
    return (h, w) if o >= 5 else (w, h)


def stored_rect(ws, hs, o, rect):
    """the upright rectangle (x0, y0, w, h) as a rectangle of the stored ws x hs picture: found by marking its pixels, not by a formula"""
    x0, y0, w, h = rect
    marks = orient(np.arange(ws * hs, dtype=np.int64).reshape(hs, ws, 1), o)[y0:y0 + h, x0:x0 + w, 0]
    ys, xs = marks // ws, marks % ws
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def tiff(value, big_endian=False, kind=SHORT, count=1, before=2, after=2, ifd_offset=8, n_entries=None, tag=0x0112):
    """a TIFF structure whose IFD0 holds `before` other tags, the orientation tag, `after` other tags (entries sorted by tag, as TIFF wants)"""
    e = ">" if big_endian else "<"
    entries = [struct.pack(e + "HHII", t, LONG, 1, 72) for t in (0x0100, 0x010F, 0x0110)[:before]]
    field = struct.pack(e + "HH", value & 0xFFFF, 0) if kind == SHORT else struct.pack(e + "I", value & 0xFFFFFFFF)
    entries.append(struct.pack(e + "HHI", tag, kind, count) + field)
    entries += [struct.pack(e + "HHII", t, LONG, 1, 300) for t in (0x011A, 0x0128, 0x0213)[:after]]
    head = (b"MM\x00\x2a" if big_endian else b"II\x2a\x00") + struct.pack(e + "I", ifd_offset)
    ifd = struct.pack(e + "H", len(entries) if n_entries is None else n_entries) + b"".join(entries) + struct.pack(e + "I", 0)
    return head + b"\x00" * max(ifd_offset - 8, 0) + ifd


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif_app1(value, **kw):
    return app1(b"Exif\x00\x00" + tiff(value, **kw))


XMP_APP1 = app1(b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta xmlns:x='adobe:ns:meta/'/>")


def splice(jpeg, *segments):
    """the segments behind SOI"""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + b"".join(segments) + jpeg[2:]


def tagged_jpeg(jpeg, value, **kw):
    return splice(jpeg, exif_app1(value, **kw))


def writer_jpeg(rng, w, h, layout):
    ncomp, hh, vv = LAYOUTS[layout]
    mc, mr = -(-w // (8 * hh)), -(-h // (8 * vv))
    quant = synth.quant_tables()
    coef = [synth._blocks(rng, mc * mr * hh * vv, quant[0])]
    coef += [synth._blocks(rng, mc * mr, quant[1]), synth._blocks(rng, mc * mr, quant[1])] if ncomp == 3 else [None, None]
    return jpeg_writer.encode(w, h, hh, vv, coef, quant)


def _chunks(webp):
    assert webp[:4] == b"RIFF" and webp[8:12] == b"WEBP"
    pos, out = 12, []
    while pos + 8 <= len(webp):
        tag, size = webp[pos:pos + 4], struct.unpack("<I", webp[pos + 4:pos + 8])[0]
        out.append((tag, webp[pos + 8:pos + 8 + size]))
        pos += 8 + size + (size & 1)
    return out


def _chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)


def tagged_webp(webp, value, exif_prefix=False, **kw):
    """RIFF / VP8X / VP8 / EXIF around the file's `VP8 ` chunk.  The canvas fields hold what the library's probe reports without a VP8X
    chunk (the frame's size rounded up to 4: it reads the stored fields as they are, as the reference does), so the picture is the
    same; a VP8X chunk the file has is kept."""
    chunks = dict(_chunks(webp))
    vp8 = chunks[b"VP8 "]
    fw, fh = (struct.unpack("<H", vp8[6:8])[0] & 0x3FFF), (struct.unpack("<H", vp8[8:10])[0] & 0x3FFF)
    w4, h4 = (fw + 3) // 4 * 4, (fh + 3) // 4 * 4
    vp8x = chunks.get(b"VP8X") or b"\x00\x00\x00\x00" + struct.pack("<I", w4)[:3] + struct.pack("<I", h4)[:3]
    vp8x = bytes([vp8x[0] | 0x08]) + vp8x[1:]                                   # the EXIF flag
    body = b"WEBP" + _chunk(b"VP8X", vp8x) + _chunk(b"VP8 ", vp8) + _chunk(b"EXIF", (b"Exif\x00\x00" if exif_prefix else b"") + tiff(value, **kw))
    return b"RIFF" + struct.pack("<I", len(body)) + body
