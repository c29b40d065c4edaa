"""Writes lossy WebP files with an alpha plane from a known plane: VP8X + ALPH + the VP8 chunk of a carrier file.  The ALPH payload is the
header byte (reserved 2 bits, pre-processing 2, filter 2, compression 2) and the FILTERED plane, raw or as a headerless VP8L stream built
from vp8l_writer's functions (the stream starts at the first transform bit; alpha is the green byte).  The knobs write the odd and the
damaged files of webp_alpha_cases."""
import numpy as np

import vp8l_writer as W

RAW, LOSSLESS = 0, 1
NONE, HORIZONTAL, VERTICAL, GRADIENT = 0, 1, 2, 3


def filter_plane(plane, f):
    """the plane as the chunk stores it under filter f: every sample minus its prediction from the FINISHED plane, mod 256"""
    a = np.asarray(plane, dtype=np.int64)
    h, w = a.shape
    if f == NONE:
        return a.astype(np.uint8)
    left = np.zeros_like(a)
    left[:, 1:] = a[:, :-1]
    left[1:, 0] = a[:-1, 0]                                       # column 0 predicts from above; (0, 0) from 0
    up = np.zeros_like(a)
    up[1:] = a[:-1]
    corner = np.zeros_like(a)
    corner[1:, 1:] = a[:-1, :-1]
    if f == HORIZONTAL:
        pred = left
    elif f == VERTICAL:
        pred = up.copy()
    else:
        pred = np.clip(left + up - corner, 0, 255)
    pred[0] = left[0]                                             # row 0 is horizontal under every filter
    pred[1:, 0] = a[:-1, 0]
    return ((a - pred) & 255).astype(np.uint8)


def headerless(argb, transforms=(), cache_bits=0, codes=None):
    """a VP8L stream without signature and header: [transform]* 0 image"""
    argb = np.asarray(argb, dtype=np.uint32)
    h, w = argb.shape
    bw = W.BitWriter()
    words, xs = [int(v) for v in argb.reshape(-1)], w
    for tr in transforms:
        tr = dict(tr)
        t = tr["type"]
        bw.put(1, 1)
        bw.put(t, 2)
        if t == W.COLOR_INDEXING:
            tr["bits"] = W.bundle_bits(len(tr["palette"]))
        words = W.forward(words, xs, h, tr)
        if t in (W.PREDICTOR, W.CROSS_COLOR):
            img = np.asarray(tr["image"], dtype=np.uint32)
            bw.put(tr["bits"] - 2, 3)
            W.put_image(bw, W.literal_tokens(img.reshape(-1)), img.shape[1], img.shape[0], False)
        elif t == W.COLOR_INDEXING:
            pal = [int(p) for p in tr["palette"]]
            bw.put(len(pal) - 1, 8)
            diff = [pal[0]] + [W._pack([a - b for a, b in zip(W._ch(pal[k]), W._ch(pal[k - 1]))]) for k in range(1, len(pal))]
            W.put_image(bw, W.literal_tokens(diff), len(pal), 1, False)
            xs = W.sub(xs, tr["bits"])
    bw.put(0, 1)
    W.put_image(bw, W.literal_tokens(words, cache_bits, True), xs, h, True, cache_bits, None, codes)
    return bw.bytes()


def green(plane):
    return np.uint32(0xff000000) | (np.asarray(plane, dtype=np.uint32) << 8)


def vp8_chunk(carrier):
    """the payload of a file's `VP8 ` chunk (chunks padded to even sizes)"""
    pos = 12
    while carrier[pos:pos + 4] != b"VP8 ":
        size = int.from_bytes(carrier[pos + 4:pos + 8], "little")
        pos += 8 + size + (size & 1)
    size = int.from_bytes(carrier[pos + 4:pos + 8], "little")
    return carrier[pos + 8:pos + 8 + size]


def frame_size(vp8):
    return int.from_bytes(vp8[6:8], "little") & 0x3fff, int.from_bytes(vp8[8:10], "little") & 0x3fff


def alph_payload(plane, compression=RAW, filter=NONE, pre=0, reserved=0, transforms=(), cache_bits=0, codes=None, header=None):
    stored = filter_plane(plane, filter)
    body = stored.tobytes() if compression == RAW else headerless(green(stored), transforms, cache_bits, codes)
    head = (reserved << 6 | pre << 4 | filter << 2 | compression) if header is None else header
    return bytes([head]) + body


def assemble(chunks):
    body = b"WEBP" + b"".join(W.chunk(t, p) for t, p in chunks)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def wrap(carrier, plane=None, compression=RAW, filter=NONE, pre=0, transforms=(), cache_bits=0, vp8x_alpha=True, vp8x=True, payload=None,
         alph_behind=False, extra=(), trailing=b"", **how):
    """VP8X + ALPH + the carrier's VP8 chunk.  payload: the ALPH chunk's bytes as given (damaged files); plane None and payload None: no
    ALPH chunk; vp8x False: no VP8X chunk; alph_behind: the ALPH chunk behind the VP8 chunk; extra: further (tag, payload) chunks between
    VP8X and ALPH; trailing: bytes appended to the ALPH payload (an odd size exercises the padding byte)"""
    vp8 = vp8_chunk(carrier)
    w, h = frame_size(vp8)
    chunks = []
    if vp8x:
        chunks.append((b"VP8X", bytes([0x10 if vp8x_alpha else 0, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")))
    chunks += list(extra)
    if payload is None and plane is not None:
        payload = alph_payload(plane, compression, filter, pre, transforms=transforms, cache_bits=cache_bits, **how)
    alph = [(b"ALPH", payload + trailing)] if payload is not None else []
    chunks += ([(b"VP8 ", vp8)] + alph) if alph_behind else (alph + [(b"VP8 ", vp8)])
    return assemble(chunks)


def chunks_of(file):
    """[(tag, payload)] of a RIFF/WEBP file whose chunks are padded to even sizes"""
    pos, out = 12, []
    while pos + 8 <= len(file):
        size = int.from_bytes(file[pos + 4:pos + 8], "little")
        out.append((file[pos:pos + 4], file[pos + 8:pos + 8 + size]))
        pos += 8 + size + (size & 1)
    return out


def with_alph(file, change):
    """the file with its ALPH payload replaced by change(payload)"""
    return assemble([(t, change(p) if t == b"ALPH" else p) for t, p in chunks_of(file)])
