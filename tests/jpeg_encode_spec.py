"""The baseline JPEG ENCODER's rule in numpy, written from the rule's text in include/ffpic_hip.h: libjpeg's quantiser
tables of a quality, its RGB -> YCbCr, its edge replication and chroma downsampling, its dummy blocks, the "islow" forward DCT and its
quantiser.  Pixels to coefficients here; the scan is tests/jpeg_writer.encode's, behind which the JFIF segment is put in.  The answer key of
the encoder's tests: test_jpeg_encode_spec.py holds it to PIL (libjpeg-turbo) byte for byte, the library's tests hold the library to it.
Test infrastructure, not product code."""
import numpy as np

import jpeg_writer

LAYOUTS = {"4:4:4": (1, 1, 3), "4:2:2": (2, 1, 3), "4:2:0": (2, 2, 3), "grey": (1, 1, 1)}      # name -> (h, v, components)
LAYOUT_ID = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2, "grey": 3}                                    # FFHIP_JPEG_ENC_*
JFIF = bytes([0xFF, 0xE0, 0, 16]) + b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])

# T.81 K.1 and K.2, natural order
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                      + [99] * 32)


def tables(quality):
    """step 1 -> uint16 [4][64] natural order: slot 0 luma, slot 1 chroma (2 and 3 unused, ones)"""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    out = np.ones((4, 64), np.uint16)
    for slot, std in enumerate((STD_LUMA, STD_CHROMA)):
        out[slot] = np.clip((std * s + 50) // 100, 1, 255)
    return out


def ycc(rgb):
    """step 2: [H][W][3] uint8 R,G,B -> Y, Cb, Cr planes (int64)"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    """edge replication down to `rows` and right to `cols`"""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def chroma_plane(full, h, v, mcu_cols, mcu_rows):
    """step 3: a full-resolution chroma plane -> the component's padded sample plane [8 mcu_rows][8 mcu_cols]"""
    H = full.shape[0]
    p = _pad(full, -(-H // v) * v, 8 * h * mcu_cols)            # rows only to a multiple of v, columns to the MCU width
    if (h, v) == (2, 2):
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        p = (s + 1 + (np.arange(s.shape[1]) & 1)) >> 2
    elif (h, v) == (2, 1):
        s = p[:, 0::2] + p[:, 1::2]
        p = (s + (np.arange(s.shape[1]) & 1)) >> 1
    return _pad(p, 8 * mcu_rows, p.shape[1])                  # the rows still missing: the last downsampled row


C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819,
         c2562=20995, c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of jfdctint.c over the LAST axis of d [..., 8] (int64 holding what the 32-bit arithmetic holds)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * C["c0541"]
    out[2] = _descale(z1 + t13 * C["c0765"], n)
    out[6] = _descale(z1 - t12 * C["c1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["c1175"]
    t4, t5, t6, t7 = t4 * C["c0298"], t5 * C["c2053"], t6 * C["c3072"], t7 * C["c1501"]
    z1, z2, z3, z4 = -z1 * C["c0899"], -z2 * C["c2562"], -z3 * C["c1961"] + z5, -z4 * C["c0390"] + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct_quant(blocks, quant):
    """steps 5 and 6: [n][8][8] samples 0..255, quant [64] -> int16 [n][64] natural order"""
    d = blocks.astype(np.int64) - 128
    d = _pass(d, True)                                         # rows
    d = np.swapaxes(_pass(np.swapaxes(d, -1, -2), False), -1, -2)  # columns
    x = d.reshape(-1, 64)
    div = 8 * quant.astype(np.int64)
    c = (np.abs(x) + (div >> 1)) // div
    return (np.sign(x) * c).astype(np.int16)


def _mcu_order(plane, h, v, mcu_cols, mcu_rows):
    """raster plane [8 v mcu_rows][8 h mcu_cols] -> [blocks][8][8] in MCU order"""
    p = plane.reshape(mcu_rows, v, 8, mcu_cols, h, 8)
    return p.transpose(0, 3, 1, 4, 2, 5).reshape(-1, 8, 8)


def coefficients(pixels, layout, quality):
    """pixels: [H][W][3] uint8 RGB, or [H][W] grey for layout "grey" -> ([coef_y, coef_u, coef_v] int16 flat, MCU order (None for grey's
    chroma), quant [4][64])"""
    h, v, ncomp = LAYOUTS[layout]
    pixels = np.asarray(pixels)
    H, W = pixels.shape[:2]
    assert (pixels.ndim == 2) == (ncomp == 1)
    mcu_cols, mcu_rows = -(-W // (8 * h)), -(-H // (8 * v))
    quant = tables(quality)
    if ncomp == 1:
        y, cb, cr = pixels.astype(np.int64), None, None
    else:
        y, cb, cr = ycc(pixels)
    yp = _pad(y, 8 * v * mcu_rows, 8 * h * mcu_cols)
    cy = fdct_quant(_mcu_order(yp, h, v, mcu_cols, mcu_rows), quant[0]).reshape(mcu_rows, mcu_cols, v, h, 64)
    # step 4: dummy blocks, in the MCU's block order
    bw, bh = -(-W // 8), -(-H // 8)
    for my in (mcu_rows - 1,):
        for mx in range(mcu_cols):
            _dummies(cy, my, mx, h, v, bw, bh)
    for mx in (mcu_cols - 1,):
        for my in range(mcu_rows):
            _dummies(cy, my, mx, h, v, bw, bh)
    out = [np.ascontiguousarray(cy.reshape(-1))]
    for c in (cb, cr):
        if c is None:
            out.append(None)
            continue
        cp = chroma_plane(c, h, v, mcu_cols, mcu_rows)
        out.append(np.ascontiguousarray(fdct_quant(_mcu_order(cp, 1, 1, mcu_cols, mcu_rows), quant[1]).reshape(-1)))
    return out, quant


def _dummies(cy, my, mx, h, v, bw, bh):
    prev = None
    for vi in range(v):
        for hi in range(h):
            blk = cy[my, mx, vi, hi]
            if mx * h + hi >= bw or my * v + vi >= bh:
                blk[:] = 0
                blk[0] = prev
            prev = blk[0]


def with_jfif(data):
    assert data[:2] == b"\xff\xd8"
    return data[:2] + JFIF + data[2:]


def file_from_coefficients(width, height, layout, coef, quant, restart=0):
    """the file of given coefficient planes: jpeg_writer.encode's with the JFIF segment behind SOI"""
    h, v, ncomp = LAYOUTS[layout]
    return with_jfif(jpeg_writer.encode(width, height, h, v, coef, quant, (0, 1, 1), restart))


def encode(pixels, layout, quality, restart=0):
    """-> the file's bytes"""
    pixels = np.asarray(pixels)
    coef, quant = coefficients(pixels, layout, quality)
    return file_from_coefficients(pixels.shape[1], pixels.shape[0], layout, coef, quant, restart)
