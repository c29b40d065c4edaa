"""The reduced-size JPEG reconstruction (include/ffpic_hip.h, "JPEG pictures at 1/2, 1/4 and 1/8 size") restated in numpy
from the rule's text, for the tests to hold the library against: the block rule over many blocks at once, and a whole picture at a
denominator -- block placement, chroma replication, the reference's colour expressions (utils/colorspace.c:148-164) in float64, one
operation at a time.  Nothing here is taken from the library."""
import numpy as np

T = {1: np.array([[8192]], np.int64),
     2: np.array([[8192, 8192], [8192, -8192]], np.int64),
     4: np.array([[8192, 10703, 8192, 4433], [8192, 4433, -8192, -10703], [8192, -4433, -8192, 10703], [8192, -10703, 8192, -4433]], np.int64)}


def basis(n):
    """the matrices from their definition: round(8192 sqrt(2) alpha(u) cos((2 x + 1) u pi / 2 N)), alpha(0) = 1 / sqrt(2), 1 otherwise"""
    x, u = np.mgrid[0:n, 0:n]
    alpha = np.where(u == 0, 1 / np.sqrt(2), 1.0)
    return np.rint(8192 * np.sqrt(2) * alpha * np.cos((2 * x + 1) * u * np.pi / (2 * n))).astype(np.int64)


def _int16(a):
    return ((a + 32768) & 0xffff) - 32768


def blocks(coef, quant, denom):
    """coef int16 [n][64], quant uint16 [64] (natural order) -> int64 [n][N][N], N = 8 / denom"""
    n = 8 // denom
    t = T[n]
    F = _int16(np.asarray(coef, np.int64).reshape(-1, 8, 8)[:, :n, :n] * np.asarray(quant, np.int64).reshape(8, 8)[:n, :n])   # F[b][v][u]
    c = _int16((np.einsum("yv,bvu->byu", t, F) + 1024) >> 11)
    s = (np.einsum("xu,byu->byx", t, c) + (257 << 17)) >> 18
    assert np.abs(np.einsum("xu,byu->byx", np.abs(t), np.abs(c))).max(initial=0) < 2 ** 31 - (257 << 17)                    # int32 holds every sum
    return np.maximum(s, 0)


def bgra_of(yy, u, v):
    """the reference's conversion of int16 samples, every double operation rounded on its own; arrays of one shape -> [...][4] uint8"""
    yy, uu, vv = yy.astype(np.float64), (u - 128).astype(np.float64), (v - 128).astype(np.float64)
    r = yy + 1.280 * vv
    g = yy - 0.215 * uu
    g = g - 0.381 * vv
    b = yy + 2.128 * uu
    px = np.stack([np.clip(np.trunc(c), 0, 255) for c in (b, g, r)] + [np.full(yy.shape, 255.0)], axis=-1)
    return px.astype(np.uint8)


def planes(mcu_cols, mcu_rows, ncomp, h, v, cy, cu, cv, quant, denom, qt_id=(0, 1, 1)):
    """-> (Y, U, V) int64 [N v mcu_rows][N h mcu_cols] at the scaled coded size, chroma replicated h x v (grey: zeros)"""
    n = 8 // denom
    quant = np.asarray(quant).reshape(4, 64)
    Y = blocks(np.asarray(cy).reshape(-1, 64), quant[qt_id[0]], denom).reshape(mcu_rows, mcu_cols, v, h, n, n)
    Y = Y.transpose(0, 2, 4, 1, 3, 5).reshape(mcu_rows * v * n, mcu_cols * h * n)
    if ncomp == 1:
        return Y, np.zeros_like(Y), np.zeros_like(Y)
    out = [Y]
    for comp, c in ((1, cu), (2, cv)):
        s = blocks(np.asarray(c).reshape(-1, 64), quant[qt_id[comp]], denom).reshape(mcu_rows, mcu_cols, n, n)
        py, px = np.arange(n * v) // v, np.arange(n * h) // h                       # pixel (y, x) of the MCU takes sample (y / v, x / h)
        s = s[:, :, py][:, :, :, px]
        out.append(s.transpose(0, 2, 1, 3).reshape(mcu_rows * v * n, mcu_cols * h * n))
    return tuple(out)


def picture(mcu_cols, mcu_rows, ncomp, h, v, cy, cu, cv, quant, denom, qt_id=(0, 1, 1)):
    """the BGRA picture [N v mcu_rows][N h mcu_cols][4] at the scaled coded size"""
    return bgra_of(*planes(mcu_cols, mcu_rows, ncomp, h, v, cy, cu, cv, quant, denom, qt_id))


def scaled_len(n, d):
    return -(-n // d)


def mapped_rect(width, height, d, roi):
    """(x0, y0, w, h) of the full-size display picture -> the rectangle of the picture at 1 / d"""
    x0, y0, w, h = roi
    X0, Y0 = x0 // d, y0 // d
    X1, Y1 = min(scaled_len(width, d), scaled_len(x0 + w, d)), min(scaled_len(height, d), scaled_len(y0 + h, d))
    return X0, Y0, X1 - X0, Y1 - Y0


def choose(rect_w, rect_h, out_w, out_h):
    for d in (8, 4, 2):
        if scaled_len(rect_w, d) >= out_w and scaled_len(rect_h, d) >= out_h:
            return d
    return 1
