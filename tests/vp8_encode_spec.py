"""The numpy witness of the lossy WebP encoder's rule (include/ffpic_hip.h "Lossy WebP encoding"): colour, modes, levels
and reconstruction from the rule's text, in Python integers and numpy; nothing of ffpic_amd is used.  The inverse side -- dequantisation,
inverse WHT and DCT, the four predictions, clamping -- is not restated: it IS tests/vp8_spec.py's with rules=SPEC (`_residual`, `_recon_mb`),
the decoder PIL is held to, so the witness's reconstruction is what a decoder shows by construction.  The file is written by
tests/vp8_writer.keyframe_from(valid=True) from the witness's own modes and levels.

  quality_index(q), steps(qi), auto_filter(qi), parts_log2(rows)
  planes(px)                 px: uint8 [H][W][3] RGB or [H][W] grey -> y, u, v of the whole macroblock grid
  fdct(d), fwht(x)           16 ints -> 16 ints
  encode_mbs(px, quality)    -> dict(ymode, uvmode, levels [n][25][16], skip [n], y, u, v = the reconstruction, qi, cols, rows)
  header(px, quality, filter) -> dict(y_ac_qi, level, log2_parts, prob_skip)
  file(px, quality, filter)  -> bytes"""
import numpy as np

import vp8_spec as S
import vp8_writer as W

QUALITY_QI = (127, 103, 96, 92, 89, 86, 83, 81, 79, 77, 75, 73, 72, 70, 69, 68, 66, 65, 64, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 51,
              50, 49, 48, 48, 47, 46, 45, 45, 44, 43, 43, 42, 41, 41, 40, 40, 39, 38, 38, 37, 37, 36, 36, 35, 35, 34, 33, 33, 32, 32, 31, 31, 30,
              30, 29, 29, 28, 28, 28, 27, 27, 26, 26, 24, 23, 22, 21, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0)
LEVEL_MAX = 2047
_R = S._Rules(S.SPEC)
_MBS = {}


def quality_index(quality):
    return QUALITY_QI[quality]


def steps(qi):
    """y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac as a decoder derives them from the index, all deltas 0"""
    return [int(v) for v in S._quant(_R, 0, 0, 0, [0] * 4, qi, [0] * 5)[0]]


def auto_filter(qi):
    return min(63, (5 * qi) >> 4)


def parts_log2(rows):
    return 3 if rows >= 8 else 2 if rows >= 4 else 1 if rows >= 2 else 0


def planes(px):
    px = np.asarray(px)
    rgb = (np.repeat(px[:, :, None], 3, 2) if px.ndim == 2 else px).astype(np.int64)
    h, w = rgb.shape[:2]
    cols, rows = (w + 15) >> 4, (h + 15) >> 4
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16
    even = np.pad(rgb, ((0, h & 1), (0, w & 1), (0, 0)), mode="edge")           # the last column and row repeated
    cell = even[0::2, 0::2] + even[0::2, 1::2] + even[1::2, 0::2] + even[1::2, 1::2]
    r, g, b = cell[..., 0], cell[..., 1], cell[..., 2]
    u = np.clip((-9719 * r - 19081 * g + 28800 * b + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    v = np.clip((28800 * r - 24116 * g - 4684 * b + (128 << 18) + (1 << 17)) >> 18, 0, 255)

    def grid(p, n):
        return np.pad(p, ((0, n * rows - p.shape[0]), (0, n * cols - p.shape[1])), mode="edge").astype(np.uint8)
    return grid(y, 16), grid(u, 8), grid(v, 8)


def fdct(d):
    d = [int(v) for v in d]
    t = [0] * 16
    for i in range(4):
        d0, d1, d2, d3 = d[4 * i:4 * i + 4]
        a0, a1, a2, a3 = d0 + d3, d1 + d2, d1 - d2, d0 - d3
        t[4 * i:4 * i + 4] = (a0 + a1) * 8, (a2 * 2217 + a3 * 5352 + 1812) >> 9, (a0 - a1) * 8, (a3 * 2217 - a2 * 5352 + 937) >> 9
    o = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = t[i] + t[12 + i], t[4 + i] + t[8 + i], t[4 + i] - t[8 + i], t[i] - t[12 + i]
        o[i] = (a0 + a1 + 7) >> 4
        o[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0)
        o[8 + i] = (a0 - a1 + 7) >> 4
        o[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16
    return o


def fwht(x):
    x = [int(v) for v in x]
    t = [0] * 16
    for i in range(4):
        x0, x1, x2, x3 = x[4 * i:4 * i + 4]
        a0, a1, a2, a3 = x0 + x2, x1 + x3, x1 - x3, x0 - x2
        t[4 * i:4 * i + 4] = a0 + a1, a3 + a2, a3 - a2, a0 - a1
    o = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = t[i] + t[8 + i], t[4 + i] + t[12 + i], t[4 + i] - t[12 + i], t[i] - t[8 + i]
        o[i], o[4 + i], o[8 + i], o[12 + i] = (a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1
    return o


def quantise(c, step, bias):
    level = min(LEVEL_MAX, (abs(c) + bias) // step)
    return -level if c < 0 else level


def _best(src, rec, x0, y0, n, x, y):
    """per mode the prediction of every plane in `src`, and the lowest mode with the smallest sum of squared differences"""
    preds, sums = [], [0] * 4
    for s, r in zip(src, rec):
        above, left, corner = S._edges(r, x0, y0, n)
        p = [S._pred_block(m, n, above, left, corner, x, y) for m in range(4)]
        preds.append(p)
        for m in range(4):
            sums[m] += int(((s[y0:y0 + n, x0:x0 + n].astype(np.int64) - p[m]) ** 2).sum())
    mode = min(range(4), key=lambda m: (sums[m], m))
    return mode, [p[mode] for p in preds]


def encode_mbs(px, quality):
    px = np.asarray(px)
    key = (px.tobytes(), px.shape, quality)
    if key in _MBS:
        return _MBS[key]
    sy, su, sv = planes(px)
    rows, cols = sy.shape[0] >> 4, sy.shape[1] >> 4
    n = rows * cols
    qi = quality_index(quality)
    q = steps(qi)
    Y, U, V = np.zeros(sy.shape, np.int64), np.zeros(su.shape, np.int64), np.zeros(su.shape, np.int64)
    ymode, uvmode, levels = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 25, 16), np.int16)
    for mby in range(rows):
        for mbx in range(cols):
            mb = mby * cols + mbx
            ym, (py,) = _best([sy], [Y], 16 * mbx, 16 * mby, 16, mbx, mby)
            uvm, (pu, pv) = _best([su, sv], [U, V], 8 * mbx, 8 * mby, 8, mbx, mby)
            ymode[mb], uvmode[mb] = ym, uvm
            coef = []
            dy = sy[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16].astype(np.int64) - py
            for b in range(16):
                coef.append(fdct(dy[4 * (b >> 2):4 * (b >> 2) + 4, 4 * (b & 3):4 * (b & 3) + 4].reshape(16)))
            for s, p in ((su, pu), (sv, pv)):
                d = s[8 * mby:8 * mby + 8, 8 * mbx:8 * mbx + 8].astype(np.int64) - p
                for b in range(4):
                    coef.append(fdct(d[4 * (b >> 1):4 * (b >> 1) + 4, 4 * (b & 1):4 * (b & 1) + 4].reshape(16)))
            lv = levels[mb]
            y2 = fwht([coef[b][0] for b in range(16)])
            lv[24] = [quantise(y2[i], q[3] if i else q[2], (q[3] if i else q[2]) >> 1) for i in range(16)]
            for b in range(16):
                lv[b, 1:] = [quantise(coef[b][i], q[1], (3 * q[1]) >> 3) for i in range(1, 16)]
            for b in range(16, 24):
                lv[b, 0] = quantise(coef[b][0], q[4], q[4] >> 1)
                lv[b, 1:] = [quantise(coef[b][i], q[5], (3 * q[5]) >> 3) for i in range(1, 16)]
            res, _ = S._residual(lv, [16] * 25, True, q, _R)
            S._recon_mb(_R, Y, U, V, mbx, mby, cols, [ym, uvm], res)
    out = dict(ymode=ymode, uvmode=uvmode, levels=levels, skip=(~levels.reshape(n, -1).any(axis=1)).astype(np.uint8), y=Y.astype(np.uint8),
               u=U.astype(np.uint8), v=V.astype(np.uint8), qi=qi, cols=cols, rows=rows)
    _MBS[key] = out
    return out


def header(px, quality, filter):
    m = encode_mbs(px, quality)
    total = len(m["skip"])
    coded = total - int(m["skip"].sum())
    return dict(y_ac_qi=m["qi"], level=auto_filter(m["qi"]) if filter < 0 else filter, log2_parts=parts_log2(m["rows"]),
                prob_skip=min(255, max(1, (256 * coded + total // 2) // total)))


def file(px, quality, filter):
    px = np.asarray(px)
    m = encode_mbs(px, quality)
    n = len(m["ymode"])
    mbs = dict(ymode=m["ymode"], bmodes=np.zeros((n, 16), np.uint8), uvmode=m["uvmode"], seg=np.zeros(n, np.uint8), skip=m["skip"], levels=m["levels"])
    return W.keyframe_from(px.shape[1], px.shape[0], mbs, valid=True, pad=0, filter_type=0, sharpness=0, **header(px, quality, filter))
