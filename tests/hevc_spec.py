"""A plain witness for the two HEVC stages -- levels to residual, and TU list plus residual to planes -- written from Rec. ITU-T
H.265 clauses 8.6.2 to 8.6.6 (scaling, transformation, residual modification, cross-component prediction) and 8.4.4.2.1 to
8.4.4.2.6 (intra sample prediction).  Python and numpy only, on int64 values that cannot wrap; nothing of ffpic_amd's native
code, the oracle, the reference or the goldens is used (ffpic_amd.synth gives the TU record's dtype and flag values alone).

Two rule sets, as tests/vp8_spec.py has them:
  SPEC       the standard.
  REFERENCE  SPEC with every NAMED DEVIATION of `FLAGS` switched on: what the project's default residuals and pictures are by
             contract.
A deviation is a flag of its own and changes one rule; it is never a tolerance.  Both entry points take any subset of the flags, so
a test can switch one on alone over SPEC or one off alone from REFERENCE.  `UNEXPLAINED` lists differences between REFERENCE and
the oracle that no rule accounts for; it is empty.

The interfaces are those of the stages:
  residual(levels[n_tu][n*n], info[n_tu][4], n, bitdepth, epp, scaling, rules) -> int64 [n_tu][n*n], row-major (x fastest)
      info[:, 0] = qP, [:, 1] = flags (1 the 4x4 luma intra TU that takes the DST, 2 transform_skip_flag, 4 cu_transquant_bypass_flag,
      8 rotation of a 4x4 block), [:, 2] = the row of `scaling` (uint8 [6][n*n], the ScalingFactor of 7.4.5; None = flat 16)
  intra(tus, residual, width, height, chroma, bd_y, bd_c, csub, rules) -> (y, u, v) int16 planes that started at 0
      tus = records of synth.HEVC_TU_DTYPE in decode order.  What 6.4.1 derives while a stream is parsed arrives in the record:
      availability per neighbouring sample (avail_top bit k = p[k][-1], avail_left bit k = p[-1][k], TU_CORNER = p[-1][-1]), and
      what depends on syntax elements outside the stage: TU_FILTER (8.4.4.2.3 may run: cIdx = 0 or ChromaArrayType = 3),
      TU_STRONG (strong_intra_smoothing_enabled_flag), TU_NO_BF / TU_NO_DC_BF (disableIntraBoundaryFilter for the angular / DC edge
      filters), TU_RDPCM (8.6.5 applies; the direction follows predModeIntra 10 / 26), TU_CCP with res_scale = ResScaleVal.

What SPEC does not cover:
  extended_precision_processing_flag = 1.  The editions of H.265 differ on transform skip there (tsShift, the coefficient range) and
      no text of the standard is at hand to settle it.  With epp = 1 the witness applies the epp = 0 rules with the wider
      log2TransformRange = Max(15, BitDepth + 6) and bdShift = Max(20 - BitDepth, 11); that is a reading, not the standard, and
      only REFERENCE (held to the oracle) is asserted there.
  Parsing and CABAC: the library has neither, so the witness starts where the stages start.
  Bit depths above 15 in intra(): the stage refuses them.  That is also why two wraps of the reference are no rules here: the int16
      store of a predicted sample and the uint16 read of a neighbour cannot move a sample while every sample of a plane is clipped to
      0 .. 2^15 - 1 at the most.  Nor is the 32-bit product of the reference's 8.6.6 a rule: a wrap moves it by a multiple of 2^32,
      hence the sum by a multiple of 2^29 after the `>> 3`, and the int16 store that follows (resmod_int16) cannot see that.
"""
import numpy as np

from ffpic_amd.synth import TU_CCP, TU_CORNER, TU_FILTER, TU_NO_BF, TU_NO_DC_BF, TU_RDPCM, TU_RESIDUAL, TU_STRONG

FLAGS = {
    # ---- rules that touch conformant streams
    "dst_round_is_shift_minus_1": "the 4x4 DST adds `shift - 1` before each of its two shifts: 6 where 8.6.4.2 has 64, bdShift - 1 "
                                  "where 8.6.2 has 1 << (bdShift - 1) (utils/idct.c:31; oracle/ffo_hevc.c:56-57)",
    "ts_without_bdshift": "a transform-skipped block is stored as d << tsShift; the (r + (1 << (bdShift - 1))) >> bdShift of 8.6.2 is "
                          "never applied to it (coding/hevc.c:4227-4246; oracle/ffo_hevc.c:143-150)",
    "rdpcm_horizontal_runs_on": "horizontal rdpcm is a running sum over the flattened block from index nTbS on: it crosses row ends and "
                                "leaves row 0 alone, where 8.6.5 accumulates along every row (coding/hevc.c:3960-3977; "
                                "oracle/ffo_hevc_intra.c:140-149)",
    "ccp_reads_chroma": "cross-component prediction takes the chroma block itself for rY, where 8.6.6 takes the luma residual "
                        "(coding/hevc.c:4750-4756; oracle/ffo_hevc_intra.c:152-162)",
    # ---- wraps and clips that matter outside the standard's value ranges only
    "dst_clips_second_pass": "the 4x4 DST clips its second pass to coeffMin .. coeffMax as it does the first; 8.6.4.2 clips the first "
                             "alone.  Live above bit depth 12 (utils/idct.c:9-55; oracle/ffo_hevc.c:57)",
    "scale_wraps_32": "the scaling product, its shift by qP / 6 and the rounding add are 32 bits wide (coding/hevc.c:3743-3816; "
                      "oracle/ffo_hevc.c:86-89)",
    "coeffs_int16": "scaled coefficients d and the first transform pass g are held in int16_t, which is narrower than coeffMin .. "
                    "coeffMax once extended precision widens that range (coding/hevc.c:3793, 3888-3956; oracle/ffo_hevc.c:89, 117)",
    "residual_int16": "the second transform pass is stored in int16_t (coding/hevc.c:3951; oracle/ffo_hevc.c:57, 123)",
    "ts_shift_int16": "the shifted transform-skip value is stored in int16_t (coding/hevc.c:4229-4236; oracle/ffo_hevc.c:148)",
    "resmod_int16": "rdpcm sums and the cross-component sum are stored in int16_t (coding/hevc.c:3960-3988; "
                    "oracle/ffo_hevc_intra.c:145-160)",
}
SPEC = frozenset()
REFERENCE = frozenset(FLAGS)
UNEXPLAINED = []           # (where, what): differences between REFERENCE and the oracle that no flag explains


def _rules(rules):
    rules = frozenset(rules)
    assert rules <= REFERENCE, rules - REFERENCE
    return rules


def _wrap(v, bits):
    """v as a two's complement integer of `bits` bits"""
    half = np.int64(1) << (bits - 1)
    return ((v + half) & ((np.int64(1) << bits) - 1)) - half


# ------------------------------------------------------------------------------------------------- tables

# 8.6.4.2, equation for transMatrix: its first column, c(n) = transMatrix[n][0] for n = 0 .. 31, and c(32) = 0.  Row 0 is the DC row
# (64 = 64 sqrt2 / sqrt2); for n >= 1, c(n) ~ 64 sqrt2 cos(n pi / 64).
COS = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0)
assert len(COS) == 33


def _c(k):
    """c extended over a period: the cosine's symmetries c(64 - k) = -c(k), c(64 + k) = -c(k), c(128 - k) = c(k)"""
    k %= 128
    if k <= 32:
        return COS[k]
    if k <= 64:
        return -COS[64 - k]
    if k <= 96:
        return -COS[k - 64]
    return COS[128 - k]


def dct_matrix(n):
    """transMatrix rows 0, 32/n, 2 * 32/n, ... and columns 0 .. n - 1 (8.6.4.2): M[j][i] = c((2i + 1) * j * 32/n mod 128); row 0 is
    the constant 64"""
    s = 32 // n
    return np.array([[64 if j == 0 else _c((2 * i + 1) * j * s) for i in range(n)] for j in range(n)], dtype=np.int64)


# 8.6.4.2, the DST-VII matrix of the 4x4 luma intra TU (trType = 1)
DST = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], dtype=np.int64)
# 8.6.3: levelScale[qP % 6]
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)
# 8.4.4.2.6, table 8-4: intraPredAngle for predModeIntra 2 .. 34
ANGLE = (32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32)
# 8.4.4.2.6, table 8-5: invAngle for predModeIntra 11 .. 25
INV_ANGLE = (-4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096)
# 8.4.4.2.3, table 8-3: intraHorVerDistThres[nTbS]
DIST_THRES = {8: 7, 16: 1, 32: 0}
assert len(ANGLE) == 33 and len(INV_ANGLE) == 15

_DCT = {n: dct_matrix(n) for n in (4, 8, 16, 32)}


# ------------------------------------------------------------------------------------------------- 8.6.2 - 8.6.4: levels to residual

def coeff_range(bitdepth, epp):
    """CoeffMinY / CoeffMaxY (7.4.3.3.2 with extended_precision_processing_flag; -32768 .. 32767 without)"""
    e = max(15, bitdepth + 6) if epp else 15
    return -(1 << e), (1 << e) - 1


def scale(levels, qp, n, bitdepth=8, epp=0, m=None, rules=SPEC, ranges=None):
    """8.6.3 on [T][n][n] levels: d = Clip3(coeffMin, coeffMax, (level * m * levelScale[qP % 6] << (qP / 6)) + (1 << (bdShift - 1))
    >> bdShift); m = None is the flat 16"""
    R = _rules(rules)
    L = np.asarray(levels).astype(np.int64)
    T = L.shape[0]
    qp = np.broadcast_to(np.asarray(qp, dtype=np.int64), (T,))
    cmin, cmax = coeff_range(bitdepth, epp)
    bd1 = bitdepth + (n.bit_length() - 1) + 10 - (max(15, bitdepth + 6) if epp else 15)
    ls = np.array(LEVEL_SCALE, np.int64)[qp % 6]
    exact = ((L * (16 if m is None else m) * ls[:, None, None]) << (qp // 6)[:, None, None]) + (1 << (bd1 - 1))
    v = _wrap(exact, 32) if "scale_wraps_32" in R else exact
    d = np.clip(v >> bd1, cmin, cmax)
    if "coeffs_int16" in R:
        d = _wrap(d, 16)
    if ranges is not None:
        ranges["product"] = np.abs(exact).reshape(T, -1).max(axis=1)
        ranges["scaled"] = np.abs(exact >> bd1).reshape(T, -1).max(axis=1)
    return d


def transform(d, n, bitdepth=8, epp=0, dst=None, rules=SPEC, ranges=None):
    """8.6.4.2 and the bdShift of 8.6.2 on [T][n][n] scaled coefficients: every column through the one-dimensional transform,
    g = Clip3(coeffMin, coeffMax, (e + 64) >> 7), every row, then (r + (1 << (bdShift - 1))) >> bdShift with
    bdShift = Max(20 - bitDepth, extended_precision_processing_flag ? 11 : 0).  dst: which TUs take the DST (trType = 1), 4x4 only"""
    R = _rules(rules)
    d = np.asarray(d).astype(np.int64)
    T = d.shape[0]
    dst = np.zeros(T, bool) if dst is None else np.broadcast_to(np.asarray(dst, dtype=bool), (T,))
    assert n == 4 or not dst.any()
    cmin, cmax = coeff_range(bitdepth, epp)
    bd2 = max(20 - bitdepth, 11 if epp else 0)
    half2 = 1 << (bd2 - 1)

    assert not d.size or np.abs(d).max() < 1 << 40

    def mat(a, b):      # an integer matrix product through float64, which is exact here: every sum stays far below 2^53
        return np.rint(np.matmul(a.astype(np.float64), b.astype(np.float64))).astype(np.int64)

    def two_pass(M, rnd1, rnd2, clip2):
        e = (mat(M.T, d) + rnd1) >> 7                        # e[y][x] = sum over j of M[j][y] * d[j][x]
        g = np.clip(e, cmin, cmax)
        if "coeffs_int16" in R:
            g = _wrap(g, 16)
        r = (mat(g, M) + rnd2) >> bd2                        # r[y][x] = sum over j of g[y][j] * M[j][x]
        if clip2:
            r = np.clip(r, cmin, cmax)
        if "residual_int16" in R:
            r = _wrap(r, 16)
        return e, r

    e, r = two_pass(_DCT[n], 64, half2, False)
    if dst.any():
        own = "dst_round_is_shift_minus_1" in R
        e2, r2 = two_pass(DST, 6 if own else 64, bd2 - 1 if own else half2, "dst_clips_second_pass" in R)
        e, r = np.where(dst[:, None, None], e2, e), np.where(dst[:, None, None], r2, r)
    if ranges is not None:
        ranges["pass1"] = np.abs(e).reshape(T, -1).max(axis=1)
    return r


def residual(levels, info, n, bitdepth=8, epp=0, scaling=None, rules=SPEC, ranges=None):
    """8.6.2 for a batch of n x n TUs.  ranges: a dict that receives, per TU, the largest magnitudes the unbounded values reached --
    'product' (8.6.3 before its shift), 'scaled' (8.6.3 before its clip), 'pass1' (8.6.4.2 before its clip), 'out' (the residual)
    -- for a test's domain predicate."""
    R = _rules(rules)
    levels, info = np.asarray(levels), np.asarray(info)
    T = levels.shape[0]
    assert n in (4, 8, 16, 32) and levels.shape == (T, n * n) and info.shape == (T, 4)
    lg = n.bit_length() - 1
    L = levels.astype(np.int64).reshape(T, n, n)                    # [tu][y][x]
    qp, fl, mid = info[:, 0].astype(np.int64), info[:, 1].astype(np.int64), info[:, 2].astype(np.int64)
    bypass = (fl & 4) != 0
    ts = ((fl & 2) != 0) & ~bypass
    dst = ((fl & 1) != 0) & ~bypass & ~ts & (n == 4)
    rot = ((fl & 8) != 0)[:, None, None]
    assert n == 4 or not rot.any(), "rotation exists for 4x4 blocks only (8.6.2)"
    flip = lambda a: a[:, ::-1, ::-1]

    # 8.6.3: m = 16 without scaling lists, and for a transform-skipped block above 4x4
    m = np.full((T, n, n), 16, np.int64)
    if scaling is not None:
        sf = np.asarray(scaling).astype(np.int64)[mid].reshape(T, n, n)
        m = np.where((~ts if n > 4 else np.ones(T, bool))[:, None, None], sf, m)
    rg = {} if ranges is not None else None
    d = scale(L, qp, n, bitdepth, epp, m, R, rg)

    # transform skip: 8.6.4.2 (rotation, r = d << tsShift with tsShift = 5 + Log2(nTbS)), then the bdShift of 8.6.2
    bd2 = max(20 - bitdepth, 11 if epp else 0)
    r_ts = np.where(rot, flip(d), d) << (5 + lg)
    if "ts_shift_int16" in R:
        r_ts = _wrap(r_ts, 16)
    if "ts_without_bdshift" not in R:
        r_ts = (r_ts + (1 << (bd2 - 1))) >> bd2

    # bypass: 8.6.2, r = TransCoeffLevel (rotated)
    r_by = np.where(rot, flip(L), L)

    r_tr = transform(d, n, bitdepth, epp, dst, R, rg)
    out = np.where(bypass[:, None, None], r_by, np.where(ts[:, None, None], r_ts, r_tr))
    if ranges is not None:
        ranges["product"] = np.where(bypass, 0, rg["product"])
        ranges["scaled"] = np.where(bypass, 0, rg["scaled"])
        ranges["pass1"] = np.where(~bypass & ~ts, rg["pass1"], 0)
        ranges["out"] = np.abs(out).reshape(T, -1).max(axis=1)
    return out.reshape(T, n * n)


# ------------------------------------------------------------------------------------------------- 8.4.4.2: intra sample prediction
#
# The neighbours of a block live in ONE vector p of 4n + 1 samples in the order of the substitution process (8.4.4.2.2): from
# p[-1][2n - 1] up the left column to p[-1][0], the corner p[-1][-1], then the top row p[0][-1] .. p[2n - 1][-1].
#   left(k) = p[2n - 1 - k]    corner = p[2n]    top(k) = p[2n + 1 + k]

def substitute(p, avail, bitdepth):
    """8.4.4.2.2: nothing available gives 1 << (bitDepth - 1); else the search starts at p[-1][2n - 1], runs up and then right until
    it finds an available sample, which replaces everything before it; then every unavailable sample takes its predecessor"""
    if avail.all():
        return p
    if not avail.any():
        return np.full_like(p, 1 << (bitdepth - 1))
    idx = np.where(avail, np.arange(p.size), 0)
    idx = np.maximum.accumulate(idx)
    idx[:np.argmax(avail)] = np.argmax(avail)
    return p[idx]


def filter_applies(mode, n, flags):
    """8.4.4.2.3: filterFlag.  DC and 4x4 blocks are never filtered; otherwise minDistVerHor > intraHorVerDistThres[nTbS]"""
    if not flags & TU_FILTER or mode == 1 or n == 4:
        return False
    return min(abs(mode - 26), abs(mode - 10)) > DIST_THRES[n]


def filter_neighbours(p, n, cidx, strong, bd_y):
    """8.4.4.2.3: the bi-linear case of a flat 32x32 luma block, else [1 2 1] / 4 along the vector with both ends kept"""
    c, bl, tr = p[2 * n], p[0], p[4 * n]
    if strong and cidx == 0 and n == 32 and abs(c + tr - 2 * p[2 * n + n]) < (1 << (bd_y - 5)) and \
            abs(c + bl - 2 * p[2 * n - n]) < (1 << (bd_y - 5)):
        k = np.arange(1, 64, dtype=np.int64)            # distance from the corner: y + 1 (x + 1) of the clause
        f = p.copy()
        f[2 * n - k] = ((64 - k) * c + k * bl + 32) >> 6
        f[2 * n + k] = ((64 - k) * c + k * tr + 32) >> 6
        return f
    f = p.copy()
    f[1:-1] = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2
    return f


_ANG_CACHE = {}


def _angular_tables(mode, n):
    """index tables of 8.4.4.2.6 for (predModeIntra, nTbS): where in p each ref[x] comes from (x = -n .. 2n, offset n), and per
    (a, b) -- a along the direction of prediction, b across -- the two ref indices and iFact"""
    key = (mode, n)
    if key not in _ANG_CACHE:
        ang = ANGLE[mode - 2]
        vert = mode >= 18
        main = (lambda k: 2 * n + 1 + k) if vert else (lambda k: 2 * n - 1 - k)       # p index of main(k), k >= -1 (k = -1: corner)
        side = (lambda k: 2 * n - 1 - k) if vert else (lambda k: 2 * n + 1 + k)
        src = np.zeros(3 * n + 2, np.int64)                  # ref[x] at src[x + n]; one more for the unused ref[2n + 1] * 0
        for x in range(0, n + 1):
            src[x + n] = main(x - 1)
        if ang < 0:
            last = (n * ang) >> 5
            if last < -1:
                inv = INV_ANGLE[mode - 11]
                for x in range(last, 0):
                    src[x + n] = side(-1 + ((x * inv + 128) >> 8))
        else:
            for x in range(n + 1, 2 * n + 1):
                src[x + n] = main(x - 1)
        a = np.arange(n, dtype=np.int64)[:, None]
        b = np.arange(n, dtype=np.int64)[None, :]
        i_idx, i_fact = ((a + 1) * ang) >> 5, ((a + 1) * ang) & 31
        _ANG_CACHE[key] = (src, b + i_idx + 1 + n, i_fact + 0 * b, vert)
    return _ANG_CACHE[key]


def predict(mode, p, n, cidx, flags, bd_y):
    """8.4.4.2.4 (planar), 8.4.4.2.5 (DC), 8.4.4.2.6 (angular) from the neighbour vector; returns [y][x]"""
    lg = n.bit_length() - 1
    left, corner, top = p[2 * n - 1::-1], p[2 * n], p[2 * n + 1:]            # left[k] = p[-1][k], top[k] = p[k][-1]
    x = np.arange(n, dtype=np.int64)[None, :]
    y = np.arange(n, dtype=np.int64)[:, None]
    if mode == 0:
        return ((n - 1 - x) * left[:n, None] + (x + 1) * top[n] + (n - 1 - y) * top[None, :n] + (y + 1) * left[n] + n) >> (lg + 1)
    if mode == 1:
        dc = (top[:n].sum() + left[:n].sum() + n) >> (lg + 1)
        out = np.full((n, n), dc, np.int64)
        if cidx == 0 and n < 32 and not flags & TU_NO_DC_BF:
            out[0, :] = (top[:n] + 3 * dc + 2) >> 2
            out[:, 0] = (left[:n] + 3 * dc + 2) >> 2
            out[0, 0] = (left[0] + 2 * dc + top[0] + 2) >> 2
        return out
    src, i0, fact, vert = _angular_tables(mode, n)
    ref = p[src]
    out = ((32 - fact) * ref[i0] + fact * ref[i0 + 1] + 16) >> 5             # iFact = 0 gives ref[i0] exactly: (32 ref + 16) >> 5
    if not vert:
        out = out.T
    if cidx == 0 and n < 32 and not flags & TU_NO_BF:
        hi = (1 << bd_y) - 1
        if mode == 26:
            out = out.copy()
            out[:, 0] = np.clip(top[0] + ((left[:n] - corner) >> 1), 0, hi)
        if mode == 10:
            out = out.copy()
            out[0, :] = np.clip(left[0] + ((top[:n] - corner) >> 1), 0, hi)
    return out


def gather(plane, x0, y0, n, at, al, corner):
    """the neighbour vector of the block at (x0, y0) and which of its samples are available"""
    k = np.arange(2 * n, dtype=np.int64)
    h, w = plane.shape
    bits = np.unpackbits(np.array([at, al], dtype="<u8").view(np.uint8).reshape(2, 8), axis=1, bitorder="little").astype(bool)
    a_top, a_left = bits[0, :2 * n], bits[1, :2 * n]
    p = np.zeros(4 * n + 1, np.int64)
    avail = np.zeros(4 * n + 1, bool)
    avail[2 * n - 1::-1] = a_left
    avail[2 * n] = corner
    avail[2 * n + 1:] = a_top
    assert not a_top.any() or y0 > 0
    assert not a_left.any() or x0 > 0
    p[2 * n - 1::-1] = plane[np.minimum(y0 + k, h - 1), x0 - 1]
    p[2 * n] = plane[y0 - 1, x0 - 1]
    p[2 * n + 1:] = plane[y0 - 1, np.minimum(x0 + k, w - 1)]
    assert (y0 + k[a_left] < h).all() and (x0 + k[a_top] < w).all(), "an available sample outside the picture"
    return np.where(avail, p, 0), avail


def residual_of_tu(t, flat, bd_y, bd_c, luma_res, R):
    """the residual a TU adds: 8.6.5 (rdpcm) and 8.6.6 (cross-component prediction) on the block of `flat` at res_offset"""
    n = 1 << int(t["log2_size"])
    flags, mode = int(t["flags"]), int(t["pred_mode"])
    if not flags & TU_RESIDUAL:
        return np.zeros((n, n), np.int64)
    o = int(t["res_offset"])
    r = flat[o:o + n * n].astype(np.int64).reshape(n, n)
    if flags & TU_RDPCM:
        assert mode in (10, 26), "intra rdpcm follows predModeIntra 10 or 26 (8.6.2)"
        if mode == 26:
            r = np.cumsum(r, axis=0)
        elif "rdpcm_horizontal_runs_on" in R:
            f = r.reshape(-1).copy()
            f[n - 1:] = np.cumsum(f[n - 1:])
            r = f.reshape(n, n)
        else:
            r = np.cumsum(r, axis=1)
        if "resmod_int16" in R:
            r = _wrap(r, 16)
    if flags & TU_CCP:
        if "ccp_reads_chroma" in R:
            ry = r
        else:
            ry = luma_res.get((int(t["x"]), int(t["y"]), n))
            ry = np.zeros((n, n), np.int64) if ry is None else ry
        r = r + ((int(t["res_scale"]) * ((ry << bd_c) >> bd_y)) >> 3)
        if "resmod_int16" in R:
            r = _wrap(r, 16)
    return r


def intra(tus, residual, width, height, chroma=True, bd_y=8, bd_c=8, csub=2, rules=SPEC, forced=None):
    """the TU list, in order: gather, substitute, filter, predict, add the residual, clip (8.4.4.2.1 - 8.4.4.2.6, 8.6.5 - 8.6.7).
    forced: planes of another decode of the same list; every TU then takes its neighbouring samples from THOSE, so that two
    decodes can be compared TU by TU without one differing TU reaching every TU after it"""
    R = _rules(rules)
    assert 8 <= bd_y <= 15 and 8 <= bd_c <= 15
    tus = np.asarray(tus)
    flat = np.asarray(residual)
    planes = [np.zeros((height, width), np.int64)]
    if chroma:
        planes += [np.zeros((height // csub, width // csub), np.int64) for _ in range(2)]
    luma_res = {}
    for t in tus:
        c, n, mode, flags = int(t["cidx"]), 1 << int(t["log2_size"]), int(t["pred_mode"]), int(t["flags"])
        x0, y0 = int(t["x"]), int(t["y"])
        P, bd = planes[c], (bd_y if c == 0 else bd_c)
        assert 0 <= mode <= 34 and x0 + n <= P.shape[1] and y0 + n <= P.shape[0]
        p, avail = gather(P if forced is None else forced[c], x0, y0, n, t["avail_top"], t["avail_left"], bool(flags & TU_CORNER))
        p = substitute(p, avail, bd)
        if filter_applies(mode, n, flags):
            p = filter_neighbours(p, n, c, bool(flags & TU_STRONG), bd_y)
        pred = predict(mode, p, n, c, flags, bd_y)
        r = residual_of_tu(t, flat, bd_y, bd_c, luma_res, R)
        if c == 0 and flags & TU_RESIDUAL:
            luma_res[(x0, y0, n)] = r
        P[y0:y0 + n, x0:x0 + n] = np.clip(pred + r, 0, (1 << bd) - 1)
    out = [pl.astype(np.int16) for pl in planes]
    return (out[0], out[1], out[2]) if chroma else (out[0], None, None)
