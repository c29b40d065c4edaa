"""Cases for the HEVC spec witness (tests/hevc_spec.py), shared by tests/test_hevc_spec.py (CPU) and tests/test_hevc_spec_gpu.py:
level batches, pictures made of cells, whole TU lists with a real residual chain, and the predicates that say which TUs lie in
the conformant domain and which a named rule touches.  Nothing here imports the oracle."""
import numpy as np

import hevc_spec as S
from ffpic_amd import synth

# flags of a level batch, cycled: mostly plain TUs, so that at least three quarters of a batch stay clear of the named rules
FLAG_CYCLE_4 = [0] * 6 + [4, 0, 0, 1, 0, 0, 2, 0, 4 | 8, 0, 2 | 8, 0, 0]
FLAG_CYCLE_N = [0] * 6 + [4, 0, 0, 0, 0, 0, 2, 0, 4, 0, 2, 0, 0]


def coefficient_positions(n):
    """(x, y) of the single-coefficient blocks: everywhere up to 8x8; rows and columns 0, 1 and n - 1 plus the diagonal above"""
    if n <= 8:
        return [(x, y) for y in range(n) for x in range(n)]
    edge = (0, 1, n - 1)
    return [(x, y) for y in range(n) for x in range(n) if x in edge or y in edge or x == y]


def largest_level(n, bitdepth, qp, m=16):
    """the largest level whose scaled coefficient (8.6.3) is still below the clip at coeffMax = 32767"""
    bd1 = bitdepth + n.bit_length() - 1 - 5
    f = (m * S.LEVEL_SCALE[qp % 6]) << (qp // 6)
    lv = min(32767, ((32768 << bd1) - (1 << (bd1 - 1)) - 1) // f)
    assert ((lv * f + (1 << (bd1 - 1))) >> bd1) <= 32767 and lv >= 1
    return lv


def residual_batch(n, bitdepth, seed=0, n_random=None):
    """One batch for ffhip_hevc_residual_batch: (levels [T][n*n] int16, info [T][4] uint8, scaling [6][n*n] uint8).
    Every single-coefficient block of coefficient_positions(n) at 1, -1 and the largest in-range level (flat scaling, qP 26; for n = 4
    once through the DCT and once through the DST), then Laplace-distributed levels of an encoder's size with qP 0 .. 51 in turn,
    the flags of FLAG_CYCLE_*, scaling row 0 flat (all 16) and rows 1 .. 5 lists; every 23rd of those TUs holds full-range levels."""
    rng = np.random.default_rng(0x4EFC + 97 * n + bitdepth + 1000 * seed)
    pos = coefficient_positions(n)
    top = largest_level(n, bitdepth, 26)
    lv, info = [], []
    for flag in ((0, 1) if n == 4 else (0,)):
        for (x, y) in pos:
            for amp in (1, -1, top):
                b = np.zeros(n * n, np.int16)
                b[x + y * n] = amp
                lv.append(b)
                info.append((26, flag, 0, 0))
    n_random = (312 if n <= 8 else 104) if n_random is None else n_random
    scaling = np.full((6, n * n), 16, np.uint8)
    scaling[1:] = rng.integers(8, 64, size=(5, n * n))
    cyc = FLAG_CYCLE_4 if n == 4 else FLAG_CYCLE_N
    yy, xx = np.mgrid[0:n, 0:n]
    decay = np.exp(-(xx + yy) / (n / 2.0)).reshape(-1)
    for i in range(n_random):
        qp, flag, mid = i % 52, cyc[i % len(cyc)], i % 6
        bd1 = bitdepth + n.bit_length() - 1 - 5
        step = ((32 * S.LEVEL_SCALE[qp % 6]) << (qp // 6)) / float(1 << bd1)              # coefficient per level at m = 32
        amp = 1500.0 / step                       # coefficients fill 16 bits at every bit depth: the residual grows with it
        if flag & 4:
            b = np.rint(rng.laplace(0, 20, size=n * n))                                    # bypass: the levels ARE the residual
        elif flag & 2:                                          # transform skip: a low qP and small levels keep d << tsShift inside 16 bits
            qp = i % 12
            step = ((32 * S.LEVEL_SCALE[qp % 6]) << (qp // 6)) / float(1 << bd1)
            dmax = 0.45 * (1 << (11 - n.bit_length()))            # under half of what tsShift leaves, for lists of up to 63
            b = np.trunc(rng.uniform(-dmax, dmax, size=n * n) / step)
        else:
            b = np.rint(rng.laplace(0, 1.0, size=n * n) * amp * decay)
        if i % 23 == 22:
            b = rng.integers(-32768, 32768, size=n * n)
        lv.append(np.clip(b, -32768, 32767).astype(np.int16))
        info.append((qp, flag, mid, 0))
    return np.stack(lv), np.array(info, np.uint8), scaling


def residual_touched(info, n):
    """TUs a named rule of the residual stage touches: the DST (dst_round_is_shift_minus_1) and transform skip (ts_without_bdshift)"""
    fl = info[:, 1]
    bypass = (fl & 4) != 0
    ts = ((fl & 2) != 0) & ~bypass
    return ts | (((fl & 1) != 0) & ~bypass & ~ts & (n == 4))


def residual_conformant(levels, info, n, bitdepth, scaling=None):
    """The conformant domain of the residual stage, TU by TU: the scaling product fits 32 bits, the scaled coefficients stay inside
    the clip, and every intermediate -- first pass, residual, for transform skip the shifted value -- stays inside 16 bits.
    The magnitudes come from the witness under SPEC, where nothing wraps."""
    rg = {}
    S.residual(levels, info, n, bitdepth, 0, scaling, S.SPEC, rg)
    ok = (rg["product"] < (1 << 31)) & (rg["scaled"] <= 32767) & (rg["pass1"] <= 32767) & (rg["out"] <= 32767)
    ts = ((info[:, 1] & 2) != 0) & ((info[:, 1] & 4) == 0)
    return ok & ~(ts & ((rg["scaled"] << (5 + n.bit_length() - 1)) > 32767))


# ------------------------------------------------------------------------------------------------- pictures made of cells

CELL = 128                                     # a cell is 2 x 2 coding tree blocks of 64; the TU under test sits at (64, 64) of it
PATTERNS = ("everything", "nothing", "top row only", "left column only", "corner only", "no below-left", "no above-right")


def _pattern_masks(pattern, n):
    full, half = (1 << (2 * n)) - 1, (1 << n) - 1
    return {"everything": (full, full, True), "nothing": (0, 0, False), "top row only": (full, 0, False),
            "left column only": (0, full, False), "corner only": (0, 0, True), "no below-left": (full, half, True),
            "no above-right": (half, full, True)}[pattern]


def intra_cells(n, bitdepth, pattern, seed=0):
    """One luma picture of 10 x 7 cells, a cell per (mode 0 .. 34) x (plain, TU_FILTER | TU_STRONG).  In a cell five DC-mode TUs of
    size n with nothing available and a random in-range residual form the ring -- above-left, above, above-right, left, below-left
    of (64, 64), each in a coding tree block that is decoded before the fourth -- then comes the TU under test at (64, 64) with the
    availability of `pattern`.  For n = 32 every third cell has a ring that is a gentle ramp, so the bi-linear filter of 8.4.4.2.3
    runs on one side of its threshold and [1 2 1] on the other.  Returns (tus, residual, width, height, index of the TU under test
    per cell)."""
    rng = np.random.default_rng(0x1C11 + 131 * n + bitdepth + 7 * PATTERNS.index(pattern) + 1000 * seed)
    lg, half = n.bit_length() - 1, 1 << (bitdepth - 1)
    at, al, corner = _pattern_masks(pattern, n)
    recs, parts, off = [], [], 0
    cells = [(mode, fl) for fl in (0, synth.TU_FILTER | synth.TU_STRONG) for mode in range(35)]
    for k, (mode, fl) in enumerate(cells):
        cx, cy = (k % 10) * CELL, (k // 10) * CELL
        ramp = n == 32 and k % 3 == 0
        for (dx, dy) in ((-n, -n), (0, -n), (n, -n), (-n, 0), (-n, n)):
            x0, y0 = cx + 64 + dx, cy + 64 + dy
            if ramp:
                yy, xx = np.mgrid[0:n, 0:n]
                r = ((xx + dx + 2 * (yy + dy)) >> 3) + int(rng.integers(-1, 2))
            else:
                r = rng.integers(-half + half // 8, half - half // 8, size=(n, n))
            recs.append((x0, y0, lg, 0, 1, synth.TU_RESIDUAL, off, 0, 0, 0))
            parts.append(r.reshape(-1))
            off += n * n
        r = np.rint(rng.laplace(0, half / 8.0, size=n * n))
        recs.append((cx + 64, cy + 64, lg, 0, mode, fl | synth.TU_RESIDUAL | (synth.TU_CORNER if corner else 0), off, 0, at, al))
        parts.append(r)
        off += n * n
    tus = np.array(recs, dtype=synth.HEVC_TU_DTYPE)
    # decode order: coding tree blocks in raster order; inside one of them at most two TUs, side by side or one above the other
    order = np.lexsort((tus["x"], tus["y"], tus["x"] // 64, tus["y"] // 64))
    tus = tus[order]
    under_test = np.nonzero(np.isin(order, np.arange(5, len(recs), 6)))[0]
    return tus, np.concatenate(parts).astype(np.int16), 10 * CELL, 7 * CELL, under_test


# ------------------------------------------------------------------------------------------------- whole lists, real residual chain

WHOLE_LISTS = {"64x64 4:2:0": dict(width=64, height=64, seed=41),
               "96x64 ctb 32": dict(width=96, height=64, seed=42, ctb=32),
               "64x64 4:4:4 ccp": dict(width=64, height=64, seed=43, ccp=True, chroma_444=True)}


def whole_list(name, bitdepth=8):
    """A picture of synth.hevc_intra_tus whose residuals come from LEVELS: returns (tus, width, height, csub, per TU size n a tuple
    (indices of the TUs, levels, info)).  Luma 4x4 TUs take the DST, about a tenth of the others transform skip or bypass."""
    kw = dict(WHOLE_LISTS[name])
    w, h = kw.pop("width"), kw.pop("height")
    tus, _ = synth.hevc_intra_tus(w, h, **kw)
    rng = np.random.default_rng(0xC4A1 + kw["seed"] + bitdepth)
    by_size = {}
    has = (tus["flags"] & synth.TU_RESIDUAL) != 0
    for n in (4, 8, 16, 32):
        idx = np.nonzero(has & (tus["log2_size"] == n.bit_length() - 1))[0]
        if not idx.size:
            continue
        qp = rng.integers(20, 40, size=idx.size)
        bd1 = bitdepth + n.bit_length() - 1 - 5
        step = ((16 * np.array(S.LEVEL_SCALE)[qp % 6]) << (qp // 6)) / float(1 << bd1)
        yy, xx = np.mgrid[0:n, 0:n]
        decay = np.exp(-(xx + yy) / (n / 2.0)).reshape(-1)
        lv = np.rint(rng.laplace(0, 1.0, size=(idx.size, n * n)) * decay * (1200.0 / step)[:, None])
        flags = np.where((tus["cidx"][idx] == 0) & (n == 4), 1, 0) | rng.choice([0] * 18 + [2, 4], size=idx.size)
        ts = (flags & 2) != 0                                       # transform skip: d << tsShift has to stay inside 16 bits
        dmax = 0.9 * (1 << (11 - n.bit_length()))
        lv[ts] = np.trunc(rng.uniform(-dmax, dmax, size=(int(ts.sum()), n * n)) / step[ts][:, None])
        info = np.zeros((idx.size, 4), np.uint8)
        info[:, 0], info[:, 1] = qp, flags
        by_size[n] = (idx, lv.astype(np.int16), info)
    return tus, w, h, (1 if kw.get("chroma_444") else 2), by_size


def scatter_residual(tus, by_size, blocks):
    """the flat residual array of a TU list from per-size blocks (blocks[n][k] belongs to TU by_size[n][0][k])"""
    has = (tus["flags"] & synth.TU_RESIDUAL) != 0
    size = int((tus["res_offset"].astype(np.int64) + (1 << (2 * tus["log2_size"].astype(np.int64))))[has].max()) if has.any() else 1
    flat = np.zeros(size, np.int64)
    for n, (idx, _, _) in by_size.items():
        for k, i in enumerate(idx):
            o = int(tus["res_offset"][i])
            flat[o:o + n * n] = blocks[n][k]
    return flat


# ------------------------------------------------------------------------------------------------- which TUs a named rule reaches

def intra_touched(tus):
    """TUs a named rule of the intra stage touches directly: horizontal rdpcm (rdpcm_horizontal_runs_on) and cross-component
    prediction (ccp_reads_chroma)"""
    fl = tus["flags"]
    res = (fl & synth.TU_RESIDUAL) != 0
    return res & ((((fl & synth.TU_RDPCM) != 0) & (tus["pred_mode"] < 26)) | ((fl & synth.TU_CCP) != 0))


def intra_reached(tus, width, height, chroma, csub, direct):
    """the closure of `direct` under prediction: a TU is reached when a named rule touches it or when an AVAILABLE neighbouring
    sample it reads lies in a TU that is reached (an unavailable sample is replaced from available ones, 8.4.4.2.2)"""
    masks = [np.zeros((height, width), bool)] + ([np.zeros((height // csub, width // csub), bool) for _ in range(2)] if chroma else [])
    out = np.zeros(len(tus), bool)
    for i, t in enumerate(tus):
        n, x0, y0, M = 1 << int(t["log2_size"]), int(t["x"]), int(t["y"]), masks[int(t["cidx"])]
        hit = bool(direct[i])
        if not hit:
            bits = np.unpackbits(np.array([t["avail_top"], t["avail_left"]], dtype="<u8").view(np.uint8).reshape(2, 8), axis=1,
                                 bitorder="little").astype(bool)[:, :2 * n]
            k = np.arange(2 * n)
            kt, kl = k[bits[0]], k[bits[1]]
            hit = bool((kt.size and M[y0 - 1, x0 + kt].any()) or (kl.size and M[y0 + kl, x0 - 1].any()) or
                       (int(t["flags"]) & synth.TU_CORNER and M[y0 - 1, x0 - 1]))
        out[i] = hit
        M[y0:y0 + n, x0:x0 + n] = hit
    return out


def tu_differs(tus, planes_a, planes_b):
    """per TU: do two plane sets differ inside it?  Valid where no later TU overwrites an earlier one (every list here)"""
    out = np.zeros(len(tus), bool)
    for i, t in enumerate(tus):
        n, x0, y0, c = 1 << int(t["log2_size"]), int(t["x"]), int(t["y"]), int(t["cidx"])
        out[i] = not np.array_equal(planes_a[c][y0:y0 + n, x0:x0 + n], planes_b[c][y0:y0 + n, x0:x0 + n])
    return out


def describe(tus, i):
    t = tus[i]
    return "plane %s, TU %d, mode %d, size %d at (%d, %d), flags 0x%02x" % ("YUV"[int(t["cidx"])], i, int(t["pred_mode"]),
                                                                            1 << int(t["log2_size"]), int(t["x"]), int(t["y"]), int(t["flags"]))
