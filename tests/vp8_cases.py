"""VP8 key frames WRITTEN from known modes, segment ids, skip flags and levels (tests/vp8_writer.keyframe_from), for the tests that pin the
library's two bool-decoder front ends -- the host parser and the two device kernels -- on the answer instead of on each other: a front
end is right when it returns exactly what went in.  Plain Python, seeded.

case(name, seed) -> Case(data, modes, levels, mbinfo, resmap, facts): the file, the arrays in the layout ops.webp_parse returns them
(modes [n][20], levels [n][25][16] as a decoder must return them -- cat6 extra bits wrapped --, mbinfo [n][27]: 25 token counts, "has a
Y2 block", segment id; resmap [n]) and a dict of facts: what the stream visits (coefficient-probability slots with the bit taken, 4x4
mode triples, tokens, positions), the bytes of every partition, `written` (the levels as written, cat6 unwrapped), `ref_ok` (the
reference's loader can take the file: at most 4 partitions, a height that is a multiple of 16, no skipped macroblock in front of every
coded one), `refused` (a twin with one partition a byte short: every front end must answer FFHIP_EINVAL) and the header arguments.

What each case is there for is said next to it in CASES; test_vp8_known_tokens.py asserts it from `facts`.  No frame is larger than
16 x 16 macroblocks: one GPU lane decodes a frame, at some 45 us a macroblock."""
import collections
import functools

import numpy as np

import vp8_writer as W

Case = collections.namedtuple("Case", "data modes levels mbinfo resmap facts")

SEG0 = dict(update_map=0, feature_mode=1, quant=(1, 0, 0, 0))     # segmentation on, the map kept: no ids coded, segment 0 has quantisers
LADDER = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 34, 35, 66, 67, 67 + 255, 67 + 256, 67 + 2047)
LADDER_POSITIONS = (0, 1, 14, 15)
SLOT_VALUES = (0, 1, 2, 3, 4, 5, 7, 11, 19, 35, 67)               # with the end of block: every node of the token tree with both bits
N_REACHABLE_SLOTS = 996


def reachable_slots():
    """The (type, band, context, node) slots of the coefficient probabilities a legal stream can read, from the grammar: a block of
    type 0 starts at position 1, the others at 0; the first position has the context of the neighbours (0, 1, 2), a later one that of
    the token in front (0 zero, 1 one, 2 larger); node 0 (end of block) is not read behind a zero.  So type 0 never sees band 0, and
    node 0 in context 0 exists only at a block's first position."""
    out = set()
    for t in range(4):
        first = 1 if t == 0 else 0
        states = {(first, c, False) for c in range(3)}
        while states:
            n, ctx, prev_zero = states.pop()
            for node in range(0 if not prev_zero else 1, 11):
                out.add((t, W.BANDS[n], ctx, node))
            if n < 15:
                states |= {(n + 1, 0, True), (n + 1, 1, False), (n + 1, 2, False)}
    return out


def _empty(n):
    return dict(ymode=np.zeros(n, np.int64), bmodes=np.zeros((n, 16), np.int64), uvmode=np.zeros(n, np.int64), seg=np.zeros(n, np.int64),
                skip=np.zeros(n, bool), levels=np.zeros((n, 25, 16), np.int64))


def _legal(m):
    """levels a stream cannot carry are cleared: position 0 of a Y block behind a Y2 block, the Y2 block of B_PRED, skipped macroblocks"""
    lv, ym = m["levels"], m["ymode"]
    lv[ym != 4, :16, 0] = 0
    lv[ym == 4, 24] = 0
    lv[m["skip"]] = 0
    return m


def _random_levels(rng, n, dense=0.5):
    mag = np.minimum(rng.geometric(0.25, (n, 25, 16)), 60) * (rng.random((n, 25, 16)) < dense)
    big = rng.random((n, 25, 16)) < 0.02
    mag = np.where(big, rng.integers(11, 67 + 2048, (n, 25, 16)), mag)
    ntok = rng.integers(0, 17, (n, 25, 1))                          # raster positions kept; which tokens that makes is up to the zigzag
    mag = np.where(np.argsort(np.argsort(rng.random((n, 25, 16)), axis=2), axis=2) < ntok, mag, 0)
    mag[rng.random((n, 25)) < 0.3] = 0
    return mag * (rng.integers(0, 2, (n, 25, 16)) * 2 - 1)


def _random_mbs(rng, n, bpred=0.4, skip_p=0.0, segs=False):
    m = _empty(n)
    m["ymode"] = np.where(rng.random(n) < bpred, 4, rng.integers(0, 4, n))
    m["bmodes"] = rng.integers(0, 10, (n, 16))
    m["uvmode"] = rng.integers(0, 4, n)
    if segs:
        m["seg"] = rng.integers(0, 4, n)
    m["skip"] = rng.random(n) < skip_p
    m["levels"] = _random_levels(rng, n)
    return _legal(m)


def _probs(rng):
    return [int(v) for v in rng.integers(1, 256, 1056)]


# ---------------------------------------------------------------------------------------------------- the builders: -> (width, height, mbs, zeros16, header)
def _contexts(cols):
    return [[0] * 9 for _ in range(cols)]


def _all_slots(rng):
    """greedy: block after block in decoding order, the token at every position chosen to visit the most (slot, bit) pairs not visited yet;
    drawn again (same generator, so still a function of the seed) should a frame end with pairs left over"""
    for _ in range(10):
        out, left_over = _all_slots_once(rng)
        if not left_over:
            return out
    raise AssertionError("all_slots: no complete frame")


def _all_slots_once(rng):
    cols = rows = 12
    n = cols * rows
    m = _empty(n)
    m["ymode"] = np.where(np.arange(n) % 4 == 3, 4, rng.integers(0, 4, n))
    m["bmodes"] = rng.integers(0, 10, (n, 16))
    m["uvmode"] = rng.integers(0, 4, n)
    z16 = np.zeros((n, 25), bool)
    need = {s + (b,) for s in reachable_slots() for b in (0, 1)}
    left_at = collections.Counter(s[:3] for s in need)      # pairs left per (type, band, context)

    def visits(t, band, ctx, prev_zero, v):
        path = [] if prev_zero else [(0, 0 if v is None else 1)]
        if v is not None:
            path += W.token_path(v)[0]
        return {(t, band, ctx, node, bit) for node, bit in path}

    def block(t, first, ctx):
        seq, prev_zero = [], False
        empty = rng.random() < 0.35
        for pos in range(first, 16):
            band = W.BANDS[pos]
            opts = [v for v in SLOT_VALUES] + ([] if prev_zero else [None])
            gains = [len(visits(t, band, ctx, prev_zero, v) & need) + rng.random() * 0.5 for v in opts]
            v = opts[int(np.argmax(gains))]
            if pos == first and empty:
                v = None
            elif max(gains) < 1:
                # nothing new here: go on towards a later position that has something left, in the context the next one wants
                later = any(left_at[(t, W.BANDS[q], c)] for q in range(pos + 1, 16) for c in range(3))
                nxt = [c for c in range(3) if pos < 15 and left_at[(t, W.BANDS[pos + 1], c)]]
                v = (0, 1, 2)[nxt[0]] if nxt else 1 if prev_zero or later else None
            for s in visits(t, band, ctx, prev_zero, v) & need:
                need.discard(s)
                left_at[s[:3]] -= 1
            if v is None:
                return seq, False
            seq.append(v)
            prev_zero, ctx = v == 0, 0 if v == 0 else 1 if v == 1 else 2
        return seq, seq[-1] == 0

    def put(mb, b, t, first, ctx):
        seq, no_eob = block(t, first, ctx)
        for k, v in enumerate(seq):
            if v >= 67:
                v += int(rng.integers(0, 2048))
            m["levels"][mb, b, W.ZIGZAG[first + k]] = v * int(rng.integers(0, 2) * 2 - 1)
        z16[mb, b] = no_eob
        return int(len(seq) > 0)

    top9 = _contexts(cols)
    for mb in range(n):
        top, left = top9[mb % cols], ([0] * 9 if mb % cols == 0 else left)
        first, ytype = 0, 3
        if m["ymode"][mb] != 4:
            top[0] = left[0] = put(mb, 24, 1, 0, top[0] + left[0])
            first, ytype = 1, 0
        for b in range(16):
            top[1 + b % 4] = left[1 + b // 4] = put(mb, b, ytype, first, top[1 + b % 4] + left[1 + b // 4])
        for b in range(16, 24):
            ch, k = (5, b - 16) if b < 20 else (7, b - 20)
            top[ch + k % 2] = left[ch + k // 2] = put(mb, b, 2, 0, top[ch + k % 2] + left[ch + k // 2])
    return (16 * cols, 16 * rows, m, z16, dict(coeff_probs=_probs(rng), segmentation=SEG0, y_ac_qi=0)), need


def _token_ladder(rng):
    """block k of a type holds LADDER value k at position 0, k + 10 at 1, k + 20 at 14 and k + 30 at 15 (of the 40 signed values): 40
    blocks of every type put every value at every position; macroblock 47 holds a block of 16 non-zero tokens of every type it has,
    macroblock 48 explicit-zero blocks (count 16, no level)"""
    cols = rows = 7
    n = cols * rows
    m = _empty(n)
    m["ymode"] = np.array([4 if mb in (40, 41, 42, 46) else mb % 4 for mb in range(n)])
    m["bmodes"] = rng.integers(0, 10, (n, 16))
    m["uvmode"] = rng.integers(0, 4, n)
    signed = [s * v for v in LADDER for s in (1, -1)]

    def fill(mb, b, k, first):
        for j, pos in enumerate(LADDER_POSITIONS):
            if pos >= first:
                m["levels"][mb, b, W.ZIGZAG[pos]] = signed[(k + 10 * j) % 40]
    for k in range(40):
        fill(k, 24, k, 0)                              # Y2: macroblocks 0..39
        fill(k, k % 16, k, 1)                          # Y behind a Y2
        fill(k // 8, 16 + k % 8, k, 0)                 # chroma: macroblocks 0..4
        fill(40 + k // 16, k % 16, k, 0)               # Y of B_PRED: macroblocks 40..42
    full = rng.integers(1, 5, (25, 16)) * (rng.integers(0, 2, (25, 16)) * 2 - 1)
    m["levels"][46], m["levels"][47] = full, full
    z16 = np.zeros((n, 25), bool)
    z16[48] = z16[45] = True
    z16[45, 24] = False
    m["ymode"][45] = 4                                 # explicit zeros in a B_PRED macroblock too (Y from position 0)
    return 16 * cols, 16 * rows, _legal(m), z16, dict(segmentation=SEG0, y_ac_qi=0)


def _extreme_probs(rng):
    """probabilities 0, 1 and 255 (and 128) dealt over all slots; random levels take the improbable branch of each many times"""
    m = _random_mbs(rng, 16)
    probs = [int(v) for v in rng.choice([0, 1, 255, 128], 1056)]
    return 64, 64, m, None, dict(coeff_probs=probs, segmentation=SEG0, y_ac_qi=10)


def _every_bmode_context(rng):
    """greedy: the 4x4 mode of every subblock chosen, in decoding order, to make an (above, left, mode) triple not seen yet; a 16x16
    macroblock of each y mode now and then, for the contexts it stands for"""
    cols = rows = 16
    n = cols * rows
    m = _empty(n)
    m["ymode"][:] = 4
    for k, mb in enumerate(range(5, n, 11)):
        m["ymode"][mb] = k % 4
    m["uvmode"] = rng.integers(0, 4, n)
    need = {(a, l, b) for a in range(10) for l in range(10) for b in range(10)}
    left_pair, left_above = collections.Counter(s[:2] for s in need), collections.Counter(s[0] for s in need)   # triples left per context
    bottom = [[0] * 4 for _ in range(cols)]
    for mb in range(n):
        x = mb % cols
        if x == 0:
            right = [0] * 4
        ym = int(m["ymode"][mb])
        if ym != 4:
            bottom[x], right = [ym] * 4, [ym] * 4
            continue
        im = [0] * 16
        for i in range(16):
            a = bottom[x][i] if i < 4 else im[i - 4]
            l = right[i >> 2] if (i & 3) == 0 else im[i - 1]
            # a mode that completes a triple here, and among those one that is wanted most as somebody's neighbour
            a2 = None if (i & 3) == 3 else bottom[x][i + 1] if i < 3 else im[i - 3]       # the next subblock's `above`: its `left` is chosen here
            want = [(1000 if (a, l, b) in need else 0) + (100 * left_pair[(a2, b)] if a2 is not None else 0) + left_above[b] + rng.random()
                    for b in range(10)]
            im[i] = int(np.argmax(want))
            if (a, l, im[i]) in need:
                need.discard((a, l, im[i]))
                left_pair[(a, l)] -= 1
                left_above[a] -= 1
        m["bmodes"][mb] = im
        bottom[x], right = im[12:16], [im[3], im[7], im[11], im[15]]
    m["levels"] = _random_levels(rng, n, dense=0.1)
    return 16 * cols, 16 * rows, _legal(m), None, dict(segmentation=SEG0, y_ac_qi=30, level=8)


Y2_PATTERN = ("A", "skipped_bpred", "C", "A", "skipped_i16", "C", "A", "coded_bpred", "C")


def _y2_context(rng):
    """row 0 and column 0 carry Y2_PATTERN: A and C coded 16x16 macroblocks, A with a non-zero Y2 block; between them a skipped B_PRED
    (the Y2 flag is kept: C sees context 1), a skipped 16x16 (cleared: 0), a coded B_PRED (untouched: 1).  The luma blocks of A are
    empty, so that the luma flags say the opposite of the Y2 flag.  The Y2 probabilities of band 0 differ widely between the contexts."""
    cols = rows = 10
    n = cols * rows
    m = _random_mbs(rng, n, bpred=0.3, skip_p=0.15)
    m["ymode"][m["ymode"] == 4] = np.where(rng.random((m["ymode"] == 4).sum()) < 0.5, 4, 0)
    line = [(0, k) for k in range(9)] + [(k, 0) for k in range(1, 9)]
    for y, x in line:
        mb, kind = y * cols + x, Y2_PATTERN[max(x, y)]
        m["skip"][mb] = kind.startswith("skipped")
        m["ymode"][mb] = 4 if kind.endswith("bpred") else 1 + (x + y) % 3
        if kind == "A":
            m["levels"][mb] = 0
            m["levels"][mb, 24, 0], m["levels"][mb, 24, 5] = 3, -1
            m["levels"][mb, 16:24, 0] = 2
        elif kind == "C":
            m["levels"][mb, 24, :4] = (1, -2, 0, 7)
        elif kind == "coded_bpred":
            m["levels"][mb, :16, 0] = 1
    # row 1 / column 1 next to the pattern stay out of its way: the line's macroblocks have the frame edge on their other side
    probs = {}
    for ctx, vals in enumerate(((250, 10, 200), (5, 240, 30), (128, 60, 250))):
        for node, v in enumerate(vals):
            probs[264 + ctx * 11 + node] = v
    return 16 * cols, 16 * rows, _legal(m), None, dict(coeff_probs=probs, prob_skip=180, segmentation=SEG0, y_ac_qi=20)


def _skips(rng, first_skipped=True, every=False):
    """5 x 4: the first macroblock skipped, row 2 skipped whole, the last macroblock of row 0 and the first of row 1 skipped"""
    m = _random_mbs(rng, 20, skip_p=0.1)
    m["skip"][[4, 5, 10, 11, 12, 13, 14]] = True
    m["skip"][0] = first_skipped
    m["skip"][1] = False
    if every:
        m["skip"][:] = True
    return 80, 64, _legal(m), None, dict(prob_skip=120, segmentation=SEG0, y_ac_qi=35, level=16)


def _segments(rng, on=True):
    m = _random_mbs(rng, 24, segs=True)
    seg = dict(update_map=1, feature_mode=1, quant=(10, 40, 90, 127), lf=(5, 20, 0, 63), probs=(120, 100, 160)) if on else None
    return 96, 64, m, None, dict(segmentation=seg, y_ac_qi=25, level=12)


def _geometry(rng, width, height, log2_parts, skip_p=0.1):
    cols, rows = (((width + 3) & ~3) + 15) >> 4, (((height + 3) & ~3) + 15) >> 4
    m = _random_mbs(rng, cols * rows, skip_p=skip_p)
    m["skip"][0] = False
    return width, height, _legal(m), None, dict(log2_parts=log2_parts, prob_skip=200 if skip_p else None, segmentation=SEG0, y_ac_qi=28, level=10)


GEOMETRY = {"1x1": (16, 16, 0), "1x9_p8": (16, 144, 3), "9x1_p8": (144, 16, 3), "3x10_p2": (48, 160, 1), "3x10_p4": (48, 160, 2), "3x10_p8": (48, 160, 3),
            "50x37": (50, 37, 0), "9x1_p4": (144, 16, 2)}
BUILDERS = {
    "all_slots": _all_slots, "token_ladder": _token_ladder, "extreme_probs": _extreme_probs, "every_bmode_context": _every_bmode_context,
    "y2_context": _y2_context, "skips": _skips, "skips_coded_first": lambda rng: _skips(rng, first_skipped=False),
    "skips_all": lambda rng: _skips(rng, every=True), "segments": _segments, "segments_off": lambda rng: _segments(rng, on=False),
}
# name: (builder or geometry, extra arguments of keyframe_from)
CASES = {name: (name, {}) for name in BUILDERS}
CASES.update({"geo_" + g: (g, {}) for g in GEOMETRY if g != "9x1_p4"})
TIGHT = ("tight_1x9_p8", "tight_3x10_p4", "tight_50x37", "tight_9x1_p8")            # every partition ends on the last byte a decoder loads
CASES.update({t: (t[6:], dict(tight=True)) for t in TIGHT})
# twins of the tight files with ONE partition a byte shorter: the first partition, a middle token partition, the last one
SHORT = {"tight_1x9_p8": ("p0", 3, 7), "tight_3x10_p4": ("p0", 1, 3), "tight_50x37": ("p0", 0), "tight_9x1_p8": ("p0", 0)}
CASES.update({f"{t}_short_{k}": (t[6:], dict(tight=True, short=k)) for t, ks in SHORT.items() for k in ks})
REFUSED = tuple(n for n in CASES if "_short_" in n)
# the 9 x 1 frame whose unread partitions have length 0: with 8 partitions, and with 4, which the reference can be asked about (it decodes it)
CASES.update({"unused_empty": ("9x1_p8", dict(empty_parts=tuple(range(1, 8)))), "unused_empty_p4": ("9x1_p4", dict(empty_parts=(1, 2, 3)))})
ACCEPTED = tuple(n for n in CASES if n not in REFUSED)
# what the reference's loader can take (facts["ref_ok"] says why; the tests hold this list against it)
REF_OK = ("all_slots", "token_ladder", "extreme_probs", "every_bmode_context", "y2_context", "skips_coded_first", "segments", "segments_off",
          "geo_1x1", "geo_3x10_p2", "geo_3x10_p4", "tight_3x10_p4", "unused_empty_p4")


def expected_modes(m):
    n = len(m["ymode"])
    rec = np.zeros((n, 20), np.uint8)
    rec[:, 0], rec[:, 1], rec[:, 18] = m["ymode"], m["uvmode"], m["seg"]
    b = m["ymode"] == 4
    rec[b, 2:18] = m["bmodes"][b]
    rec[~b, 2] = m["ymode"][~b]
    return rec


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    what, extra = CASES[name]
    rng = np.random.default_rng([seed, sum(what.encode())])         # a tight file, its twins and the padded file of one geometry share their data
    width, height, m, z16, header = BUILDERS[what](rng) if what in BUILDERS else _geometry(rng, *GEOMETRY[what])
    facts = W.new_facts()
    data = W.keyframe_from(width, height, m, zeros16=z16, facts=facts, **header, **extra)
    n = len(m["ymode"])
    mbinfo = np.zeros((n, 27), np.uint8)
    mbinfo[:, :25], mbinfo[:, 25], mbinfo[:, 26] = facts["counts"], m["ymode"] != 4, m["seg"]
    nparts = 1 << header.get("log2_parts", 0)
    facts.update(name=name, seed=seed, width=width, height=height, mbcols=(((width + 3) & ~3) + 15) >> 4, mbrows=(((height + 3) & ~3) + 15) >> 4,
                 nparts=nparts, header=header, written=m["levels"], skip=m["skip"], ymode=m["ymode"], zeros16=z16, probs=W.decode(data)["probs"] if "short" not in extra else None,
                 refused=name in REFUSED, short=extra.get("short"),
                 ref_ok=nparts <= 4 and height % 16 == 0 and not m["skip"][0] and "short" not in extra)
    arrays = [expected_modes(m), facts["levels"], mbinfo, facts["resmap"]]
    for a in arrays:
        a.setflags(write=False)
    return Case(data, *arrays, facts)
