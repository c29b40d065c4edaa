"""Baseline JPEG files WRITTEN from known coefficients (tests/jpeg_writer.py), for the tests that pin every entropy decoder of the project on the answer
instead of on each other: a decoder is right when it returns exactly the planes that went in.  Plain Python, seeded, no PIL.

case(name, seed) -> Case(data, coef, quant, facts): the file's bytes, the coefficient planes as written (per component int16, flat, blocks in MCU order,
natural order inside a block -- what jpeg_entropy.decode and the library's decoders return; None for a component the picture lacks), the quantisers
[4][64] and a dict of facts: layout, MCU counts, picture size, restart interval, family, tables and the writer's stats.

Coefficient families (all within [-1023, 1023] for AC, [-1024, 1023] for DC: legal baseline) and the decoder branches they are there for:
  laplace  synth._blocks: what a photograph looks like (the common path, as a control)
  dense    64 non-zero coefficients a block, magnitudes 1, 2^s - 1, 2^(s-1) and 1023 over all sizes 1..10, DC alternating -1024 / 1023: no EOB (the block
           ends by k = 63), DC differences of +-2047 (size 11), AC size 10 under 16-bit codes (26-bit steps; 27 with the long DC codes), blocks of more than
           1 024 bits that straddle lanes of the subsequence decoder (the `staged` / `cmask` hand-over at the end of k_huff_span)
  sparse   all-zero blocks and blocks with ONE coefficient at k = 1, 16, 17, 32, 33, 48, 49 or 63: runs of exactly 15, 16, 31, 47 and 62, up to three ZRLs
           in a row, a coefficient at k = 63 reached by a run (no EOB), hundreds of blocks of a few bits to one lane
  ones     values 2^s - 1 and -2^s + 1 under ones_tables: a scan dense in 0xFF and stuffed zeros (stage_scan's unstuffing, the alignment of every interval)
  mixed    dense blocks alternate with near-empty ones and blocks of the other families: lanes loaded unevenly
Table families (jpeg_writer): annexk; deep (more long-code prefixes than the look-up table has groups: the canonical-code walk, `if (!e)`, in both
kernels); long (16-bit codes for everything in use); shared (one DC / AC pair for all components); ones; ids23 / deep23 (tables under ids 2 and 3)."""
import collections
import functools

import numpy as np

import jpeg_writer as W
from ffpic_amd import synth
from jpeg_entropy import ZZ

Case = collections.namedtuple("Case", "data coef quant facts")

LAYOUTS = {"420": (3, 2, 2), "444": (3, 1, 1), "422": (3, 2, 1), "440": (3, 1, 2), "h4v1": (3, 4, 1), "h1v4": (3, 1, 4), "grey": (1, 1, 1)}
SPARSE_K = (1, 16, 17, 32, 33, 48, 49, 63)
LUT_GROUPS = 8          # of ffhip_huff_gpu.hip
SUB_BITS = 2048         # the subsequence decoder's shortest default


def tables_of(name):
    """-> (tables, table_ids) for jpeg_writer.encode"""
    std = ((0, 0), (1, 1), (1, 1))
    if name == "annexk":
        return None, None
    if name == "deep":
        return W.deep_tables(), std
    if name == "long":
        return W.long_tables(), std
    if name == "ones":
        return W.ones_tables(), std
    if name == "shared":
        return W.short_dc_tables(), ((0, 0),) * 3
    annexk = {(0, 0): W.DC_L, (1, 0): W.AC_L, (0, 1): W.DC_C, (1, 1): W.AC_C}
    if name == "ids23":     # luma: DC table 2, AC table 3; chroma: DC table 3, AC table 2
        return W.with_ids(annexk, {(0, 0): 2, (1, 0): 3, (0, 1): 3, (1, 1): 2}), ((2, 3), (3, 2), (3, 2))
    if name == "deep23":    # luma under 3 / 2, chroma under 0 / 1
        return W.with_ids(W.deep_tables(), {(0, 0): 3, (1, 0): 2, (0, 1): 0, (1, 1): 1}), ((3, 2), (0, 1), (0, 1))
    raise KeyError(name)


def walk_symbols(counts, symbols):
    """the symbols of a table whose codes the device look-up table does NOT hold: codes of 10..16 bits under a nine-bit prefix that got no group (the
    first LUT_GROUPS prefixes in the order of (length, code) get one, as build_lut deals them out).  -> {symbol: nine-bit prefix}"""
    codes = W._codes(counts, symbols)
    grouped, out = [], {}
    for sym, (code, length) in sorted(codes.items(), key=lambda kv: (kv[1][1], kv[1][0])):
        if length <= 9:
            continue
        prefix = code >> (length - 9)
        if prefix not in grouped:
            if len(grouped) == LUT_GROUPS:
                out[sym] = prefix
                continue
            grouped.append(prefix)
    return out


# ---------------------------------------------------------------------------------------------------- coefficient families: int16 [n][64], natural order
def _signs(rng, shape):
    return rng.integers(0, 2, shape) * 2 - 1


def laplace(rng, n, q):
    return synth._blocks(rng, n, q)


def dense(rng, n, q=None):
    s = rng.integers(1, 11, (n, 64))
    kind = rng.choice(4, (n, 64), p=[0.1, 0.2, 0.2, 0.5])
    mag = np.choose(kind, [np.ones_like(s), (1 << s) - 1, 1 << (s - 1), np.full_like(s, 1023)])
    b = (mag * _signs(rng, (n, 64))).astype(np.int16)
    b[:, 0] = np.where(np.arange(n) % 2 == 0, -1024, 1023)
    return b


def sparse(rng, n, q=None):
    b = np.zeros((n, 64), np.int16)
    one = rng.random(n) < 0.6
    k = rng.choice(SPARSE_K, n)
    val = rng.integers(1, 4, n) * _signs(rng, n)
    rows = np.flatnonzero(one)
    b[rows, ZZ[k[rows]]] = val[rows]
    b[:, 0] = np.cumsum(np.where(rng.random(n) < 0.1, rng.integers(-2, 3, n), 0))      # mostly a DC difference of 0
    return b


def ones(rng, n, q=None):
    s = rng.integers(1, 11, (n, 64))
    b = (((1 << s) - 1) * _signs(rng, (n, 64))).astype(np.int16)
    b[rng.random((n, 64)) < 0.5] = 0
    b[:, 0] = ((1 << rng.integers(1, 11, n)) - 1) * _signs(rng, n)
    return b


def mixed(rng, n, q):
    fam = [dense(rng, n), sparse(rng, n), laplace(rng, n, q), ones(rng, n), np.zeros((n, 64), np.int16)]
    pick = np.where(np.arange(n) % 2 == 0, 0, rng.choice([1, 1, 2, 3, 4, 4], n))
    b = np.choose(pick[:, None], fam).astype(np.int16)
    b[pick == 4, 0] = b[np.maximum(np.flatnonzero(pick == 4) - 1, 0), 0]                # an empty block repeats the DC in front: a difference of 0 where both
    return b                                                                            # are of one component (grey), a small block anyway


FAMILIES = {"laplace": laplace, "dense": dense, "sparse": sparse, "ones": ones, "mixed": mixed}

# name: (layout, mcu_cols, mcu_rows, family, tables, restart, pixels short of the coded width, of the coded height)
CASES = {
    # one MCU
    "420_1_dense": ("420", 1, 1, "dense", "annexk", 0, 7, 5),
    "444_1_sparse_deep": ("444", 1, 1, "sparse", "deep", 0, 0, 0),
    "422_1_ones": ("422", 1, 1, "ones", "ones", 0, 0, 0),
    "440_1_mixed_long": ("440", 1, 1, "mixed", "long", 0, 0, 0),
    "h4v1_1_laplace_shared": ("h4v1", 1, 1, "laplace", "shared", 0, 0, 0),
    "h1v4_1_dense_ids23": ("h1v4", 1, 1, "dense", "ids23", 0, 0, 0),
    "grey_1_mixed_deep": ("grey", 1, 1, "mixed", "deep", 0, 0, 0),
    # 3 x 2 MCUs: restart intervals of 1 MCU, 5 MCUs (the last one short) and an MCU row; widths that are no multiple of the MCU
    "420_3x2_mixed_deep23_r1": ("420", 3, 2, "mixed", "deep23", 1, 0, 0),
    "444_3x2_dense_long_r5": ("444", 3, 2, "dense", "long", 5, 0, 0),
    "422_3x2_laplace_row": ("422", 3, 2, "laplace", "annexk", 3, 5, 0),
    "440_3x2_sparse_shared": ("440", 3, 2, "sparse", "shared", 0, 0, 0),
    "h4v1_3x2_ones_r1": ("h4v1", 3, 2, "ones", "ones", 1, 0, 0),
    "h1v4_3x2_mixed_long": ("h1v4", 3, 2, "mixed", "long", 0, 3, 3),
    "grey_3x2_dense_ids23_r5": ("grey", 3, 2, "dense", "ids23", 5, 0, 0),
    # one picture per layout of 40 subsequences of 2 048 bits or more
    "420_dense": ("420", 6, 4, "dense", "annexk", 0, 0, 0),
    "444_sparse": ("444", 48, 32, "sparse", "annexk", 0, 0, 0),
    "422_mixed_row": ("422", 10, 6, "mixed", "annexk", 10, 0, 0),
    "440_mixed_deep": ("440", 10, 6, "mixed", "deep", 0, 0, 0),
    "h4v1_ones": ("h4v1", 8, 5, "ones", "ones", 0, 0, 0),
    "h1v4_mixed_long_r1": ("h1v4", 8, 5, "mixed", "long", 1, 0, 0),        # 40 intervals: RSTn wraps D7 -> D0 four times
    "grey_dense_deep_r5": ("grey", 10, 8, "dense", "deep", 5, 0, 0),       # 16 intervals
}
LARGE = ("420_dense", "444_sparse", "422_mixed_row", "440_mixed_deep", "h4v1_ones", "h1v4_mixed_long_r1", "grey_dense_deep_r5")
HARD = ("420_dense", "444_sparse", "422_mixed_row", "440_mixed_deep")        # the large dense, sparse, mixed and deep_tables pictures
ZERO_STRETCH = 600      # all-zero blocks in a row in the large sparse picture: more than SUB_BITS / 4 of them, 2..4 bits each (6 under the luma tables)


def _write(layout, mc, mr, family, tables, restart, short_w, short_h, seed, name, end_in_ones=False):
    ncomp, h, v = LAYOUTS[layout]
    rng = np.random.default_rng([seed, sum(name.encode())])
    quant = synth.quant_tables(60 + 5 * (seed % 7))
    mcus = mc * mr
    fam = FAMILIES[family]
    planes = [fam(rng, mcus * h * v, quant[0])]
    if ncomp == 3:
        planes += [fam(rng, mcus, quant[1]), fam(rng, mcus, quant[1])]
    if name == "444_sparse":        # a subsequence and more of blocks that are nothing but a DC difference of 0 and an EOB
        for p in planes:
            a = mcus // 3
            p[a:a + ZERO_STRETCH // 3] = 0
            p[a:a + ZERO_STRETCH // 3, 0] = p[a - 1, 0]
    if end_in_ones:
        # The scan's last coefficient: 1023 at k = 63 -- ten one-bits and no EOB behind them, so with the padding the scan ends in FF 00.  The reference's
        # loader keeps a scan's last byte only when it is such a pair (read_compressed_scan, format/jpg.c:604-633, stores the byte BEFORE the one it
        # has just read) and otherwise decodes the end of the last data unit from a byte of memory it never wrote: pixels that differ from run to run,
        # or "bits longer than expect" and exit (utils/bitstream.c:117).  With this ending its decode of the whole file is a function of the file.
        planes[-1][-1, 63] = 1023
    tabs, ids = tables_of(tables)
    stats = {}
    coef = planes + [None] * (3 - ncomp)
    width, height = mc * 8 * h - short_w, mr * 8 * v - short_h
    data = W.encode(width, height, h, v, coef, quant, restart=restart, tables=tabs, table_ids=ids, stats=stats)
    facts = dict(name=name, layout=layout, ncomp=ncomp, h=h, v=v, mcu_cols=mc, mcu_rows=mr, width=width, height=height, restart=restart, family=family,
                 tables=tables, table_ids=ids or ((0, 0), (1, 1), (1, 1)), dht=tabs or {(0, 0): W.DC_L, (1, 0): W.AC_L, (0, 1): W.DC_C, (1, 1): W.AC_C},
                 stats=stats, seed=seed)
    flat = [np.ascontiguousarray(p.reshape(-1)) if p is not None else None for p in coef]
    for p in flat:
        if p is not None:
            p.setflags(write=False)
    return Case(data, flat, quant, facts)


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """seed 0: the file every witness reads, the reference among them, with the ending the reference needs (_write); other seeds end as they fall, most
    in an EOB and padding bits"""
    return _write(*CASES[name], seed, name, end_in_ones=seed == 0)


@functools.lru_cache(maxsize=None)
def small(layout, tables, restart, mc=2, mr=2, family="mixed", seed=0):
    """a small picture outside the list: the batches of many files"""
    return _write(layout, mc, mr, family, tables, restart, 0, 0, seed, f"{layout}_{mc}x{mr}_{family}_{tables}_r{restart}")


def table_cycle(n=40, layout="420"):
    """n files of 2 x 2 MCUs of one geometry whose neighbours carry different tables: Annex K, deep, long, the shared pair, in turn"""
    return [small(layout, ("annexk", "deep", "long", "shared")[i % 4], 0, seed=i) for i in range(n)]


def everything():
    """one batch for the mixed-geometry call: every layout with every table family, with and without restart markers (56 small pictures of 2 x 2 and
    3 x 1 MCUs), and the large pictures once each -- shuffled"""
    out = []
    for li, layout in enumerate(LAYOUTS):
        for ti, tables in enumerate(("annexk", "deep", "long", "shared")):
            for restart in (0, 2):
                mc, mr = ((2, 2), (3, 1))[(li + ti) % 2]
                out.append(small(layout, tables, restart, mc, mr, ("mixed", "dense", "sparse", "ones", "laplace")[(li + ti + restart) % 5], seed=li))
    out += [case(name) for name in LARGE]
    order = np.random.default_rng(99).permutation(len(out))
    return [out[i] for i in order]


def planes_of(cases):
    """the written planes of a batch of one geometry, picture after picture: what the batch calls return"""
    cat = lambda k: np.concatenate([c.coef[k] for c in cases]) if cases[0].coef[k] is not None else None
    return cat(0), cat(1), cat(2)
