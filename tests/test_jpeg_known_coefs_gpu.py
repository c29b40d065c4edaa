"""GPU: both device JPEG entropy decoders against the ANSWER -- files written from known coefficients (tests/jpeg_cases.py); equality is exact everywhere.
tests/test_jpeg_known_coefs.py has the Python decoder, the host decoder and the reference agree with the written coefficients on the CPU, so a
mismatch here is a kernel's -- or, where both kernels and the host agree with each other, huff_build's / build_lut's.

Which test stands for which branch of ffhip_huff_gpu.hip:
  the canonical-code walk, `if (!e)`, of k_jpeg_huff (form lane_per_interval) and of k_huff_span (form subsequences), and build_lut leaving an incomplete
      table's zeros alone (marked complete, every walked code would read "no such code" and the call would fail):
      test_deep_tables_take_the_canonical_code_walk, and test_planes[...deep...]
  the `staged` / `cmask` hand-over at the end of k_huff_span, a block that goes on in the lane behind:
      test_dense_blocks_are_handed_from_lane_to_lane (blocks of 1 100 bits under subsequences of 128, 2 048 and 8 192 bits), test_subsequence_switches
  the `in_lds == false` copy of either kernel's loop, a wave over pictures with different tables: test_different_tables_side_by_side
  table ids 2 / 3, one pair for all components, DC size 11, 26 / 27-bit steps, k = 63 by a run, three ZRLs, runs of 15 and 16, lanes of hundreds of
      tiny blocks, scans dense in FF 00: test_planes on the cases of those names (jpeg_cases.CASES)"""
import numpy as np
import pytest

import jpeg_cases as JC
import oracle_lib as O
from ffpic_amd import capi, ops

pytestmark = pytest.mark.gpu
ALL = list(JC.CASES)


@pytest.fixture(params=["subsequences", "lane_per_interval"])
def form(request, monkeypatch):
    """both device decoders: the subsequence decoder (FFHIP_JPEG_SYNC=1: a lane per subsequence of a restart interval, synchronised over rounds) and
    k_jpeg_huff (FFHIP_JPEG_SYNC=0: a lane per restart interval, a file without markers one lane's)"""
    monkeypatch.setenv("FFHIP_JPEG_SYNC", "1" if request.param == "subsequences" else "0")
    capi.reload_env()
    yield request.param
    monkeypatch.undo()
    capi.reload_env()


@pytest.fixture
def switch(monkeypatch):
    def set_(**kw):
        for k, v in kw.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        capi.reload_env()
    yield set_
    monkeypatch.undo()
    capi.reload_env()


def written_planes(cases):
    """ffhip_jpeg_entropy_batch_gpu on the cases' files (one geometry) returns the written planes and quantisers"""
    g, cy, cu, cv, q = ops.jpeg_entropy_batch_gpu([c.data for c in cases])
    wy, wu, wv = JC.planes_of(cases)
    names = [c.facts["name"] for c in cases]
    assert np.array_equal(cy, wy), names
    if g.ncomp == 3:
        assert np.array_equal(cu, wu) and np.array_equal(cv, wv), names
    for i, c in enumerate(cases):
        for t in set(tuple(g.qt_id)[:g.ncomp]):
            assert np.array_equal(q[i][t], c.quant[t]), names


def oracle_pixels(case):
    """the oracle's reconstruction of the WRITTEN coefficients, at the coded size"""
    f = case.facts
    g = O.make_geom(f["mcu_cols"], f["mcu_rows"], f["ncomp"], f["h"], f["v"])
    return O.oracle_jpeg_recon(g, case.coef[0], case.coef[1], case.coef[2], case.quant)[0]


# ---------------------------------------------------------------------------------------------------- 1. planes
@pytest.mark.parametrize("name", ALL)
def test_planes(form, name):
    """every case alone and as a batch of three pictures of its geometry with different content"""
    written_planes([JC.case(name)])
    written_planes([JC.case(name, seed) for seed in range(3)])


@pytest.mark.parametrize("name", ["440_mixed_deep", "grey_dense_deep_r5", "420_3x2_mixed_deep23_r1", "444_1_sparse_deep"])
def test_deep_tables_take_the_canonical_code_walk(form, name):
    """AC tables with long codes under 30 nine-bit prefixes, 8 of which get a group of the look-up table: EOB, ZRL and the small run/size pairs are
    decoded by the `if (!e)` walk of the kernel `form` selects (thousands of times in the two large pictures), from struct huff's maxcode / mincode /
    valptr in global memory.  Without the walk, or with the table marked complete by build_lut, these planes cannot come out"""
    written_planes([JC.case(name)])
    written_planes([JC.case(name, seed) for seed in (3, 4)])


@pytest.mark.parametrize("bits", [None, 128, 2048, 8192])
def test_dense_blocks_are_handed_from_lane_to_lane(switch, bits):
    """blocks of 64 non-zero coefficients, 1 100 bits each: under subsequences of 128 bits a block spans nine lanes, under 2 048 every lane begins and
    ends inside one.  The write pass keeps the first four rows of a block it began in LDS; a block that goes on in the lane behind leaves them through
    the `cmask` loop at the end of k_huff_span, and the lanes behind store coefficient by coefficient (`staged` false)"""
    switch(FFHIP_JPEG_SYNC=1, FFHIP_JPEG_SYNC_BITS=bits)
    written_planes([JC.case("420_dense")])
    written_planes([JC.case("420_dense", 1), JC.case("420_dense", 2)])


# ---------------------------------------------------------------------------------------------------- 2. the subsequence decoder's switches
@pytest.mark.parametrize("env", [{"FFHIP_JPEG_SYNC_BITS": 128}, {"FFHIP_JPEG_SYNC_BITS": 65536}, {"FFHIP_JPEG_SYNC_ROUNDS": 1}, {"FFHIP_JPEG_SYNC_PARTS": 3}],
                         ids=["bits128", "bits65536", "rounds1", "parts3"])
@pytest.mark.parametrize("name", JC.HARD)
def test_subsequence_switches(switch, name, env):
    """the large dense, sparse, mixed and deep-tables pictures: subsequences of 128 bits (a block spans a dozen lanes) and of 65 536 (the scan in two or
    three lanes); one list round per batch of launches, so that the fixed point is reached through huff_sync_finish only; the batch in three parts"""
    switch(FFHIP_JPEG_SYNC=1, **env)
    written_planes([JC.case(name, seed) for seed in range(3)])


# ---------------------------------------------------------------------------------------------------- 3. different tables side by side
def test_different_tables_side_by_side(form):
    """40 files of 2 x 2 MCUs whose neighbours carry Annex K's, deep, long and one shared pair of tables: a picture is a lane (lane_per_interval) or a
    few (subsequences), so every wave spans pictures whose tables are not the ones in LDS -- the copy of the loop that looks up in global memory"""
    written_planes(JC.table_cycle(40))


# ---------------------------------------------------------------------------------------------------- 4. files to pixels
@pytest.mark.parametrize("device_entropy", [None, "1", "0"])
@pytest.mark.parametrize("name", ALL)
def test_files_to_pixels(switch, name, device_entropy):
    """ffhip_jpeg_decode_files_device as shipped, with every file's entropy decode forced onto the device, and onto the host threads: the oracle's
    reconstruction of the written coefficients"""
    switch(FFHIP_JPEG_GPU_ENTROPY=device_entropy)
    cases = [JC.case(name), JC.case(name, 1)]
    got = ops.jpeg_decode_files_device([c.data for c in cases], n_threads=3)[1]
    for i, c in enumerate(cases):
        assert np.array_equal(got[i], oracle_pixels(c)), (name, i)


@pytest.mark.parametrize("device_entropy", [None, "1", "0"])
def test_every_layout_and_table_family_in_one_mixed_call(switch, device_entropy):
    """ffhip_jpeg_decode_files_mixed_device on one shuffled batch: 56 small pictures -- seven layouts x Annex K / deep / long / shared tables x with and
    without restart markers -- and the seven large ones"""
    switch(FFHIP_JPEG_GPU_ENTROPY=device_entropy)
    cases = JC.everything()
    assert len(cases) == 63
    geoms, images, _ = ops.jpeg_decode_files_mixed_device([c.data for c in cases], n_threads=4, crop=False)
    for c, img in zip(cases, images):
        assert np.array_equal(img, oracle_pixels(c)), c.facts["name"]
