"""The two kernels of the device front end (k_webp_mb_headers: mode records, residual map; k_webp_tokens: levels, token counts) and
the files call built on them against the answer key of tests/vp8_cases.py: key frames written from known modes, segment ids, skip
flags and levels.  Expectations come from the writer, the CPU oracle chain and nothing else."""
import functools

import numpy as np
import pytest

import vp8_cases as VC
from ffpic_amd import capi, ops
from test_vp8_known_tokens import ALL, header_status
from test_webp_front_capi import check_modes, oracle_bgra, oracle_residual

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    for n in ("FFHIP_WEBP_GPU_ENTROPY", "FFHIP_WEBP_PACK"):
        capi.setenv(n, None)


def same_arrays(dev, case, who):
    """kernel A and kernel B separately, so that a failure says which half is wrong"""
    check_modes(dev["modes"], case.modes)
    assert np.array_equal(dev["resmap"], case.resmap), f"{who}: kernel A, residual map"
    assert np.array_equal(dev["mbinfo"][:, :27], case.mbinfo), f"{who}: kernel B, token counts / has_y2 / segment"
    assert np.array_equal(dev["levels"], case.levels), f"{who}: kernel B, levels"


def check_call(cases, outs, status):
    for c, o, st in zip(cases, outs, status):
        if c.facts["refused"]:
            assert st == capi.FFHIP_EINVAL and o is None, c.facts["name"]
        else:
            assert st == 0, c.facts["name"]
            same_arrays(o, c, c.facts["name"])


@pytest.mark.parametrize("name", VC.ACCEPTED)
def test_kernels_return_what_was_written(name):
    """every case alone, and as a batch of three seeds"""
    one = [VC.case(name)]
    check_call(one, *ops.webp_parse_device([c.data for c in one]))
    three = [VC.case(name, seed) for seed in (0, 1, 2)]
    check_call(three, *ops.webp_parse_device([c.data for c in three]))


@pytest.mark.parametrize("pack", [5, 32])
def test_one_shuffled_batch_of_all_cases_packed(pack):
    """several frames to a wave: neighbouring lanes carry different probabilities, partition counts and sizes, and some of them a
    partition that runs dry"""
    capi.setenv("FFHIP_WEBP_PACK", pack)
    cases = [VC.case(ALL[i]) for i in np.random.default_rng(pack).permutation(len(ALL))]
    check_call(cases, *ops.webp_parse_device([c.data for c in cases]))


def test_tight_files_and_their_one_byte_short_twins():
    names = [n for t in VC.TIGHT for n in [t] + [f"{t}_short_{k}" for k in VC.SHORT[t]]] + ["unused_empty", "unused_empty_p4"]
    cases = [VC.case(n) for n in names]
    outs, status = ops.webp_parse_device([c.data for c in cases])
    check_call(cases, outs, status)
    assert sum(st != 0 for st in status) == len(VC.REFUSED) == 10
    for c, st in zip(cases, status):
        if c.facts["short"] == "p0":
            # cut in the macroblock headers: the host's header pass accepts the file, so the refusal is kernel A's verdict word
            assert header_status(c.data) == 0 and st == capi.FFHIP_EINVAL


@functools.lru_cache(maxsize=None)
def oracle_pixels(name):
    """the CPU oracle chain on the WRITTEN arrays (the header's quantisers and filter parameters from the host parser)"""
    c = VC.case(name)
    p = ops.webp_parse(c.data)
    info = np.zeros((len(c.mbinfo), 32), np.uint8)
    info[:, :27] = c.mbinfo
    w = dict(p, modes=c.modes.copy(), levels=c.levels.copy(), mbinfo=info, resmap=c.resmap.copy())
    return p["width"], p["height"], oracle_bgra(w, oracle_residual(w)).reshape(16 * p["mbrows"], 16 * p["mbcols"], 4)


@pytest.mark.parametrize("entropy", [1, 0, None])
def test_files_call_gives_the_oracle_pixels_of_the_written_arrays(entropy):
    """ffhip_webp_decode_files_device over every case and twin in one call, the kernels forced, the host threads forced, and the default"""
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
    files = [VC.case(n).data for n in ALL]
    for crop in (True, False):
        infos, images, _, status = ops.webp_decode_files_device(files, strict=False, crop=crop)
        for n, img, st in zip(ALL, images, status):
            if VC.case(n).facts["refused"]:
                assert st == capi.FFHIP_EINVAL and img is None, n
                continue
            assert st == 0, n
            w, h, want = oracle_pixels(n)
            assert np.array_equal(img, want[:h, :w] if crop else want), (n, crop)
    dev_parts, host_parts = ops.webp_last_parts()
    assert (dev_parts, host_parts) == ((1, 0) if entropy == 1 else (0, 1))
