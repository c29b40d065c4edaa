"""Lossy WebP files to device pixels (ffhip_webp_decode_files_device): the bool decoder on the GPU against the reference's BGRA of
every fixture, its two kernels against the host parser, and the switches of the path."""
import os
import threading

import numpy as np
import pytest

from ffpic_amd import capi, ops
from test_webp_front_capi import FRONT, GOLDEN, NAMES, UNPINNED, file_bytes, oracle_bgra, oracle_residual

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    names = ("FFHIP_WEBP_GPU_ENTROPY", "FFHIP_WEBP_GPU_MIN_FILES", "FFHIP_WEBP_PACK", "FFHIP_WEBP_PART_MB")
    yield
    for n in names:
        capi.setenv(n, None)


def ref_bgra(name, img):
    """the reference's pixels of the fixture, cut like `img` (crop=True: the probe's width x height)"""
    ref = FRONT[f"{name}_bgra"]
    h, w = img.shape[:2]
    return ref[:h, :4 * w].reshape(h, w, 4)


def check_all(images, names):
    for n, img in zip(names, images):
        w, h, _ = [int(x) for x in FRONT[f"{n}_dims"]]
        assert img.shape[:2] == (h, w), n
        assert np.array_equal(img, ref_bgra(n, img)), n


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_alone(name):
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", 1)
    infos, images, _ = ops.webp_decode_files_device([file_bytes(name)])
    check_all(images, [name])


def mixed_batch():
    rng = np.random.default_rng(11)
    order = [NAMES[i] for i in rng.permutation(len(NAMES))]
    files = [file_bytes(n) for n in order]
    bad = bytearray(file_bytes("syn_parts4"))
    del bad[len(bad) - 20000:]                      # a partition size now points outside the file: refused with the header
    mid = len(files) // 2
    files.insert(mid, bytes(bad))
    return order, files, mid


def late_bad():
    """truncated inside its LAST partition: the header is fine, kernel B (or the host loop) runs off the partition"""
    return file_bytes("syn_parts2")[:-5950]


@pytest.mark.parametrize("mode", ["kernels", "kernels_packed", "kernels_small_parts", "host_threads", "default"])
def test_all_fixtures_in_one_call_with_a_damaged_file(mode):
    order, files, mid = mixed_batch()
    if mode != "default":
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", 0 if mode == "host_threads" else 1)
    if mode == "kernels_packed":
        capi.setenv("FFHIP_WEBP_PACK", 5)           # five frames to a wave, divergent
    if mode == "kernels_small_parts":
        capi.setenv("FFHIP_WEBP_PART_MB", 100)      # many parts; files of more macroblocks are parts of their own
    files = files + [late_bad()]
    infos, images, _, status = ops.webp_decode_files_device(files, strict=False)
    assert status[mid] == capi.FFHIP_EINVAL and images[mid] is None
    assert status[-1] == capi.FFHIP_EINVAL and images[-1] is None
    assert not any(status[:mid] + status[mid + 1:-1])
    check_all(images[:mid] + images[mid + 1:-1], order)
    dev_parts, host_parts = ops.webp_last_parts()
    if mode in ("host_threads", "default"):         # 27 small files: far below 32 per host thread of the largest
        assert dev_parts == 0 and host_parts >= 1
    else:
        assert host_parts == 0 and (dev_parts > 5 if mode == "kernels_small_parts" else dev_parts == 1)


def test_min_files_switch_moves_the_crossover():
    """FFHIP_WEBP_GPU_MIN_FILES: parts of fewer files go to the host threads; same bytes either side of it"""
    order, files, mid = mixed_batch()
    del files[mid]
    for v, want in ((1, (1, 0)), (10 ** 6, (0, 1))):
        capi.setenv("FFHIP_WEBP_GPU_MIN_FILES", v)
        infos, images, _ = ops.webp_decode_files_device(files)
        check_all(images, order)
        assert ops.webp_last_parts() == want


def test_default_crossover_scales_with_the_host_threads():
    """unforced: the kernels from 32 x n_threads of the largest frame on, the host threads below"""
    data = file_bytes("syn_q0")
    for n, nt, want in ((64, 2, (1, 0)), (63, 2, (0, 1)), (64, 3, (0, 1)), (96, 3, (1, 0))):
        infos, images, _ = ops.webp_decode_files_device([data] * n, n_threads=nt)
        assert ops.webp_last_parts() == want, (n, nt)
        check_all(images[:2] + images[-1:], ["syn_q0"] * 3)


@pytest.mark.parametrize("name", UNPINNED)
def test_unpinned_files_three_ways(name):
    """no reference output exists for these (8 partitions; a height of 37): the kernels, the host threads and the CPU oracle chain on
    the host parser's arrays must give the same pixels, and the rows up to the height rounded up to 4 come out"""
    data = file_bytes(name)
    host = ops.webp_parse(data)
    want = oracle_bgra(host, oracle_residual(host)).reshape(16 * host["mbrows"], 16 * host["mbcols"], 4)
    for val in (1, 0):
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", val)
        infos, images, _ = ops.webp_decode_files_device([data])
        assert images[0].shape[:2] == (host["height"], host["width"])
        assert np.array_equal(images[0], want[:host["height"], :host["width"]]), val
        infos, full, _ = ops.webp_decode_files_device([data], crop=False)
        assert np.array_equal(full[0], want), val


@pytest.mark.parametrize("name", NAMES + UNPINNED + ["file_1080p_q75"])
def test_kernels_equal_the_host_parser(name):
    """kernel A (modes, resmap) and kernel B (levels, mbinfo) separately, so that a failure says which half is wrong"""
    data = file_bytes(name)
    host = ops.webp_parse(data)
    dev, status = ops.webp_parse_device([data])
    assert status == [0]
    assert np.array_equal(dev[0]["modes"], host["modes"]), "kernel A: mode records"
    assert np.array_equal(dev[0]["resmap"], host["resmap"]), "kernel A: residual map"
    assert np.array_equal(dev[0]["mbinfo"], host["mbinfo"]), "kernel B: token counts"
    assert np.array_equal(dev[0]["levels"], host["levels"]), "kernel B: levels"
    assert np.array_equal(dev[0]["quant"], host["quant"]) and np.array_equal(dev[0]["filters"], host["filters"])


def test_kernels_give_a_truncated_file_their_verdict():
    dev, status = ops.webp_parse_device([file_bytes("syn_q0"), late_bad()])   # 50 bytes of its second token partition are left
    assert status[0] == 0 and status[1] == capi.FFHIP_EINVAL


def row_sums(img):
    rows = np.ascontiguousarray(img).reshape(img.shape[0], -1).view(np.uint32).astype(np.uint64)
    return (rows * (np.arange(rows.shape[1], dtype=np.uint64) + np.uint64(1))).sum(axis=1, dtype=np.uint64)


def test_256_copies_of_the_1080p_stream():
    data = file_bytes("file_1080p_q75")
    want = np.load(os.path.join(GOLDEN, "webp_file_1080p.npz"))
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", 1)
    infos, images, _ = ops.webp_decode_files_device([data] * 256)
    assert images[0].shape == (1088, 1920, 4)
    assert np.array_equal(images[0][:32], want["bgra_head"][:32, :1920 * 4].reshape(32, 1920, 4))
    for k in (0, 1, 100, 255):
        assert np.array_equal(row_sums(images[k]), want["bgra_row_sums"]), k
    for k in range(256):
        assert np.array_equal(images[k], images[0]), k


def test_two_host_threads_with_a_stream_each():
    L = capi.lib()
    order, files, mid = mixed_batch()
    del files[mid]
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", 1)
    results, errors = {}, []

    def work(t):
        try:
            capi.require_device(0)
            st = L.ffhip_stream_create()
            mine = files[t::2] * 3
            infos, images, _ = ops.webp_decode_files_device(mine, stream=st)
            results[t] = images
            L.ffhip_stream_destroy(st)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for t in range(2):
        check_all(results[t], order[t::2] * 3)
