"""GPU: the PNG file calls with FFHIP_PNG_INFLATE_DEVICE -- k_inflate instead of the host threads' inflate.  Every case of png_cases.py
in one ffhip_png_decode_files_device_ex call against the witness and the host decoder; in parts; the same pictures written with other
streams and IDAT cuts; damaged files, whose codes have to be the host path's and whose places stay untouched; the tensor call against
itself with inflate='host', bit for bit; the switch FFHIP_PNG_INFLATE_GPU under the tests of test_png_gpu.py; the scratch protocol and
two threads on streams of their own.  No tolerance anywhere."""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import png_cases
import png_writer as W
import scratch_fill as SF
import test_png_gpu as HOST
from ffpic_amd import capi, ops, tensors

pytestmark = pytest.mark.gpu
DEVICE = capi.FFHIP_PNG_INFLATE_DEVICE
SHORT_PALETTE = ("pal4_short", "pal8_trns_short")


@pytest.fixture(scope="module")
def files():
    capi.require_device(0)
    return [c.data for c in png_cases.cases()]


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    for name in ("FFHIP_PNG_PART_BYTES", "FFHIP_PNG_INFLATE_GPU", "FFHIP_PNG_TIMES"):
        capi.setenv(name, None)


def test_all_cases_in_one_call(files):
    _, host_images, _ = ops.png_decode_files_device(files)
    host_last = ops.png_last()
    assert ops.png_inflate_last()[:3] == (0, len(files), 0)
    infos, images, _ = ops.png_decode_files_device(files, inflate="device")
    HOST.check_all(images)
    assert ops.png_last() == host_last == (1, max(HOST.levels_of(f) for f in files))
    names = [c.name for c in png_cases.cases()]
    assert len(files) == 50 and all(n in names for n in SHORT_PALETTE)
    on_device, on_host, uploaded, ms = ops.png_inflate_last()
    assert (on_device, on_host) == (48, 2) and ms == 0                # the two short palettes go the host way; no clock without the switch
    assert uploaded == sum(len(idat(c.data)) for c in png_cases.cases() if c.name not in SHORT_PALETTE)
    for c, info in zip(png_cases.cases(), infos):
        assert (info.width, info.height, info.bit_depth, info.color_type) == (c.samples.shape[1], c.samples.shape[0], c.depth, c.ctype)


def idat(data):
    """the IDAT payloads of a file, joined"""
    out, at = b"", 8
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        if data[at + 4:at + 8] == b"IDAT":
            out += data[at + 8:at + 8 + n]
        at += n + 12
    return out


def test_the_clock_keeps_the_inflate_apart(files):
    capi.setenv("FFHIP_PNG_TIMES", 1)
    _, images, _ = ops.png_decode_files_device(files, inflate="device")
    HOST.check_all(images)
    assert ops.png_inflate_last()[3] > 0 and all(t > 0 for t in ops.png_times())


def test_several_parts_give_the_same_pictures(files):
    capi.setenv("FFHIP_PNG_PART_BYTES", 30000)                        # the largest file is a part of its own
    ops.png_decode_files_device(files, n_threads=3)
    host_last = ops.png_last()
    _, images, _ = ops.png_decode_files_device(files, n_threads=3, inflate="device")
    assert ops.png_last() == host_last and host_last[0] >= 8          # the budget sums filtered bytes either way
    assert ops.png_inflate_last()[:2] == (48, 2)
    HOST.check_all(images)


def test_other_streams_and_idat_cuts(files):
    """the same pictures, their streams made at levels 0, 1 and 9, with fixed codes and with a 512-byte window, cut into IDAT chunks of
    1, 7 and the rest -- all in one call"""
    batch, keys = [], []
    hows = (dict(level=0), dict(level=1), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(wbits=9))
    for how in hows:
        for k, c in enumerate(png_cases.cases()):
            batch.append(W.write(c.samples, c.ctype, c.depth, filters=[(k + r) % 5 for r in range(7)], interlace=c.interlace, palette=c.palette,
                                 trns=c.trns, idat_sizes=(1, 7, 0), **how))
            keys.append(png_cases.expected()[k])
    _, images, _ = ops.png_decode_files_device(batch, inflate="device")
    assert ops.png_inflate_last()[:2] == (48 * len(hows), 2 * len(hows))
    for k, (got, want) in enumerate(zip(images, keys)):
        assert got is not None and np.array_equal(got, want), (k // 50, png_cases.cases()[k % 50].name)


def test_bytes_beyond_the_picture():
    rng = np.random.default_rng(5)
    s = png_cases.random_samples(rng, 40, 60, 6, 8)
    raw = W.filtered_stream(s, 6, 8, [4, 1, 3, 2])
    batch = [W.write(s, 6, 8, stream=raw + b"\x07" * 40), W.write(s, 6, 8, stream=raw + bytes(range(256)) * 300, level=1), W.write(s, 6, 8, stream=raw)]
    _, host, _, host_status = ops.png_decode_files_device(batch, strict=False)
    _, dev, _, dev_status = ops.png_decode_files_device(batch, strict=False, inflate="device")
    assert host_status == dev_status == [0, 0, 0]
    for h, d in zip(host, dev):
        assert np.array_equal(h, d) and np.array_equal(d, W.expected_bgra(s, 6, 8))


def runner(files, keys, s, statuses=None, png_flags=DEVICE, n_threads=4):
    """a checked run through ffhip_png_decode_files_device_ex: every picture in a frame of 0xA5 of its own, against its key; a refused
    file's place, like every frame, has to hold its 0xA5"""
    L = capi.lib()
    sizes = [(7, 6) if k is None else (k.shape[1], k.shape[0]) for k in keys]
    places = [(4 * w, h) for w, h in sizes]

    def run():
        rc, status = SF.files_call(lambda ptrs, lens, n, outs, pitches, status: L.ffhip_png_decode_files_device_ex(
            ptrs, lens, n, n_threads, outs, pitches, None, status, png_flags, SF.h(s)), files, places, keys, statuses)
        capi.sync(SF.h(s))
        return status
    return run


def damaged_batch():
    good, keys = [c.data for c in png_cases.cases()[:6]], list(png_cases.expected()[:6])
    files, want = [], []
    for k, (_, data) in enumerate(png_cases.damaged()):
        files += [good[k % 6], data]
        want += [keys[k % 6], None]
    return files, want


def test_damaged_files_get_the_host_paths_codes_and_write_nothing():
    capi.require_device(0)
    files, keys = damaged_batch()
    host = runner(files, keys, None, png_flags=0)()
    assert [s != 0 for s in host] == [k is None for k in keys]
    got = runner(files, keys, None, {i: code for i, code in enumerate(host) if code})()
    assert got == host
    assert ops.png_inflate_last()[0] > 0


def test_tensors_equal_the_host_paths_bit_for_bit(files):
    torch = pytest.importorskip("torch")
    rois = [(w // 3, h // 4, w - w // 3 - w // 5, h - h // 4 - h // 6) for h, w in (e.shape[:2] for e in png_cases.expected())]
    for kw in (dict(), dict(roi=rois), dict(size=(32, 32)), dict(alpha="straight"), dict(orientation=6)):
        host = tensors.decode_png_to_tensors(files, **kw)
        assert ops.png_inflate_last()[0] == 0
        dev = tensors.decode_png_to_tensors(files, inflate="device", **kw)
        assert ops.png_inflate_last()[:2] == (48, 2), kw
        assert len(host) == len(dev) == len(files)
        for c, h, d in zip(png_cases.cases(), host, dev):
            assert h.shape == d.shape and h.dtype == d.dtype and torch.equal(h, d), (kw.keys(), c.name)


def test_the_switch_puts_the_old_entries_on_the_device_path(files, monkeypatch):
    """FFHIP_PNG_INFLATE_GPU=1: the tests of test_png_gpu.py, which know nothing of the flag, over k_inflate"""
    pytest.importorskip("torch")
    capi.setenv("FFHIP_PNG_INFLATE_GPU", 1)
    HOST.test_all_cases_in_one_call(files)
    assert ops.png_inflate_last()[:2] == (48, 2)
    HOST.test_several_parts_give_the_same_pictures(files, monkeypatch)
    capi.setenv("FFHIP_PNG_PART_BYTES", None)
    HOST.test_damaged_files_are_their_files_alone(files)
    for name in ("adam7_rgba16_65x130", "c6d16_65x130"):
        HOST.test_a_lone_file_over_its_levels(name)
        assert ops.png_inflate_last()[:2] == (1, 0)
    ref = HOST.Reference()
    HOST.test_tensors_plain(files, ref)
    HOST.test_tensors_roi(files, ref)
    for antialias in (True, False):
        HOST.test_tensors_resized(files, ref, antialias)
    HOST.test_tensors_turned(files, ref)
    assert ops.png_inflate_last()[0] > 0
    capi.setenv("FFHIP_PNG_INFLATE_GPU", 0)                           # "0" changes nothing
    ops.png_decode_files_device(files[:3])
    assert ops.png_inflate_last()[:2] == (0, 3)


def test_scratch_protocol_over_the_device_path(files):
    L = capi.require_device(0)
    s = L.ffhip_stream_create()
    assert s
    keys = list(png_cases.expected())
    everything = runner(files, keys, s)
    dfiles, dkeys = damaged_batch()
    damaged = runner(dfiles, dkeys, s, {i: capi.FFHIP_EINVAL for i, k in enumerate(dkeys) if k is None})

    def in_parts():
        capi.setenv("FFHIP_PNG_PART_BYTES", 1)                        # every file a part of its own: they reuse the staging
        everything()
        assert ops.png_last()[0] == len(files)
        capi.setenv("FFHIP_PNG_PART_BYTES", None)
    SF.run_protocol("png files, inflate on the device", s, [everything], [everything, in_parts, damaged], ["SCRATCH_PNG"])
    L.ffhip_stream_destroy(s)


def test_two_threads_on_their_own_streams(files):
    """two threads, each with a stream it made, decode different halves of the case list over the device path in three rounds behind a
    barrier, every picture against its key; each fills its own stream's scratch with 0xFF between the rounds"""
    L = capi.require_device(0)
    keys = list(png_cases.expected())
    barrier, errors = threading.Barrier(2), []

    def work(t):
        try:
            capi.require_device(0)
            s = L.ffhip_stream_create()
            assert s
            run = runner(files[t::2], keys[t::2], s)
            for rnd in range(3):
                barrier.wait(timeout=60)
                run()
                assert ops.png_inflate_last()[0] == len(files[t::2]) - 1          # one short palette in either half
                if rnd < 2:
                    dev, host, kinds = SF.fill(s, 0xFF)
                    assert dev > 0 and host > 0 and "SCRATCH_PNG" in {SF.base_of(k) for k in kinds}
            L.ffhip_stream_destroy(s)
        except BaseException as e:  # noqa: BLE001 -- reported below, on the main thread
            errors.append((t, e))
            barrier.abort()

    names = [c.name for c in png_cases.cases()]
    assert {names.index(n) % 2 for n in SHORT_PALETTE} == {0, 1}
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
