"""GPU: the lossless WebP encoder on the device against the host entry ffhip_vp8l_encode_picture -- the same body compiled by
gcc, held to the numpy witness, PIL and two more decoders by tests/test_vp8l_encode_capi.py -- file for file and byte for byte: every case
in ONE mixed batch and one call per item, every source form, a BGRA picture straight from the decoder, the cap, a batch of two parts, two threads with a stream
each, the device decoder on the device's files, and tensors.encode_webp_lossless.  The scratch protocol is
tests/test_lossless_webp_encode_scratch_gpu.py's."""
import ctypes as C
import threading

import numpy as np
import pytest

import vp8l_encode_spec as spec
from ffpic_amd import capi, ops, tensors
from png_encode_cases import FORMS, source_form
from vp8l_encode_cases import CASES, LARGE, SMALL

pytestmark = pytest.mark.gpu
FILL = 0xA5
NOSPACE = capi.FFHIP_EVP8L_NOSPACE
PART_ITEMS = 4096            # ffhip_vp8l_encode_items: a part holds at most this many pictures (VE_PART_ITEMS)
HOST = {}


def host_file(case):
    if case.id not in HOST:
        HOST[case.id] = ops.vp8l_encode_picture(case.samples, case.flags)
    return HOST[case.id]


def up(n, a=256):
    return (n + a - 1) // a * a


class Arena:
    """host arrays at aligned offsets of ONE device allocation filled with 0xA5, a guard of 256 bytes behind each"""

    def __init__(self):
        self.parts, self.total = [], 256

    def add(self, nbytes, host=None):
        off = self.total
        self.parts.append((off, host))
        self.total = up(off + nbytes) + 256
        return off

    def upload(self):
        flat = np.full(self.total, FILL, np.uint8)
        for off, host in self.parts:
            if host is not None:
                flat[off:off + host.nbytes] = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.dev = ops.DeviceBuffer(host=flat)
        return self.dev.ptr

    def read(self):
        return self.dev.to_host((self.total,), np.uint8)


def encode_call(cases, form="HWC", caps=None, strict=True, stream=None, one_by_one=False):
    """-> ([what lies below cap of every file], lengths, status); asserts the 0xA5 behind every file's bytes and in front of its place"""
    arena = Arena()
    sources, outs = [], []
    for k, c in enumerate(cases):
        host, off, row, pixel, chan = source_form(c.samples, FORMS[k % len(FORMS)] if form == "mixed" else form)
        sources.append((arena.add(host.nbytes, host) + off, row, pixel, chan))
    for k, c in enumerate(cases):
        cap = ops.vp8l_encode_bound(c.width, c.height) if caps is None or caps[k] is None else caps[k]
        outs.append((arena.add(cap), cap))
    base = arena.upload()
    items = []
    for c, (off, row, pixel, chan), (out, cap) in zip(cases, sources, outs):
        it = capi.Vp8lEncodeItem()
        it.src, it.flags, it.d_out, it.cap = capi.png_source(base + off, c.width, c.height, row, pixel, chan), c.flags, (base + out) if cap else None, cap
        items.append(it)
    if one_by_one:
        lens, status = [], []
        for it in items:
            n, s = ops.vp8l_encode_items([it], stream, strict=strict)
            lens += n
            status += s
    else:
        lens, status = ops.vp8l_encode_items(items, stream, strict=strict)
    flat = arena.read()
    files = []
    for (out, cap), n in zip(outs, lens):
        end = out + min(n, cap)
        assert (flat[end:up(out + cap) + 256] == FILL).all() and (flat[out - 256:out] == FILL).all(), "bytes beside a file"
        files.append(flat[out:end].tobytes())
    return files, lens, status


def test_all_cases_in_one_call():
    """every size, channel count, content and flag, the source forms in turn, the 300 x 300 picture among them, in ONE call: the host
    entry's files, byte for byte"""
    capi.require_device()
    files, lens, status = encode_call(CASES, form="mixed")
    assert status == [0] * len(CASES)
    for c, f, n in zip(CASES, files, lens):
        want = host_file(c)
        assert n == len(want) and f == want, (c.id, n, len(want), next((i for i, (a, b) in enumerate(zip(f, want)) if a != b), None))


def test_one_call_per_item():
    capi.require_device()
    cases = SMALL[::2]
    files, _, status = encode_call(cases, one_by_one=True)
    assert status == [0] * len(cases) and files == [host_file(c) for c in cases]


@pytest.mark.parametrize("form", FORMS)
def test_every_source_form(form):
    capi.require_device()
    cases = SMALL[::3] + LARGE[:1]
    files, _, status = encode_call(cases, form=form)
    assert status == [0] * len(cases) and files == [host_file(c) for c in cases]


def test_the_device_decoder_gives_the_samples_back():
    """ffhip_vp8l_decode_files_device on the device's own files: the input samples, alpha and the colour under alpha 0 included"""
    capi.require_device()
    files, _, status = encode_call(CASES)
    assert status == [0] * len(CASES)
    infos, images, _ = ops.vp8l_decode_files_device(files)
    for c, im in zip(CASES, images):
        assert np.array_equal(im, spec.to_bgra(c.samples)), c.id


def test_a_bgra_picture_straight_from_the_decoder():
    """a file of ours, decoded by ffhip_vp8l_decode_files_device into BGRA on the device, encoded again from there with chan = {2, 1, 0, 3}
    (and with three channels, its alpha dropped): the host entry's files of the same samples"""
    capi.require_device()
    case = next(c for c in CASES if c.id == "40x36x4-colour-under-alpha-0")
    infos, images, dout = ops.vp8l_decode_files_device([host_file(case)])
    pitch = (4 * case.width + 15) & ~15
    for chan, samples in (((2, 1, 0, 3), case.samples), ((2, 1, 0), case.samples[..., :3])):
        want = ops.vp8l_encode_picture(np.ascontiguousarray(samples))
        out = ops.DeviceBuffer(host=np.full(len(want) + 256, FILL, np.uint8))
        it = capi.Vp8lEncodeItem()
        it.src, it.flags, it.d_out, it.cap = capi.png_source(dout.ptr, case.width, case.height, pitch, 4, chan), 3, out.ptr, len(want)
        lens, status = ops.vp8l_encode_items([it])
        got = out.to_host((len(want) + 256,), np.uint8)
        assert status == [0] and lens == [len(want)] and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()


def test_cap_exact_one_short_and_none():
    """FFHIP_EVP8L_NOSPACE, the length the file needs, the 0xA5 behind cap intact, the bytes below cap the file's, the neighbours whole"""
    capi.require_device()
    cases = (SMALL[1::3] + LARGE)[:12]
    wants = [host_file(c) for c in cases]
    caps = [len(w) - 1 if k % 4 == 1 else (len(w) if k % 4 == 2 else (0 if k % 4 == 3 else None)) for k, w in enumerate(wants)]
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert status == [NOSPACE if k % 4 in (1, 3) else 0 for k in range(len(cases))]
    for k, (c, w, f, n) in enumerate(zip(cases, wants, files, lens)):
        assert n == len(w), c.id
        assert f == (w[:-1] if k % 4 == 1 else (b"" if k % 4 == 3 else w)), c.id
    files, lens, status = encode_call(cases[:2], caps=[13, 29], strict=False)       # inside the RIFF header; an odd cap inside the bits
    assert status == [NOSPACE, NOSPACE] and files == [wants[0][:13], wants[1][:29]] and lens == [len(wants[0]), len(wants[1])]
    with pytest.raises(capi.FfhipError):
        encode_call(cases[:2], caps=[13, None])


def test_a_batch_of_several_parts():
    """a part holds at most 4096 pictures (ffhip_parts_run with VE_PART_ITEMS): 4096 + 5 pictures of a few pixels are two parts, with a
    picture that does not fit in the second; its status is the call's return code, and every other file is the host entry's"""
    L = capi.require_device()
    small = sorted(SMALL, key=lambda c: c.width * c.height)[:4]
    assert all(c.width * c.height <= 70 for c in small)
    cases = [small[k % len(small)] for k in range(PART_ITEMS + 5)]
    caps = [None] * len(cases)
    caps[PART_ITEMS + 2] = 30
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert [k for k, s in enumerate(status) if s] == [PART_ITEMS + 2] and status[PART_ITEMS + 2] == NOSPACE
    wants = [host_file(c) for c in small]
    assert all(len(w) > 30 for w in wants)
    for k, (f, n) in enumerate(zip(files, lens)):
        w = wants[k % len(small)]
        assert n == len(w) and f == (w[:30] if k == PART_ITEMS + 2 else w), k
    # the call's return code: the status of the picture that did not fit, from the second part
    c = cases[PART_ITEMS + 2]
    src = ops.DeviceBuffer(host=np.ascontiguousarray(c.samples))
    out = ops.DeviceBuffer(host=np.full(len(cases) * 256, FILL, np.uint8))
    items = (capi.Vp8lEncodeItem * len(cases))()
    for k, it in enumerate(items):
        it.src = capi.png_source(src.ptr, c.width, c.height, c.width * c.channels, c.channels, tuple(range(c.channels)))
        it.flags, it.d_out, it.cap = c.flags, out.ptr + 256 * k, 30 if k == PART_ITEMS + 2 else 256
    n_out, st_out = (C.c_size_t * len(cases))(), (C.c_int * len(cases))()
    assert L.ffhip_vp8l_encode_items(items, len(cases), n_out, st_out, None) == NOSPACE
    assert list(st_out) == status and list(n_out) == [len(host_file(c))] * len(cases)


def test_two_threads_a_stream_each():
    """the "Threads and streams" contract: the whole batch at once from two threads, each on a stream of its own; both give the host's files"""
    L = capi.require_device()
    wants = [host_file(c) for c in CASES]
    results, errors = {}, []

    def work(k):
        stream = L.ffhip_stream_create()
        try:
            barrier.wait()
            for _ in range(2):
                files, _, status = encode_call(CASES, form="mixed", stream=stream)
                assert status == [0] * len(CASES)
                results.setdefault(k, []).append(files)
        except BaseException as e:                                           # the main thread reports it
            errors.append(e)
        finally:
            L.ffhip_stream_destroy(stream)

    barrier = threading.Barrier(2)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(files == wants for k in range(2) for files in results[k])


def test_tensors_encode_webp_lossless_round_trips():
    """decode_webp... of encode_webp_lossless(x) is x for 1..4 channels, CHW and HWC, strided views included; the files are the host entry's"""
    import torch
    capi.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    cases = [next(c for c in CASES if c.channels == ch and c.height >= 33 and c.flags == 3) for ch in (1, 2, 3, 4)]
    pictures = []
    for k, c in enumerate(cases):
        t = torch.from_numpy(c.samples).to(dev)
        pictures.append(t if k % 2 else t.permute(2, 0, 1).contiguous())
    wide = torch.from_numpy(np.ascontiguousarray(np.concatenate([cases[2].samples, cases[2].samples], axis=1))).to(dev)
    pictures.append(wide[:, :cases[2].width])                            # a view with a padded pitch
    cases.append(cases[2])
    files = tensors.encode_webp_lossless(pictures, to_host=True)
    assert files == [host_file(c) for c in cases]
    on_device = tensors.encode_webp_lossless(pictures[:2])
    assert [bytes(f.cpu().numpy()) for f in on_device] == files[:2] and all(f.is_cuda and f.dtype == torch.uint8 and f.dim() == 1 for f in on_device)
    noise = np.random.default_rng(3).integers(0, 256, (128, 128, 4), dtype=np.uint8)     # noise takes 4.1 bytes a pixel, half the bound is 3.75 and 2 KiB
    t = torch.from_numpy(noise).to(dev)
    want = ops.vp8l_encode_picture(noise)
    assert len(want) > ops.vp8l_encode_bound(128, 128) // 2 + 256             # longer than its first cap: the second call
    assert tensors.encode_webp_lossless(t, to_host=True) == want
    plain = tensors.encode_webp_lossless([t, t], predict=[True, False], subtract_green=False, to_host=True)
    assert plain[0] == ops.vp8l_encode_picture(noise, 2) and plain[1] == ops.vp8l_encode_picture(noise, 0)
    infos, images, _ = ops.vp8l_decode_files_device(files + plain)
    for px, im in zip([c.samples for c in cases] + [noise, noise], images):
        assert np.array_equal(im, spec.to_bgra(px))


def test_argument_errors_come_before_the_device():
    import torch
    L = capi.lib()
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()

    def item(w=4, h=4, channels=3, flags=3, reserved=0, d_out=16, cap=100, src_reserved=0):
        it = capi.Vp8lEncodeItem()
        it.src = capi.png_source(16, w, h, 4 * w, 4, (0, 1, 2, 3)[:min(channels, 4)], channels)
        it.src.reserved = src_reserved
        it.flags, it.reserved, it.d_out, it.cap = flags, reserved, d_out, cap
        return it

    E = capi.FFHIP_EINVAL
    good = item()
    assert L.ffhip_vp8l_encode_items(None, 1, lens, status, None) == E and L.ffhip_vp8l_encode_items(C.byref(good), -1, lens, status, None) == E
    assert L.ffhip_vp8l_encode_items(C.byref(good), 1, None, status, None) == E and L.ffhip_vp8l_encode_items(C.byref(good), 1, lens, None, None) == E
    for bad in (item(w=0), item(h=0), item(w=16385), item(h=16385), item(channels=5), item(channels=0), item(reserved=1), item(src_reserved=1),
                item(flags=4), item(d_out=None)):
        assert L.ffhip_vp8l_encode_items(C.byref(bad), 1, lens, status, None) == E
    capi.require_device()
    assert L.ffhip_vp8l_encode_items(None, 0, None, None, None) == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    for t in (torch.zeros((5, 8, 8), dtype=torch.uint8, device=dev), torch.zeros((3, 8, 8), dtype=torch.float32, device=dev),
              torch.zeros((3, 8, 8), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8, device=dev), torch.zeros((3, 0, 8), dtype=torch.uint8, device=dev),
              torch.zeros((1, 2, 16385), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            tensors.encode_webp_lossless([t])
    with pytest.raises(ValueError):
        tensors.encode_webp_lossless([torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev)], predict="yes")
    with pytest.raises(ValueError):
        tensors.encode_webp_lossless([torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev)], subtract_green=[True, False])
    assert tensors.encode_webp_lossless([]) == []
