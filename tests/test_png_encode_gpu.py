"""GPU: the PNG encoder on the device against the host entry ffhip_png_encode_picture -- the same bodies compiled by gcc, held
to the numpy witness, zlib and PIL by tests/test_png_encode_capi.py -- file for file and byte for byte: mixed batches in ONE call and one
call per item, every source form, a BGRA picture straight from the PNG decoder, the cap, a batch of several parts, the scratch, a second
stream, and tensors.encode_png through the library's own decoders with the host and the device inflate.  No PIL here."""
import ctypes as C

import numpy as np
import pytest

import png_encode_spec as spec
import scratch_fill as SF
import stream_order as SO
from ffpic_amd import capi, ops, tensors
from png_encode_cases import CASES, FORMS, LARGE, SMALL, source_form

pytestmark = pytest.mark.gpu
FILL = 0xA5
NOSPACE = capi.FFHIP_EPNG_NOSPACE
PART_ITEMS = 4096            # ffhip_png_encode_items: a part holds at most this many pictures (include/ffpic_hip.h)
HOST = {}


def host_file(case):
    if case.id not in HOST:
        HOST[case.id] = ops.png_encode_picture(case.samples, case.filter)
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
        cap = ops.png_encode_bound(c.width, c.height, c.channels) if caps is None or caps[k] is None else caps[k]
        outs.append((arena.add(cap), cap))
    base = arena.upload()
    items = []
    for c, (off, row, pixel, chan), (out, cap) in zip(cases, sources, outs):
        it = capi.PngEncodeItem()
        it.src, it.filter, it.d_out, it.cap = capi.png_source(base + off, c.width, c.height, row, pixel, chan), c.filter, (base + out) if cap else None, cap
        items.append(it)
    if one_by_one:
        lens, status = [], []
        for it in items:
            n, s = ops.png_encode_items([it], stream, strict=strict)
            lens += n
            status += s
    else:
        lens, status = ops.png_encode_items(items, stream, strict=strict)
    flat = arena.read()
    files = []
    for (out, cap), n in zip(outs, lens):
        end = out + min(n, cap)
        assert (flat[end:up(out + cap) + 256] == FILL).all() and (flat[out - 256:out] == FILL).all(), "bytes beside a file"
        files.append(flat[out:end].tobytes())
    return files, lens, status


def test_all_cases_in_one_call():
    """every channel count, size, content and filter, the source forms in turn, in ONE call: the host entry's files, byte for byte"""
    capi.require_device()
    files, lens, status = encode_call(CASES, form="mixed")
    assert status == [0] * len(CASES)
    for c, f, n in zip(CASES, files, lens):
        want = host_file(c)
        assert n == len(want) and f == want, (c.id, n, len(want), next((i for i, (a, b) in enumerate(zip(f, want)) if a != b), None))


def test_one_call_per_item():
    capi.require_device()
    files, _, status = encode_call(CASES, one_by_one=True)
    assert status == [0] * len(CASES) and files == [host_file(c) for c in CASES]


@pytest.mark.parametrize("form", FORMS)
def test_every_source_form(form):
    capi.require_device()
    cases = SMALL[::2] + LARGE[::5]
    files, _, status = encode_call(cases, form=form)
    assert status == [0] * len(cases) and files == [host_file(c) for c in cases]


def test_a_bgra_picture_straight_from_the_decoder():
    """a file of ours, decoded by ffhip_png_decode_files_device into BGRA on the device, encoded again from there with chan = {2, 1, 0, 3}
    (and with three channels, its alpha dropped): the host entry's files of the same samples"""
    capi.require_device()
    case = next(c for c in CASES if c.channels == 4 and c.height > 8)
    infos, images, dout = ops.png_decode_files_device([host_file(case)])
    assert np.array_equal(images[0], spec.to_bgra(case.samples))
    pitch = (4 * case.width + 15) & ~15
    for chan, samples in (((2, 1, 0, 3), case.samples), ((2, 1, 0), case.samples[..., :3])):
        want = ops.png_encode_picture(np.ascontiguousarray(samples))
        out = ops.DeviceBuffer(host=np.full(len(want) + 256, FILL, np.uint8))
        it = capi.PngEncodeItem()
        it.src, it.filter, it.d_out, it.cap = capi.png_source(dout.ptr, case.width, case.height, pitch, 4, chan), spec.ADAPTIVE, out.ptr, len(want)
        lens, status = ops.png_encode_items([it])
        got = out.to_host((len(want) + 256,), np.uint8)
        assert status == [0] and lens == [len(want)] and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()


def test_cap_exact_one_short_and_none():
    """FFHIP_EPNG_NOSPACE, the length the file needs, the 0xA5 behind cap intact, the bytes below cap the file's, the neighbours whole"""
    capi.require_device()
    cases = (SMALL[1::5] + LARGE[::6])[:12]
    wants = [host_file(c) for c in cases]
    caps = [len(w) - 1 if k % 4 == 1 else (len(w) if k % 4 == 2 else (0 if k % 4 == 3 else None)) for k, w in enumerate(wants)]
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert status == [NOSPACE if k % 4 in (1, 3) else 0 for k in range(len(cases))]
    for k, (c, w, f, n) in enumerate(zip(cases, wants, files, lens)):
        assert n == len(w), c.id
        assert f == (w[:-1] if k % 4 == 1 else (b"" if k % 4 == 3 else w)), c.id
    files, lens, status = encode_call(cases[:2], caps=[20, 40], strict=False)       # inside IHDR; inside the first IDAT's head
    assert status == [NOSPACE, NOSPACE] and files == [wants[0][:20], wants[1][:40]]
    with pytest.raises(capi.FfhipError):
        encode_call(cases[:2], caps=[20, None])


def test_a_batch_of_several_parts():
    """a part holds at most 4096 pictures: 2 x 4096 + 5 small pictures are three parts, with a picture that does not fit in the second"""
    capi.require_device()
    small = [c for c in SMALL if c.samples.size <= 64][:8]
    cases = [small[k % len(small)] for k in range(2 * PART_ITEMS + 5)]
    caps = [None] * len(cases)
    caps[PART_ITEMS + 7] = 30
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert [k for k, s in enumerate(status) if s] == [PART_ITEMS + 7] and status[PART_ITEMS + 7] == NOSPACE
    wants = [host_file(c) for c in small]
    for k, (f, n) in enumerate(zip(files, lens)):
        w = wants[k % len(small)]
        assert n == len(w) and f == (w[:30] if k == PART_ITEMS + 7 else w), k


def test_the_scratch_is_no_input():
    """the protocol of tests/scratch_fill.py on a stream of its own: the library's scratch overwritten between calls, the files the same"""
    L = SF.lib()
    stream = L.ffhip_stream_create()
    try:
        def run(cases, form):
            def case():
                files, _, status = encode_call(cases, form=form, stream=stream)
                assert status == [0] * len(cases) and files == [host_file(c) for c in cases]
            return case
        small = SMALL[::5]
        SF.run_protocol("png_encode", stream, [run(LARGE + SMALL[::3], "HWC")], [run(small, "CHW"), run(small[:3], "mixed")], kinds=("SCRATCH_PNG_ENC",))
    finally:
        L.ffhip_stream_destroy(stream)


def test_on_a_second_stream():
    """The call synchronises, so the stalled scenario of tests/stream_order.py does not apply; its operands and copies do.  On a stream of
    its own the picture arrives by a copy enqueued in front of the call and is overwritten by one enqueued behind it, the file leaves by a
    copy enqueued behind the call, and nothing waits in between: a call that worked on another stream would read the decoy."""
    L = capi.require_device()
    case = next(c for c in LARGE if c.channels == 3)
    want = host_file(case)
    stream = L.ffhip_stream_create()
    try:
        px = SO.Operand(case.samples, 255 - case.samples)
        out = SO.Output(len(want))
        it = capi.PngEncodeItem()
        it.src = capi.png_source(px.ptr, case.width, case.height, case.width * 3, 3, (0, 1, 2))
        it.filter, it.d_out, it.cap = case.filter, out.ptr, len(want)
        SO.copy(px.dev.ptr, px.true.ptr, px.nbytes, stream)
        lens, status = ops.png_encode_items([it], stream)
        SO.copy(out.copy.ptr, out.dev.ptr, out.nbytes, stream)
        SO.copy(px.dev.ptr, px.decoy.ptr, px.nbytes, stream)
        capi.sync(stream)
        assert status == [0] and lens == [len(want)] and out.copied().tobytes() == want
    finally:
        L.ffhip_stream_destroy(stream)


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_tensors_encode_png_round_trips(inflate):
    """decode_png_to_tensors(encode_png(x), alpha='straight') is x for 1..4 channels, CHW and HWC, strided views included; the files are the
    host entry's"""
    import torch
    capi.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    cases = [next(c for c in CASES if c.channels == ch and c.height >= 33) for ch in (1, 2, 3, 4)] + [next(c for c in CASES if c.id.startswith("910x9x4"))]
    pictures = []
    for k, c in enumerate(cases):
        t = torch.from_numpy(c.samples).to(dev)
        pictures.append(t if k % 2 and c.height > 4 else t.permute(2, 0, 1).contiguous())
    wide = torch.from_numpy(np.ascontiguousarray(np.concatenate([cases[2].samples, cases[2].samples], axis=1))).to(dev)
    pictures.append(wide[:, :cases[2].width])                            # a view with a padded pitch
    cases.append(cases[2])
    files = tensors.encode_png(pictures, to_host=True)
    assert files == [host_file(c) for c in cases]
    on_device = tensors.encode_png(pictures[:2])
    assert [bytes(f.cpu().numpy()) for f in on_device] == files[:2] and all(f.is_cuda and f.dtype == torch.uint8 and f.dim() == 1 for f in on_device)
    noisy = next(c for c in CASES if c.id == "100x64x4-noise-filter4")   # longer than half its bound: the second call
    assert tensors.encode_png(torch.from_numpy(noisy.samples).to(dev), filter="paeth", to_host=True) == host_file(noisy)
    files, cases = files + [host_file(noisy)], cases + [noisy]            # stored blocks for the decoders as well
    decoded = tensors.decode_png_to_tensors(files, layout="HWC", alpha="straight", inflate=inflate)
    for c, d in zip(cases, decoded):
        assert np.array_equal(d.cpu().numpy(), spec.to_bgra(c.samples)[..., [2, 1, 0, 3]]), c.id
    infos, images, _ = ops.png_decode_files_device(files, inflate=inflate)
    for c, im in zip(cases, images):
        assert np.array_equal(im, spec.to_bgra(c.samples)), c.id


def test_argument_errors_come_before_the_device():
    import torch
    L = capi.lib()
    lens, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    good = capi.PngEncodeItem()
    good.src, good.filter, good.d_out, good.cap = capi.png_source(16, 4, 4, 12, 3, (0, 1, 2)), 5, 16, 100
    E = capi.FFHIP_EINVAL
    assert L.ffhip_png_encode_items(None, 1, lens, status, None) == E and L.ffhip_png_encode_items(C.byref(good), -1, lens, status, None) == E
    assert L.ffhip_png_encode_items(C.byref(good), 1, None, status, None) == E and L.ffhip_png_encode_items(C.byref(good), 1, lens, None, None) == E
    for field, value in (("reserved", 1), ("filter", 6), ("d_out", None)):
        bad = capi.PngEncodeItem()
        bad.src, bad.filter, bad.d_out, bad.cap = good.src, good.filter, good.d_out, good.cap
        setattr(bad, field, value)
        assert L.ffhip_png_encode_items(C.byref(bad), 1, lens, status, None) == E, field
    bad = capi.PngEncodeItem()
    bad.src, bad.filter, bad.d_out, bad.cap = capi.png_source(16, 65535, 65535, 65535, 1, (0,)), 5, 16, 100      # the bound reaches 2^32
    assert L.ffhip_png_encode_items(C.byref(bad), 1, lens, status, None) == E
    capi.require_device()
    assert L.ffhip_png_encode_items(None, 0, None, None, None) == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    for t in (torch.zeros((5, 8, 8), dtype=torch.uint8, device=dev), torch.zeros((3, 8, 8), dtype=torch.float32, device=dev),
              torch.zeros((3, 8, 8), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8, device=dev), torch.zeros((3, 0, 8), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            tensors.encode_png([t])
    with pytest.raises(ValueError):
        tensors.encode_png([torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev)], filter="best")
    with pytest.raises(ValueError):
        tensors.encode_png([torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev)], filter=[0, 1])
    assert tensors.encode_png([]) == []
