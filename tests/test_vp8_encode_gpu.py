"""GPU: the lossy WebP encoder on the device against the host entry ffhip_vp8_encode_picture -- the same body compiled by
gcc, held to the numpy witness, PIL and the spec decoder by tests/test_vp8_encode_capi.py -- file for file and byte for byte: every case in
ONE mixed batch, every source form, offset and non-contiguous sources, the cap with neighbours that succeed, a batch of two parts, the
device decoder on the device's files (the round trip to the reconstruction), and tensors.encode_webp.  The scratch protocol and the two
threads are tests/test_vp8_encode_scratch_gpu.py's."""
import ctypes as C

import numpy as np
import pytest

from ffpic_amd import capi, ops, tensors
from png_encode_cases import FORMS, source_form
from test_vp8l_encode_gpu import Arena, FILL, up
from vp8_encode_cases import CASES, Case, picture

pytestmark = pytest.mark.gpu
NOSPACE = capi.FFHIP_EVP8_NOSPACE
PART_ITEMS = 4096            # ffhip_vp8_encode_items: a part holds at most this many pictures (V8_PART_ITEMS)
HOST = {}


def host_file(case):
    if case.id not in HOST:
        HOST[case.id] = ops.vp8_encode_picture(case.pixels, case.quality, case.filter)
    return HOST[case.id]


def samples_of(case):
    return case.pixels if case.pixels.ndim == 3 else case.pixels[..., None]


def encode_call(cases, form="HWC", caps=None, strict=True, stream=None):
    """-> ([what lies below cap of every file], lengths, status); asserts the 0xA5 behind every file's bytes and in front of its place"""
    arena = Arena()
    sources, outs = [], []
    for k, c in enumerate(cases):
        host, off, row, pixel, chan = source_form(samples_of(c), FORMS[k % len(FORMS)] if form == "mixed" else form)
        sources.append((arena.add(host.nbytes, host) + off, row, pixel, chan))
    for k, c in enumerate(cases):
        h, w = c.pixels.shape[:2]
        cap = ops.vp8_encode_bound(w, h) if caps is None or caps[k] is None else caps[k]
        outs.append((arena.add(cap), cap))
    base = arena.upload()
    items = []
    for c, (off, row, pixel, chan), (out, cap) in zip(cases, sources, outs):
        h, w = c.pixels.shape[:2]
        it = capi.Vp8EncodeItem()
        it.src = capi.jpeg_source(base + off, w, h, row, pixel, chan, len(chan))
        it.quality, it.filter, it.d_out, it.cap = c.quality, c.filter, (base + out) if cap else None, cap
        items.append(it)
    lens, status = ops.vp8_encode_items(items, stream, strict=strict)
    flat = arena.read()
    files = []
    for (out, cap), n in zip(outs, lens):
        end = out + min(n, cap)
        assert (flat[end:up(out + cap) + 256] == FILL).all() and (flat[out - 256:out] == FILL).all(), "bytes beside a file"
        files.append(flat[out:end].tobytes())
    return files, lens, status


def test_all_cases_in_one_call():
    """every size, content, quality and filter level, the source forms in turn, in ONE call: the host entry's files, byte for byte"""
    capi.require_device()
    files, lens, status = encode_call(CASES, form="mixed")
    assert status == [0] * len(CASES)
    for c, f, n in zip(CASES, files, lens):
        want = host_file(c)
        assert n == len(want) and f == want, (c.id, n, len(want), next((i for i, (a, b) in enumerate(zip(f, want)) if a != b), None))


@pytest.mark.parametrize("form", FORMS)
def test_every_source_form(form):
    capi.require_device()
    cases = CASES[2:9:2]
    files, _, status = encode_call(cases, form=form)
    assert status == [0] * len(cases) and files == [host_file(c) for c in cases]


def test_one_nospace_between_two_that_succeed():
    """FFHIP_EVP8_NOSPACE, the length the file needs, the 0xA5 behind cap intact, the bytes below cap the file's, the neighbours whole"""
    capi.require_device()
    cases = [CASES[3], CASES[4], CASES[5], CASES[7], CASES[0]]
    wants = [host_file(c) for c in cases]
    caps = [None, len(wants[1]) - 1, len(wants[2]), 0, None]
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert status == [0, NOSPACE, 0, NOSPACE, 0] and lens == [len(w) for w in wants]
    assert files == [wants[0], wants[1][:-1], wants[2], b"", wants[4]]
    files, lens, status = encode_call(cases[:2], caps=[13, 45], strict=False)       # inside the RIFF head; inside the first partition
    assert status == [NOSPACE, NOSPACE] and files == [wants[0][:13], wants[1][:45]] and lens == [len(wants[0]), len(wants[1])]
    with pytest.raises(capi.FfhipError):
        encode_call(cases[:2], caps=[13, None])


def test_the_device_decoder_gives_the_reconstruction_back():
    """ffhip_webp_decode_files_device under libwebp's rule on the device's own files: with filter 0 its planes are the unfiltered
    reconstruction ffhip_vp8_encode_mbs returns"""
    capi.require_device()
    cases = [c for c in CASES if c.filter == 0]
    files, _, status = encode_call(cases)
    assert status == [0] * len(cases)
    out = ops.webp_decode_files_device(files, pixels="libwebp", planes=True)
    for c, (y, u, v) in zip(cases, out[-1]):
        m = ops.vp8_encode_mbs(c.pixels, c.quality)
        assert np.array_equal(y, m["y"]) and np.array_equal(u, m["u"]) and np.array_equal(v, m["v"]), c.id


def test_a_batch_of_several_parts():
    """a part holds at most 4096 pictures (ffhip_parts_run with V8_PART_ITEMS): 4096 + 5 pictures of one macroblock are two parts, with a
    picture that does not fit in the second; its status is the call's return code, and every other file is the host entry's"""
    L = capi.require_device()
    small = [Case(f"tiny{k}", picture(5 + k, 16 - k, 20 + k), (30, 75, 90)[k], (0, -1, 7)[k]) for k in range(3)]
    cases = [small[k % 3] for k in range(PART_ITEMS + 5)]
    wants = [host_file(c) for c in small]
    assert all(len(w) > 40 for w in wants)
    caps = [256] * len(cases)
    caps[PART_ITEMS + 2] = 40
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert [k for k, s in enumerate(status) if s] == [PART_ITEMS + 2] and status[PART_ITEMS + 2] == NOSPACE
    for k, (f, n) in enumerate(zip(files, lens)):
        w = wants[k % 3]
        assert n == len(w) and f == (w[:40] if k == PART_ITEMS + 2 else w), k
    c = small[0]
    src = ops.DeviceBuffer(host=np.ascontiguousarray(c.pixels))
    out = ops.DeviceBuffer(host=np.full(len(cases) * 256, FILL, np.uint8))
    items = (capi.Vp8EncodeItem * len(cases))()
    h, w = c.pixels.shape[:2]
    for k, it in enumerate(items):
        it.src = capi.jpeg_source(src.ptr, w, h, 3 * w, 3, (0, 1, 2), 3)
        it.quality, it.filter, it.d_out, it.cap = c.quality, c.filter, out.ptr + 256 * k, 40 if k == PART_ITEMS + 2 else 256
    n_out, st_out = (C.c_size_t * len(cases))(), (C.c_int * len(cases))()
    assert L.ffhip_vp8_encode_items(items, len(cases), n_out, st_out, None) == NOSPACE      # the call's return code comes from the second part
    assert list(st_out) == status and list(n_out) == [len(wants[0])] * len(cases)
    assert L.ffhip_vp8_encode_items(None, 0, None, None, None) == 0


def test_tensors_encode_webp():
    """a single tensor, a list and to_host; CHW, HWC, grey and a view with a padded pitch; qualities and filters per picture; a file longer
    than its first cap goes through the second call"""
    import torch
    capi.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    rgb, grey = CASES[3], next(c for c in CASES if c.pixels.ndim == 2)
    t_hwc = torch.from_numpy(rgb.pixels).to(dev)
    t_chw = t_hwc.permute(2, 0, 1).contiguous()
    t_grey = torch.from_numpy(grey.pixels).to(dev)[None]
    wide = torch.from_numpy(np.ascontiguousarray(np.concatenate([rgb.pixels, rgb.pixels], axis=1))).to(dev)
    view = wide[:, :rgb.pixels.shape[1]]
    want = ops.vp8_encode_picture(rgb.pixels, 75, -1)
    one = tensors.encode_webp(t_hwc)
    assert one.is_cuda and one.dtype == torch.uint8 and one.dim() == 1 and bytes(one.cpu().numpy()) == want
    files = tensors.encode_webp([t_hwc, t_chw, t_grey, view], quality=[75, 30, 50, 75], filter=[None, 0, 63, None], to_host=True)
    assert files == [want, ops.vp8_encode_picture(rgb.pixels, 30, 0), ops.vp8_encode_picture(grey.pixels, 50, 63), want]
    noise = np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    big = ops.vp8_encode_picture(noise, 100, -1)
    assert len(big) > 64 * 64 * 3 // 2 + 256                                  # longer than its first cap: the second call
    assert tensors.encode_webp(torch.from_numpy(noise).to(dev), quality=100, to_host=True) == big
    assert tensors.encode_webp([]) == []
    for bad in (dict(quality=101), dict(quality=[75, 75]), dict(filter=64), dict(quality=7.5)):
        with pytest.raises(ValueError):
            tensors.encode_webp([t_hwc], **bad)
    for t in (torch.zeros((4, 8, 8), dtype=torch.uint8, device=dev), torch.zeros((3, 8, 8), dtype=torch.float32, device=dev), torch.zeros((3, 8, 8), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            tensors.encode_webp([t])
