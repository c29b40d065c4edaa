"""GPU: lossless WebP files to device pixels and tensors.  Every case of vp8l_cases.py in one ffhip_vp8l_decode_files_device call against
the answer key, the host decoder and the witness (vp8l_spec.py), byte for byte, alpha included; the golden's files; the same call in several
parts; damaged files among good ones; a lone file over three predictor levels; the bytes beside the pictures; decode_webp_lossless_to_tensors
against the existing tensor, resize and orient stages applied to the witness's pictures.  No tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vp8l_cases
import vp8l_spec
from ffpic_amd import capi, ops, tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_vp8l as golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    capi.require_device(0)
    return [c.data for c in vp8l_cases.cases()]


@pytest.fixture(scope="module")
def witness():
    return [vp8l_spec.decode(c.data) for c in vp8l_cases.cases()]


def check_all(images, witness):
    for c, got, want, wit in zip(vp8l_cases.cases(), images, vp8l_cases.expected(), witness):
        assert got is not None and got.shape == want.shape, c.name
        assert np.array_equal(got, want), (c.name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, ops.vp8l_picture(c.data)) and np.array_equal(got, wit), c.name


def test_all_cases_in_one_call(files, witness):
    infos, images, _ = ops.vp8l_decode_files_device(files)
    check_all(images, witness)
    cs = vp8l_cases.cases()
    assert ops.vp8l_last() == (1, max(vp8l_cases.levels_of(c) for c in cs), sum(c.host for c in cs))
    for c, info in zip(cs, infos):
        assert (info.width, info.height, info.has_alpha) == (c.argb.shape[1], c.argb.shape[0], int(c.alpha)), c.name
        assert tuple(info.transforms[:info.n_transforms]) == c.types and (info.cache_bits, info.has_meta) == (c.cache_bits, int(c.meta)), c.name


def test_the_goldens_files_give_the_goldens_pixels():
    capi.require_device(0)
    stored = golden.load()
    _, images, _ = ops.vp8l_decode_files_device([d for _, d, _ in stored])
    for (name, _, pixels), got in zip(stored, images):
        assert np.array_equal(got, pixels), name


def test_several_parts_give_the_same_pictures(files, witness, monkeypatch):
    monkeypatch.setenv("FFHIP_VP8L_PART_BYTES", "6000")              # the largest file is a part of its own
    capi.reload_env()
    _, images, _ = ops.vp8l_decode_files_device(files, n_threads=3)
    assert ops.vp8l_last()[0] >= 8
    check_all(images, witness)


def test_damaged_files_are_their_files_alone(files):
    bad = {d.name: d.data for d in vp8l_cases.damaged_cases()}
    batch = list(files[:6])
    batch.insert(1, bad["over-subscribed"])
    batch.insert(3, bad["distance-beyond-start"])
    batch.append(bad["prefix-transforms-400"])
    _, images, _, status = ops.vp8l_decode_files_device(batch, strict=False)
    assert [k for k, s in enumerate(status) if s] == [1, 3, 8] and all(status[k] == capi.FFHIP_EINVAL for k in (1, 3, 8))
    good = [im for k, im in enumerate(images) if k not in (1, 3, 8)]
    assert all(images[k] is None for k in (1, 3, 8))
    for got, want in zip(good, vp8l_cases.expected()[:6]):
        assert np.array_equal(got, want)
    with pytest.raises(capi.FfhipError):
        ops.vp8l_decode_files_device(batch)


def test_a_lone_file_over_its_levels():
    capi.require_device(0)
    k = [c.name for c in vp8l_cases.cases()].index("size-65x130")
    _, images, _ = ops.vp8l_decode_files_device([vp8l_cases.cases()[k].data])
    assert np.array_equal(images[0], vp8l_cases.expected()[k])
    assert ops.vp8l_last() == (1, 3, 0)


def test_bytes_beside_the_pictures_keep_a_sentinel(files):
    """every picture in a frame of its own: 16 bytes wider than its rows and two rows higher, filled with a sentinel"""
    cs = vp8l_cases.cases()
    pitches = [((4 * c.argb.shape[1] + 15) & ~15) + 16 for c in cs]
    offs, total = [], 0
    for c, p in zip(cs, pitches):
        offs.append(total + p)                                        # a row of sentinel above
        total += p * (c.argb.shape[0] + 2)
    dev = ops.DeviceBuffer(host=np.full(total, 0xA5, np.uint8))
    n = len(cs)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * n)(*[dev.ptr + o for o in offs])
    status = (C.c_int * n)()
    rc = capi.lib().ffhip_vp8l_decode_files_device(ptrs, lens, n, 4, outs, (C.c_int64 * n)(*pitches), None, status, None)
    assert rc == 0 and not any(status)
    flat = dev.to_host((total,), np.uint8)
    for c, p, o, want in zip(cs, pitches, offs, vp8l_cases.expected()):
        h, w = c.argb.shape
        frame = flat[o - p:o + p * (h + 1)].reshape(h + 2, p)
        assert np.array_equal(frame[1:h + 1, :4 * w].reshape(h, w, 4), want), c.name
        assert (frame[0] == 0xA5).all() and (frame[h + 1] == 0xA5).all() and (frame[1:h + 1, 4 * w:] == 0xA5).all(), c.name


class Reference:
    """the witness's pictures on the device, and tensors made of them by the existing stages"""
    def __init__(self, pics):
        import torch
        self.torch = torch
        self.pics = pics
        self.offs, total = [], 0
        for p in self.pics:
            self.offs.append(total)
            total += (p.nbytes + 15) & ~15
        flat = np.zeros(total, np.uint8)
        for p, o in zip(self.pics, self.offs):
            flat[o:o + p.nbytes] = p.reshape(-1)
        self.dev = ops.DeviceBuffer(host=flat)
        self.fmt = tensors.tensor_format()
        self.keep = []

    def src(self, k):
        h, w, _ = self.pics[k].shape
        return self.dev.ptr + self.offs[k], 4 * w, w, h

    def scratch(self, nbytes):
        self.keep.append(ops.DeviceBuffer(nbytes=nbytes))
        return self.keep[-1].ptr

    def to_tensors(self, views):
        """views [(ptr, pitch, x0, y0, w, h)] -> [uint8 CHW tensors]"""
        outs = [self.torch.empty((3, h, w), dtype=self.torch.uint8, device="cuda") for _, _, _, _, w, h in views]
        tensors.bgra_to_tensors([capi.TensorItem(p, pitch, x0, y0, w, h, t.data_ptr(), w, w * h) for (p, pitch, x0, y0, w, h), t in zip(views, outs)], self.fmt)
        capi.sync()
        return outs


# the tensor tests take the cases that are at least 5 x 3, so that a rectangle inside them has pixels
BIG = [k for k, c in enumerate(vp8l_cases.cases()) if c.argb.shape[1] >= 5 and c.argb.shape[0] >= 3]


@pytest.fixture(scope="module")
def ref(files, witness):
    pytest.importorskip("torch")
    return Reference([witness[k] for k in BIG])


@pytest.fixture(scope="module")
def big(files):
    return [files[k] for k in BIG]


def same(ref, got, want):
    assert len(got) == len(want)
    for k, g, w in zip(BIG, got, want):
        assert g.shape == w.shape and ref.torch.equal(g, w), vp8l_cases.cases()[k].name


def test_tensors_plain(big, ref):
    views = [(p, pitch, 0, 0, w, h) for p, pitch, w, h in (ref.src(k) for k in range(len(big)))]
    same(ref, tensors.decode_webp_lossless_to_tensors(big), ref.to_tensors(views))


def test_tensors_roi(big, ref):
    rois, views = [], []
    for k in range(len(big)):
        p, pitch, w, h = ref.src(k)
        r = (w // 3, h // 4, w - w // 3 - w // 5, h - h // 4 - h // 6)
        rois.append(r)
        views.append((p, pitch) + r)
    same(ref, tensors.decode_webp_lossless_to_tensors(big, roi=rois), ref.to_tensors(views))


@pytest.mark.parametrize("antialias", [True, False])
def test_tensors_resized(big, ref, antialias):
    items, views = [], []
    for k in range(len(big)):
        p, pitch, w, h = ref.src(k)
        dst = ref.scratch(4 * 32 * 32)
        items.append(capi.ResizeItem(p, pitch, 0, 0, w, h, dst, 128, 32, 32))
        views.append((dst, 128, 0, 0, 32, 32))
    tensors.resize_bgra(items, antialias=antialias)
    got = tensors.decode_webp_lossless_to_tensors(big, size=(32, 32), antialias=antialias, stack=True)
    assert tuple(got.shape) == (len(big), 3, 32, 32)
    same(ref, list(got), ref.to_tensors(views))


def test_tensors_upright(big, ref):
    """apply_exif_orientation: the file with an EXIF chunk of orientation 6 is turned, the others are not"""
    items, views, want_turns = [], [], []
    for j, k in enumerate(BIG):
        p, pitch, w, h = ref.src(j)
        o = vp8l_cases.cases()[k].orientation
        want_turns.append(o)
        dst = ref.scratch(4 * w * h)
        items.append(capi.OrientItem(p, pitch, 0, 0, w, h, dst, 4 * (h if o >= 5 else w), o))
        views.append((dst, 4 * (h if o >= 5 else w), 0, 0, h if o >= 5 else w, w if o >= 5 else h))
    tensors.orient_bgra(items)
    got, turns = tensors.decode_webp_lossless_to_tensors(big, apply_exif_orientation=True, return_orientation=True)
    assert turns == want_turns and 6 in turns
    same(ref, got, ref.to_tensors(views))
