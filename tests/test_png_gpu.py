"""GPU: PNG files to device pixels and tensors.  Every case of png_cases.py in one ffhip_png_decode_files_device call against the witness
(png_spec.py) and against the host decoder, byte for byte, alpha included; the same call in several parts; damaged files among good ones;
a lone file over several unfilter levels; decode_png_to_tensors against the existing tensor, resize and orient stages applied to the
witness's pictures.  No tolerance anywhere."""
import numpy as np
import pytest

import png_cases
import png_spec
from ffpic_amd import capi, ops, tensors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    capi.require_device(0)
    return [c.data for c in png_cases.cases()]


def check_all(images):
    for c, got, want in zip(png_cases.cases(), images, png_cases.expected()):
        assert got is not None and got.shape == want.shape, c.name
        assert np.array_equal(got, want), (c.name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, ops.png_picture(c.data)), c.name


def levels_of(data):
    return max((r + 63) // 64 for r in png_spec.layout(data)["pass_rows"])


def test_all_cases_in_one_call(files):
    infos, images, _ = ops.png_decode_files_device(files)
    check_all(images)
    parts, launches = ops.png_last()
    assert parts == 1 and launches == max(levels_of(f) for f in files)
    for c, info in zip(png_cases.cases(), infos):
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (c.samples.shape[1], c.samples.shape[0], c.depth, c.ctype, int(c.interlace))


def test_several_parts_give_the_same_pictures(files, monkeypatch):
    monkeypatch.setenv("FFHIP_PNG_PART_BYTES", "30000")               # the largest file is a part of its own
    capi.reload_env()
    _, images, _ = ops.png_decode_files_device(files, n_threads=3)
    assert ops.png_last()[0] >= 8
    check_all(images)


def test_damaged_files_are_their_files_alone(files):
    bad = dict(png_cases.damaged())
    batch = list(files[:6])
    batch.insert(1, bad["filter_byte_5"])
    batch.insert(3, bad["crc_idat"])
    batch.append(bad["index_beyond_plte"])
    _, images, _, status = ops.png_decode_files_device(batch, strict=False)
    assert [k for k, s in enumerate(status) if s] == [1, 3, 8] and all(status[k] == capi.FFHIP_EINVAL for k in (1, 3, 8))
    good = [im for k, im in enumerate(images) if k not in (1, 3, 8)]
    assert all(images[k] is None for k in (1, 3, 8))
    for got, want in zip(good, png_cases.expected()[:6]):
        assert np.array_equal(got, want)
    with pytest.raises(capi.FfhipError):
        ops.png_decode_files_device(batch)


@pytest.mark.parametrize("name", ["adam7_rgba16_65x130", "c6d16_65x130"])
def test_a_lone_file_over_its_levels(name):
    k = [c.name for c in png_cases.cases()].index(name)
    data = png_cases.cases()[k].data
    _, images, _ = ops.png_decode_files_device([data])
    assert np.array_equal(images[0], png_cases.expected()[k])
    assert ops.png_last() == (1, levels_of(data)) and levels_of(data) == (3 if name.startswith("c6") else 2)


class Reference:
    """the witness's pictures on the device, and tensors made of them by the existing stages"""
    def __init__(self):
        import torch
        self.torch = torch
        self.pics = png_cases.expected()
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


@pytest.fixture(scope="module")
def ref(files):
    pytest.importorskip("torch")
    return Reference()


def same(ref, got, want):
    assert len(got) == len(want)
    for c, g, w in zip(png_cases.cases(), got, want):
        assert g.shape == w.shape and ref.torch.equal(g, w), c.name


def test_tensors_plain(files, ref):
    views = [(p, pitch, 0, 0, w, h) for p, pitch, w, h in (ref.src(k) for k in range(len(files)))]
    same(ref, tensors.decode_png_to_tensors(files), ref.to_tensors(views))


def test_tensors_roi(files, ref):
    rois, views = [], []
    for k in range(len(files)):
        p, pitch, w, h = ref.src(k)
        r = (w // 3, h // 4, w - w // 3 - w // 5, h - h // 4 - h // 6)
        rois.append(r)
        views.append((p, pitch) + r)
    same(ref, tensors.decode_png_to_tensors(files, roi=rois), ref.to_tensors(views))


@pytest.mark.parametrize("antialias", [True, False])
def test_tensors_resized(files, ref, antialias):
    items, views = [], []
    for k in range(len(files)):
        p, pitch, w, h = ref.src(k)
        dst = ref.scratch(4 * 32 * 32)
        items.append(capi.ResizeItem(p, pitch, 0, 0, w, h, dst, 128, 32, 32))
        views.append((dst, 128, 0, 0, 32, 32))
    tensors.resize_bgra(items, antialias=antialias)
    got = tensors.decode_png_to_tensors(files, size=(32, 32), antialias=antialias, stack=True)
    assert tuple(got.shape) == (len(files), 3, 32, 32)
    same(ref, list(got), ref.to_tensors(views))


def test_tensors_turned(files, ref):
    items, views = [], []
    for k in range(len(files)):
        p, pitch, w, h = ref.src(k)
        dst = ref.scratch(4 * w * h)
        items.append(capi.OrientItem(p, pitch, 0, 0, w, h, dst, 4 * h, 6))
        views.append((dst, 4 * h, 0, 0, h, w))
    tensors.orient_bgra(items)
    got, turns = tensors.decode_png_to_tensors(files, orientation=6, return_orientation=True)
    assert turns == [6] * len(files)
    same(ref, got, ref.to_tensors(views))
