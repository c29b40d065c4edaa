"""GPU: the alpha plane of lossy WebP files into byte 3 of their device pixels (FFHIP_WEBP_ALPHA).  Every case of webp_alpha_cases.py in one
ffhip_webp_decode_files_device_ex call: alpha against the answer key, the colour bytes against the UNFLAGGED pixels='libwebp' call on the
same files, the debug counts; the golden's files against their stored pixels; the same call in several parts; damaged files among good
ones; a lone file over three unfilter levels; the bytes beside the pictures; a batch without any alpha file.  Byte for byte, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import webp_alpha_cases as K
from ffpic_amd import capi, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_webp_alpha as golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    capi.require_device(0)
    return [c.data for c in K.cases()]


@pytest.fixture(scope="module")
def unflagged(files):
    """the parent's code path on the same files, once: the colour every flagged call must keep"""
    _, images, _ = ops.webp_decode_files_device(files, pixels="libwebp")
    assert all((im[..., 3] == 255).all() for im in images)
    return images


def check_all(images, unflagged):
    for c, got, plain in zip(K.cases(), images, unflagged):
        assert got is not None and got.shape == plain.shape, c.name
        assert np.array_equal(got[..., :3], plain[..., :3]), c.name
        want = c.plane if c.plane is not None else np.full(plain.shape[:2], 255, np.uint8)
        assert np.array_equal(got[..., 3], want), (c.name, np.argwhere(got[..., 3] != want)[:4].tolist())


def expected_counts(cs, parts=1):
    with_plane = [c for c in cs if c.plane is not None]
    return (len(with_plane), sum(c.compression == 1 for c in with_plane), max([K.levels_of(c) for c in with_plane] + [0]), parts)


def test_all_cases_in_one_call(files, unflagged):
    infos, images, _ = ops.webp_decode_files_device(files, pixels="libwebp", alpha=True)
    check_all(images, unflagged)
    assert ops.webp_alpha_last() == expected_counts(K.cases())
    for c, info in zip(K.cases(), infos):
        if c.plane is not None:
            assert (info.width, info.height) == c.plane.shape[::-1], c.name


def test_the_goldens_files_give_the_goldens_pixels():
    capi.require_device(0)
    stored = golden.load()
    _, images, _ = ops.webp_decode_files_device([d for _, d, _ in stored], pixels="libwebp", alpha=True)
    for (name, _, pixels), got in zip(stored, images):
        assert np.array_equal(got, pixels), name


def test_several_parts_give_the_same_pictures(files, unflagged, monkeypatch):
    monkeypatch.setenv("FFHIP_WEBP_ALPHA_PART_BYTES", "20000")       # the largest files are parts of their own
    capi.reload_env()
    _, images, _ = ops.webp_decode_files_device(files, n_threads=3, pixels="libwebp", alpha=True)
    last = ops.webp_alpha_last()
    assert last[3] >= 8 and last[:2] == expected_counts(K.cases())[:2]
    check_all(images, unflagged)


def test_damaged_files_are_their_files_alone(files, unflagged):
    bad = {d.name: d.data for d in K.damaged_cases()}
    batch = list(files[:6])
    batch.insert(1, bad["raw-short"])
    batch.insert(3, bad["lossless-over-subscribed"])
    batch.append(bad["lossless-truncated"])
    batch.append(bad["reserved-bit-6"])
    at = (1, 3, 8, 9)
    _, images, _, status = ops.webp_decode_files_device(batch, strict=False, pixels="libwebp", alpha=True)
    assert [k for k, s in enumerate(status) if s] == list(at) and all(status[k] == capi.FFHIP_EINVAL for k in at)
    assert all(images[k] is None for k in at)
    good = [im for k, im in enumerate(images) if k not in at]
    for c, got, plain in zip(K.cases()[:6], good, unflagged[:6]):
        assert np.array_equal(got[..., :3], plain[..., :3]) and np.array_equal(got[..., 3], c.plane), c.name
    assert ops.webp_alpha_last()[:2] == (6, 3)                        # the planes delivered
    with pytest.raises(capi.FfhipError):
        ops.webp_decode_files_device(batch, pixels="libwebp", alpha=True)
    _, plain_images, _, plain_status = ops.webp_decode_files_device(batch, strict=False, pixels="libwebp")
    assert not any(plain_status)                                      # without the flag these files decode, opaque


def test_a_lone_gradient_file_over_its_levels():
    capi.require_device(0)
    c = {c.name: c for c in K.cases()}["h130-w5-raw-f3"]
    _, images, _ = ops.webp_decode_files_device([c.data], pixels="libwebp", alpha=True)
    assert np.array_equal(images[0][..., 3], c.plane)
    assert ops.webp_alpha_last() == (1, 0, 3, 1)


def test_bytes_beside_the_pictures_keep_a_sentinel(files, unflagged):
    """every picture in a frame of its own: 16 bytes wider than its pitch asks and two rows higher, filled with a sentinel; the call
    writes width x height pixels and nothing beside them"""
    cs = K.cases()
    grids = [ops.webp_probe(f, "libwebp") for f in files]
    pitches = [64 * c + 16 for _, _, c, _ in grids]
    offs, total = [], 0
    for (w, h, c, r), p in zip(grids, pitches):
        offs.append(total + p)                                        # a row of sentinel above
        total += p * (16 * r + 2)
    dev = ops.DeviceBuffer(host=np.full(total, 0xA5, np.uint8))
    n = len(cs)
    bufs, ptrs, lens = ops.file_args(files)
    outs = (C.c_void_p * n)(*[dev.ptr + o for o in offs])
    status = (C.c_int * n)()
    rc = capi.lib().ffhip_webp_decode_files_device_ex(ptrs, lens, n, 4, outs, (C.c_int64 * n)(*pitches), None,
                                                      capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA, None, status, None)
    assert rc == 0 and not any(status)
    flat = dev.to_host((total,), np.uint8)
    for c, (w, h, mc, mr), p, o, plain in zip(cs, grids, pitches, offs, unflagged):
        frame = flat[o - p:o + p * (16 * mr + 1)].reshape(16 * mr + 2, p)
        got = frame[1:h + 1, :4 * w].reshape(h, w, 4)
        want = c.plane if c.plane is not None else np.full((h, w), 255, np.uint8)
        assert np.array_equal(got[..., :3], plain[..., :3]) and np.array_equal(got[..., 3], want), c.name
        assert (frame[0] == 0xA5).all() and (frame[h + 1:] == 0xA5).all() and (frame[1:h + 1, 4 * w:] == 0xA5).all(), c.name


def test_a_batch_without_alpha_equals_the_unflagged_call(files, unflagged):
    ks = [k for k, c in enumerate(K.cases()) if c.plane is None]
    assert len(ks) >= 5
    _, images, _ = ops.webp_decode_files_device([files[k] for k in ks], pixels="libwebp", alpha=True)
    for k, got in zip(ks, images):
        assert np.array_equal(got, unflagged[k]), K.cases()[k].name
    assert ops.webp_alpha_last() == (0, 0, 0, 0)
