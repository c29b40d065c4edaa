"""pixels='libwebp' on the device: the kernels' instances under the rule, the planes and the pixels of the file call, and the tensors of
decode_webp_to_tensors, against the witness (tests/vp8_spec.py, rules=SPEC) and against PIL's RGB as the npz fixtures and
webp_libwebp_real.json hold it.  Every input is at most 5 x 4 macroblocks but the one hashed 1080p file.  No tolerance anywhere."""
import hashlib

import numpy as np
import pytest

import vp8_spec as S
from ffpic_amd import capi, ops, tensors
from test_webp_front_capi import NAMES as FIXTURES, file_bytes
from webp_pixels_cases import NAMES, REAL, data_of, first_plane_difference, pil_rgb, real_bytes, witness

pytestmark = pytest.mark.gpu
SWITCHES = ("FFHIP_WEBP_GPU_ENTROPY", "FFHIP_WEBP_PACK", "FFHIP_WEBP_PART_MB")


@pytest.fixture(autouse=True)
def _device_and_switches():
    capi.require_device(0)
    yield
    for n in SWITCHES:
        capi.setenv(n, None)


def files_of(names):
    return [data_of(n) for n in names]


def assert_pils_pixels(names, images, status):
    assert not any(status), [(n, s) for n, s in zip(names, status) if s]            # no file refused
    for name, img in zip(names, images):
        want = pil_rgb(name)
        assert img.shape == want.shape[:2] + (4,), (name, img.shape)
        assert np.array_equal(img[:, :, 2::-1], want) and (img[:, :, 3] == 255).all(), (name, np.argwhere((img[:, :, 2::-1] != want).any(axis=2))[:4])


@pytest.mark.parametrize("pack", [1, 5])
def test_kernels_a_and_b_under_the_rule_against_the_witness(pack):
    """one call for all files; pack = 5: five frames to a wave, divergent"""
    capi.setenv("FFHIP_WEBP_PACK", pack)
    dev, status = ops.webp_parse_device(files_of(NAMES), pixels="libwebp")
    assert not any(status)
    for name, p in zip(NAMES, dev):
        w = witness(name)
        assert np.array_equal(p["modes"], w["modes"]), name
        assert np.array_equal(p["levels"], w["levels"]), name
        assert np.array_equal(p["mbinfo"][:, :25], w["counts"]) and np.array_equal(p["mbinfo"][:, 26], w["modes"][:, 18]), name
        assert np.array_equal(p["resmap"], np.arange(len(w["modes"]))), name
        assert np.array_equal(p["quant"][:, :6], w["quant"]) and np.array_equal(p["filters"], w["filters"]) and p["filter_type"] == w["filter_type"], name
        host = ops.webp_parse(data_of(name), pixels="libwebp")
        assert all(np.array_equal(p[k], host[k]) for k in ("modes", "levels", "mbinfo", "resmap")), name


def test_planes_of_the_file_call_against_the_witness():
    infos, images, dout, status, planes = ops.webp_decode_files_device(files_of(NAMES), strict=False, pixels="libwebp", planes=True)
    assert not any(status)
    for name, pl in zip(NAMES, planes):
        w = witness(name)
        diff = first_plane_difference(pl, (w["y"], w["u"], w["v"]))
        assert diff is None, f"{name} (filter type {w['filter_type']}): {diff}"
    assert_pils_pixels(NAMES, images, status)


@pytest.mark.parametrize("entropy", [0, 1])
def test_pixels_of_the_file_call_against_pil(entropy):
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
    infos, images, dout, status = ops.webp_decode_files_device(files_of(NAMES), strict=False, pixels="libwebp")
    assert ops.webp_last_parts() == ((1, 0) if entropy else (0, 1))
    assert_pils_pixels(NAMES, images, status)
    for name, info in zip(NAMES, infos):
        w = witness(name)
        assert (info.width, info.height, info.mbcols, info.mbrows) == (w["width"], w["height"], w["mbcols"], w["mbrows"]), name


def test_a_permuted_mixed_call_and_several_parts():
    order = list(np.random.default_rng(9).permutation(len(NAMES)))
    names = [NAMES[i] for i in order]
    infos, images, dout, status = ops.webp_decode_files_device(files_of(names), strict=False, pixels="libwebp")
    assert_pils_pixels(names, images, status)
    for entropy in (0, 1):
        capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
        capi.setenv("FFHIP_WEBP_PART_MB", 40)
        infos, images, dout, status = ops.webp_decode_files_device(files_of(names), strict=False, pixels="libwebp")
        assert sum(ops.webp_last_parts()) > 4
        assert_pils_pixels(names, images, status)


def test_more_than_eight_frames_per_compute_unit():
    """every workgroup's share holds several frames: each copy equals its original.  One direct call (probing and slicing two thousand files
    through ops would be ten seconds of Python): zeroed pictures, so a copy's whole place -- what the call does not write included -- is compared"""
    import ctypes as C
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = (8 * cus) // len(NAMES) + 1
    n = reps * len(NAMES)
    assert n > 8 * cus
    grid = [ops.webp_probe(data_of(name), pixels="libwebp") for name in NAMES]
    size = [(64 * c * 16 * r + 15) & ~15 for _, _, c, r in grid]
    offs = np.concatenate([[0], np.cumsum(size * reps)])
    out = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    bufs, ptrs, lens = ops.file_args(files_of(NAMES) * reps)
    outs = (C.c_void_p * n)(*[out.data_ptr() + int(o) for o in offs[:-1]])
    pitch = (C.c_int64 * n)(*[64 * c for _, _, c, r in grid] * reps)
    status = (C.c_int * n)()
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", 1)
    rc = capi.lib().ffhip_webp_decode_files_device_ex(ptrs, lens, n, 8, outs, pitch, None, capi.FFHIP_WEBP_PIXELS_LIBWEBP, None, status, None)
    assert rc == 0 and not any(status)
    flat = out.cpu().numpy()
    for k, name in enumerate(NAMES):
        w, h, c, r = grid[k]
        first = flat[offs[k]:offs[k] + size[k]]
        assert np.array_equal(first[:64 * c * 16 * r].reshape(16 * r, 16 * c, 4)[:h, :w, 2::-1], pil_rgb(name)), name
        for rep in range(1, reps):
            at = offs[rep * len(NAMES) + k]
            assert np.array_equal(flat[at:at + size[k]], first), (name, rep)


@pytest.mark.parametrize("name", list(REAL))
def test_real_encoder_files_against_their_hashes(name):
    want = REAL[name]
    infos, images, dout = ops.webp_decode_files_device([real_bytes(name)], pixels="libwebp")
    rgb = np.ascontiguousarray(images[0][:, :, 2::-1])
    assert rgb.shape == (want["height"], want["width"], 3)
    if hashlib.sha256(rgb.tobytes()).hexdigest() == want["sha256"]:
        return
    bands = [hashlib.sha256(rgb[r:r + 16].tobytes()).hexdigest() for r in range(0, rgb.shape[0], 16)]
    bad = [k for k, (g, w) in enumerate(zip(bands, want["bands"])) if g != w]
    w = S.decode(real_bytes(name), S.SPEC)                   # only now: the witness says where
    at = np.argwhere((rgb != w["rgb"]).any(axis=2))
    pytest.fail(f"{name}: bands of 16 rows {bad[:8]} differ from PIL; first pixel that differs from the witness: {at[:1].tolist()}")


# ------------------------------------------------------------------------------------------------------------ tensors
TENSOR_NAMES = ["pil_noise_50x37_q30_m4", "pil_smooth_72x56_q60_m4", "wm_size_17x31", "wm_size_79x63", "wr_simple", "pil_noise_64x48_q60_m6"]


def uploaded_bgra(name):
    """PIL's RGB as a dense BGRA picture on the device (a torch tensor keeps it), alpha 255"""
    import torch
    rgb = pil_rgb(name)
    bgra = np.concatenate([rgb[:, :, ::-1], np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return torch.from_numpy(np.ascontiguousarray(bgra)).cuda()


def by_hand(names, roi=None, size=None, orientation=1):
    """the unchanged stages on uploaded pictures: rectangle, resize (in stored axes), orientation, tensor: list of [3][H][W] uint8"""
    import torch
    fmt = tensors.tensor_format()
    outs, keep = [], []
    for name in names:
        src = uploaded_bgra(name)
        h, w = src.shape[:2]
        ptr, pitch = src.data_ptr(), 4 * w
        x0, y0, rw, rh = (0, 0, w, h)
        if roi:                                                   # roi is in upright axes
            x0, y0, rw, rh = ops.orient_rect(w, h, orientation, roi) if orientation != 1 else roi
        swap = orientation >= 5
        if size:
            oh, ow = size
            sw, sh = (oh, ow) if swap else (ow, oh)               # the resize works in stored axes
            small = torch.empty((sh, sw, 4), dtype=torch.uint8, device="cuda")
            tensors.resize_bgra([capi.ResizeItem(ptr, pitch, x0, y0, rw, rh, small.data_ptr(), 4 * sw, sw, sh)])
            keep.append(small)
            ptr, pitch, x0, y0, rw, rh = small.data_ptr(), 4 * sw, 0, 0, sw, sh
        if orientation != 1:
            uw, uh = (rh, rw) if swap else (rw, rh)
            up = torch.empty((uh, uw, 4), dtype=torch.uint8, device="cuda")
            tensors.orient_bgra([capi.OrientItem(ptr, pitch, x0, y0, rw, rh, up.data_ptr(), 4 * uw, orientation)])
            keep.append(up)
            ptr, pitch, x0, y0, rw, rh = up.data_ptr(), 4 * uw, 0, 0, uw, uh
        t = torch.empty((3, rh, rw), dtype=torch.uint8, device="cuda")
        tensors.bgra_to_tensors([capi.TensorItem(ptr, pitch, x0, y0, rw, rh, t.data_ptr(), t.stride(1), t.stride(0))], fmt)
        keep.append(src)
        outs.append(t)
    torch.cuda.synchronize()
    return outs


def test_tensors_plain():
    import torch
    got = tensors.decode_webp_to_tensors(files_of(TENSOR_NAMES), pixels="libwebp")
    for name, g, w in zip(TENSOR_NAMES, got, by_hand(TENSOR_NAMES)):
        assert tuple(g.shape) == (3,) + pil_rgb(name).shape[:2] and torch.equal(g, w), name
        assert np.array_equal(g.cpu().numpy().transpose(1, 2, 0), pil_rgb(name)), name


def test_tensors_with_roi_and_size():
    import torch
    roi, size = (3, 2, 13, 11), (24, 20)
    got = tensors.decode_webp_to_tensors(files_of(TENSOR_NAMES), roi=roi, size=size, pixels="libwebp")
    for name, g, w in zip(TENSOR_NAMES, got, by_hand(TENSOR_NAMES, roi=roi, size=size)):
        assert tuple(g.shape) == (3, 24, 20) and torch.equal(g, w), name


def test_tensors_turned_and_stacked_over_files_of_different_sizes():
    import torch
    size = (40, 28)
    got, turned = tensors.decode_webp_to_tensors(files_of(TENSOR_NAMES), orientation=6, size=size, stack=True, return_orientation=True, pixels="libwebp")
    assert turned == [6] * len(TENSOR_NAMES) and tuple(got.shape) == (len(TENSOR_NAMES), 3, 40, 28)
    assert len({pil_rgb(n).shape for n in TENSOR_NAMES}) > 3
    for k, (name, w) in enumerate(zip(TENSOR_NAMES, by_hand(TENSOR_NAMES, size=size, orientation=6))):
        assert torch.equal(got[k], w), name


# ------------------------------------------------------------------------------------------------------------ the default rule keeps its bytes
def test_the_reference_rule_gives_the_bytes_of_the_existing_calls():
    import ctypes as C
    import torch
    files = [file_bytes(n) for n in FIXTURES]
    old = tensors.decode_webp_to_tensors(files, strict=False)
    new = tensors.decode_webp_to_tensors(files, strict=False, pixels="reference")
    assert old[1] == new[1]
    for a, b in zip(old[0], new[0]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    infos, images, dout, status = ops.webp_decode_files_device(files, strict=False)
    infos2, images2, dout2, status2 = ops.webp_decode_files_device(files, strict=False, pixels="reference")
    assert status == status2 and all((a is None) == (b is None) and (a is None or np.array_equal(a, b)) for a, b in zip(images, images2))
    # ffhip_webp_decode_files_device_ex with flags == 0, called directly
    L = capi.lib()
    good = [(f, img) for f, img, s in zip(files, images, status) if not s]
    n = len(good)
    bufs, ptrs, lens = ops.file_args([f for f, _ in good])
    grids = [ops.webp_probe(f) for f, _ in good]
    pics = [torch.zeros((16 * r, 64 * c), dtype=torch.uint8, device="cuda") for _, _, c, r in grids]
    outs = (C.c_void_p * n)(*[p.data_ptr() for p in pics])
    pitches = (C.c_int64 * n)(*[64 * c for _, _, c, r in grids])
    st = (C.c_int * n)()
    assert L.ffhip_webp_decode_files_device_ex(ptrs, lens, n, 4, outs, pitches, None, 0, None, st, None) == 0 and not any(st)
    for (f, img), pic, (w, h, c, r) in zip(good, pics, grids):
        assert np.array_equal(pic.cpu().numpy().reshape(16 * r, 16 * c, 4)[:img.shape[0], :img.shape[1]], img)
