"""GPU: progressive JPEG files to device pixels.  Every progressive file is held against its BASELINE TWIN through the existing calls
(the twin holds the same quantised coefficients, and the reconstruction behind the planes is shared), with either front end forced by
FFHIP_JPEG_PROGRESSIVE_GPU: k_jpeg_huff_prog, a lane per (picture, scan, restart interval), or the host threads."""
import ctypes as C

import numpy as np
import pytest

import exif_cases
import jpeg_progressive as P
import jpeg_writer
import progressive_cases as PC
from ffpic_amd import capi, ops

pytestmark = pytest.mark.gpu


@pytest.fixture
def front_end(monkeypatch):
    def set_(value):
        if value is None:
            monkeypatch.delenv("FFHIP_JPEG_PROGRESSIVE_GPU", raising=False)
        else:
            monkeypatch.setenv("FFHIP_JPEG_PROGRESSIVE_GPU", value)
        capi.reload_env()
    yield set_
    monkeypatch.undo()
    capi.reload_env()


@pytest.fixture(scope="module")
def pairs():
    """[(tag, progressive file, baseline twin)]: the PIL pairs and the writer files"""
    pytest.importorskip("PIL.Image")
    return PC.pil_pairs() + [(c["tag"], c["file"], c["twin"]) for c in PC.writer_cases()]


@pytest.fixture(scope="module")
def twin_pixels(pairs):
    """the twins' BGRA from the EXISTING mixed call, computed once"""
    return ops.jpeg_decode_files_mixed_device([t for _, _, t in pairs], n_threads=8)[1]


@pytest.mark.parametrize("gpu", ["1", "0"])
def test_one_mixed_call_gives_the_twins_pixels(pairs, twin_pixels, front_end, gpu):
    front_end(gpu)
    rng = np.random.default_rng(7)
    files = [(k, 1, p) for k, (_, p, _) in enumerate(pairs)] + [(k, 0, t) for k, (_, _, t) in enumerate(pairs)]
    order = rng.permutation(len(files))
    batch = [files[i] for i in order]
    geoms, images, _ = ops.jpeg_decode_files_mixed_device([f for _, _, f in batch], n_threads=8, progressive=True)
    last = ops.progressive_last()
    for (k, is_prog, _), img in zip(batch, images):
        assert np.array_equal(img, twin_pixels[k]), (pairs[k][0], "progressive" if is_prog else "baseline")
    assert last[0] == len(pairs) and last[4] == int(gpu)
    assert last[1] == sum(len(P.model_decode(p, k_max=-1)["scans"]) for _, p, _ in pairs) and last[2] == 0
    if gpu == "1":
        assert last[3] >= 4                                           # (the deepest script has four levels; classes launch theirs one after the other)


def _seventy():
    """70 small progressive files of one geometry, every one with tables of its own; some with restart markers"""
    rng = np.random.default_rng(70)
    files = []
    for i in range(70):
        coef = P.random_coef(rng, 24, 16, 2, 2, 3, density=0.1 + 0.005 * i)
        files.append(P.encode_progressive(24, 16, 2, 2, coef, PC.QUANT[:2], P.pil_script(3), restart=(0, 0, 2, 5)[i % 4]))
    return files


@pytest.fixture
def lanes_env(monkeypatch):
    def set_(value):
        if value is None:
            monkeypatch.delenv("FFHIP_JPEG_PROG_LANES", raising=False)
        else:
            monkeypatch.setenv("FFHIP_JPEG_PROG_LANES", str(value))
        capi.reload_env()
    yield set_
    monkeypatch.undo()
    capi.reload_env()


@pytest.mark.parametrize("lanes", [None, 2, 7, 64])
def test_device_planes_equal_host_planes(lanes, lanes_env):
    """ffhip_jpeg_progressive_batch_gpu against ffhip_jpeg_progressive_decode: 70 files of ten scans, every file with tables of its own, are
    some 900 work items in the first level (intervals count too).  Left to itself the launch gives every item a wave of its own while the
    device has waves to spare, so FFHIP_JPEG_PROG_LANES packs 2, 7 and 64 items into a wave: neighbours in a wave walk different scans with
    different tables and store to neighbouring coefficients of one block, workgroups and waves are crossed, and no level's item count is a
    multiple of 7 or 64 (asserted below from the files), so the last workgroup is partly empty.
    The public entry takes ONE geometry, so planes are compared for files of one size; pictures of mixed sizes in one class go through the
    per-picture geometries of the file call and are compared as pixels (test_mixed_sizes_of_one_class_on_the_device)."""
    files = _seventy()
    lanes_env(lanes)
    items = {}
    for f in files:
        for level, sc in zip((1, 1, 1, 1, 1, 2, 2, 2, 2, 3), P.model_decode(f, k_max=-1)["scans"]):
            units = len(P.scan_units(24, 16, 2, 2, sc["comps"]))
            restart = int.from_bytes(f[f.find(b"\xff\xdd") + 4:f.find(b"\xff\xdd") + 6], "big") if b"\xff\xdd" in f else 0
            items[level] = items.get(level, 0) + (-(-units // restart) if restart else 1)
    assert all(n % 7 and n % 64 and n > 64 for n in items.values()), items
    for k_max in (63, 0):
        g, cy, cu, cv, q = ops.jpeg_progressive_batch_gpu(files, k_max=k_max, n_threads=4)
        last = ops.progressive_last()
        assert last[0] == 70 and last[4] == 1 and last[1] + last[2] == 700 and last[3] == (3 if k_max else 2)
        assert last[2] == (0 if k_max else 560)
        yb, cb = g.y_blocks * 64, g.c_blocks * 64
        for i, f in enumerate(files):
            _, hy, hu, hv, hq = ops.jpeg_progressive_decode(f, k_max)
            assert np.array_equal(cy[i * yb:(i + 1) * yb], hy), (k_max, i)
            assert np.array_equal(cu[i * cb:(i + 1) * cb], hu) and np.array_equal(cv[i * cb:(i + 1) * cb], hv), (k_max, i)
            assert np.array_equal(q[i], hq), (k_max, i)


def test_mixed_sizes_of_one_class_on_the_device(front_end):
    """70 4:2:0 files of different sizes in one class: the device front end with per-picture geometries against the host threads"""
    rng = np.random.default_rng(71)
    files = []
    for i in range(70):
        w, h = 8 + 3 * (i % 11), 8 + 5 * (i % 7)
        coef = P.random_coef(rng, w, h, 2, 2, 3, density=0.15)
        files.append(P.encode_progressive(w, h, 2, 2, coef, PC.QUANT[:2], P.pil_script(3), restart=(0, 3)[i % 2]))
    front_end("0")
    host = ops.jpeg_decode_files_mixed_device(files, n_threads=8, progressive=True)[1]
    assert ops.progressive_last()[4] == 0
    front_end("1")
    dev = ops.jpeg_decode_files_mixed_device(files, n_threads=8, progressive=True)[1]
    assert ops.progressive_last() [4] == 1 and ops.progressive_last()[3] == 3
    for i in range(70):
        assert np.array_equal(host[i], dev[i]), i


@pytest.mark.parametrize("gpu", ["1", "0"])
def test_bad_progressive_file_in_the_middle_fails_alone(pairs, twin_pixels, front_end, gpu):
    """a file cut in its third scan -- as it is (no EOI: the parse refuses it) and with an EOI behind the cut (the scan runs dry: the decoder's
    verdict, on the device the kernel's) -- gets a non-zero status; the files around it decode"""
    front_end(gpu)
    good = pairs[0][1]
    third = [i for i in range(len(good) - 1) if good[i] == 0xFF and good[i + 1] == 0xDA][2]
    cut = good[:third + 14]
    batch = [pairs[0][1], cut, pairs[1][1], cut + b"\xff\xd9", pairs[3][1], pairs[0][2]]
    geoms, images, _, status = ops.jpeg_decode_files_mixed_device(batch, n_threads=4, strict=False, progressive=True)
    assert [bool(s) for s in status] == [False, True, False, True, False, False]
    for img, k in ((images[0], 0), (images[2], 1), (images[4], 3), (images[5], 0)):
        assert np.array_equal(img, twin_pixels[k])
    assert images[1] is None and images[3] is None


def test_tensors_without_size(pairs, front_end):
    """decode_jpeg_to_tensors(progressive=True) without size=: the _ex entry with no resize, every tensor at its file's own size"""
    torch = pytest.importorskip("torch")
    from ffpic_amd import tensors
    tags = {tag: (p, t) for tag, p, t in pairs}
    picks = ["420_41x23", "grey_37x19", "444_33x17", "h4v1_40x8"]
    mixed = [tags[picks[0]][0], tags[picks[1]][0], tags[picks[2]][1], tags[picks[3]][0]]
    base = [tags[t][1] for t in picks]
    exp = tensors.decode_jpeg_to_tensors(base)
    exp2 = tensors.decode_jpeg_to_tensors(base, reduce=2)
    for gpu in ("1", "0"):
        front_end(gpu)
        got = tensors.decode_jpeg_to_tensors(mixed, progressive=True)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, exp)), gpu
        got2 = tensors.decode_jpeg_to_tensors(mixed, progressive=True, reduce=2)
        assert all(torch.equal(a, b) for a, b in zip(got2, exp2)), gpu


def test_tensors_with_reduce_orientation_and_resize(pairs, front_end):
    torch = pytest.importorskip("torch")
    from ffpic_amd import tensors
    tags = {tag: (p, t) for tag, p, t in pairs}
    picks = ["420_40x24", "444_33x17", "grey_37x19", "420_41x23", "h4v1_40x8", "420_40x24_dri2"]
    prog = [tags[t][0] for t in picks]
    twin = [tags[t][1] for t in picks]
    prog[1], twin[1] = exif_cases.tagged_jpeg(prog[1], 6), exif_cases.tagged_jpeg(twin[1], 6)
    prog[3], twin[3] = exif_cases.tagged_jpeg(prog[3], 3), exif_cases.tagged_jpeg(twin[3], 3)
    mixed = [prog[0], twin[1], prog[2], prog[3], twin[4], prog[5], prog[1], prog[4]]
    base = [twin[0], twin[1], twin[2], twin[3], twin[4], twin[5], twin[1], twin[4]]
    kw = dict(size=(32, 48), reduce="auto", apply_exif_orientation=True, stack=True)
    exp = tensors.decode_jpeg_to_tensors(base, **kw)
    for gpu in ("1", "0", None):
        front_end(gpu)
        got = tensors.decode_jpeg_to_tensors(mixed, progressive=True, **kw)
        assert torch.equal(got, exp), gpu
        assert ops.progressive_last()[0] == 6 and ops.progressive_last()[4] == (1 if gpu == "1" else 0)
    # reduce=8: nothing but the DC scans is decoded
    front_end("1")
    exp8 = tensors.decode_jpeg_to_tensors(base, reduce=8, size=(8, 8), stack=True)
    got8 = tensors.decode_jpeg_to_tensors(mixed, reduce=8, size=(8, 8), stack=True, progressive=True)
    assert torch.equal(got8, exp8)
    last = ops.progressive_last()
    scans = [P.model_decode(f, k_max=-1)["scans"] for f in (mixed[0], mixed[2], mixed[3], mixed[5], mixed[6], mixed[7])]
    assert last[2] == sum(1 for s in scans for x in s if x["ss"] > 0) and last[1] == sum(1 for s in scans for x in s if x["ss"] == 0)
    # the default refuses the progressive files as it always did
    with pytest.raises(capi.FfhipError):
        tensors.decode_jpeg_to_tensors(mixed, **kw)
    res, status = tensors.decode_jpeg_to_tensors(mixed, strict=False)
    assert [bool(s) for s in status] == [True, False, True, True, False, True, True, True]


def test_progressive_gpu_switch(pairs, twin_pixels, front_end):
    """FFHIP_JPEG_PROGRESSIVE_GPU: =1 the device front end, =0 and unset the host threads; the same pixels either way"""
    files = [pairs[0][1], pairs[4][1]]
    for value, taken in (("1", 1), ("0", 0), (None, 0)):
        front_end(value)
        images = ops.jpeg_decode_files_mixed_device(files, n_threads=2, progressive=True)[1]
        assert ops.progressive_last()[4] == taken, value
        assert np.array_equal(images[0], twin_pixels[0]) and np.array_equal(images[1], twin_pixels[4]), value
