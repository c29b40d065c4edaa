"""GPU: the JPEG encoder on the device against the witness (tests/jpeg_encode_spec.py, held to PIL byte for byte by
test_jpeg_encode_spec.py; no PIL here): ffhip_jpeg_fdct_items coefficient for coefficient through every source form, ffhip_jpeg_huff_encode_items
and ffhip_jpeg_encode_items file for file -- mixed batches in ONE call and one call per item --, the cap, the scratch, and tensors.encode_jpeg
through the library's own decoder."""
import numpy as np
import pytest

import jpeg_encode_spec as spec
import scratch_fill as SF
import stream_order as SO
from ffpic_amd import capi, ops, tensors
from jpeg_encode_cases import CASES, LARGE, SMALL

pytestmark = pytest.mark.gpu
FILL = 0xA5
NOSPACE, RANGE = capi.FFHIP_EJPEG_NOSPACE, capi.FFHIP_EJPEG_RANGE


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


def plane_sizes(case):
    """int16 elements of the case's three coefficient planes"""
    return [0 if c is None else c.size for c in case.key[0]]


FORMS = ["HWC", "CHW", "BGR", "BGRA"]


def source_of(case, form, arena):
    """the case's pixels in one of the source forms -> a function of the arena's base that gives its capi.JpegSource"""
    px, W, H = case.pixels, case.width, case.height
    if px.ndim == 2:                                                    # grey: rows with a padded pitch in every form but the first
        pitch = W if form == "HWC" else W + 5
        host = np.full((H, pitch), 0x5A, np.uint8)
        host[:, :W] = px
        off = arena.add(host.nbytes, host)
        return lambda base: capi.jpeg_source(base + off, W, H, pitch, 1, (0,), 1)
    if form == "HWC":
        off = arena.add(px.nbytes, px)
        return lambda base: capi.jpeg_source(base + off, W, H, 3 * W, 3, (0, 1, 2), 3)
    if form == "CHW":
        host = np.ascontiguousarray(px.transpose(2, 0, 1))
        off = arena.add(host.nbytes, host)
        return lambda base: capi.jpeg_source(base + off, W, H, W, 1, (0, W * H, 2 * W * H), 3)
    if form == "BGR":
        host = np.ascontiguousarray(px[..., ::-1])
        off = arena.add(host.nbytes, host)
        return lambda base: capi.jpeg_source(base + off, W, H, 3 * W, 3, (2, 1, 0), 3)
    pitch = 4 * W + 16                                                  # BGRA with a padded pitch; alpha and padding are never the picture's
    host = np.full((H, pitch), 0x5A, np.uint8)
    host[:, :4 * W].reshape(H, W, 4)[..., :3] = px[..., ::-1]
    off = arena.add(host.nbytes, host)
    return lambda base: capi.jpeg_source(base + off, W, H, pitch, 4, channels=4)


def coef_places(cases, arena, upload=False):
    places = []
    for c in cases:
        places.append([None if n == 0 else arena.add(2 * n, c.key[0][k] if upload else None) for k, n in enumerate(plane_sizes(c))])
    return places


def check_planes(cases, places, flat):
    for c, offs in zip(cases, places):
        for k, off in enumerate(offs):
            if off is None:
                continue
            want = c.key[0][k]
            got = flat[off:off + 2 * want.size].view(np.int16)
            assert np.array_equal(got, want), (c.id, k, np.flatnonzero(got != want)[:8].tolist())
            assert (flat[off + 2 * want.size:off + 2 * want.size + 256] == FILL).all() and (flat[off - 256:off] == FILL).all(), ("bytes beside a plane", c.id, k)


# ---------------------------------------------------------------------------------------------------- pixels to coefficients
@pytest.mark.parametrize("form", FORMS)
def test_fdct_items_equal_the_witness(form):
    """every case in ONE call, through one source form: the witness's coefficients, dummy blocks included, and nothing beside the planes"""
    capi.require_device()
    cases = [c for c in CASES if not (form == "BGRA" and c.layout == "grey")]
    arena = Arena()
    sources = [source_of(c, form, arena) for c in cases]
    places = coef_places(cases, arena)
    base = arena.upload()
    items = []
    for c, src, offs in zip(cases, sources, places):
        it = capi.JpegFdctItem()
        it.src, it.layout, it.quality = src(base), spec.LAYOUT_ID[c.layout], c.quality
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [None if o is None else base + o for o in offs]
        items.append(it)
    ops.jpeg_fdct_items(items)
    capi.sync()
    check_planes(cases, places, arena.read())


def test_fdct_items_is_stream_ordered():
    """The scenario of tests/stream_order.py on the enqueue-only entry: the pictures arrive on the stalled stream behind the call's enqueue (the
    buffers hold other pictures then) and are overwritten behind it; the consumer's copy must hold the coefficients of the REAL pictures"""
    L = capi.require_device(0)
    stall = SO.Stall()
    stream = L.ffhip_stream_create()
    try:
        cases = [next(c for c in SMALL if c.id.startswith(f"40x24-{layout}-q75-r0")) for layout in ("4:2:0", "4:4:4", "grey")]
        pixels = [SO.Operand(c.pixels, 255 - c.pixels) for c in cases]
        offs, total = [], 0
        for c in cases:
            offs.append([])
            for n in plane_sizes(c):
                offs[-1].append(total if n else None)
                total += up(2 * n)
        out = SO.Output(total)
        items = []
        for c, px, o in zip(cases, pixels, offs):
            it = capi.JpegFdctItem()
            grey = c.layout == "grey"
            it.src = capi.jpeg_source(px.ptr, c.width, c.height, c.width * (1 if grey else 3), 1 if grey else 3, (0, 1, 2), 1 if grey else 3)
            it.layout, it.quality = spec.LAYOUT_ID[c.layout], c.quality
            it.d_coef_y, it.d_coef_u, it.d_coef_v = [None if x is None else out.ptr + x for x in o]
            items.append(it)
        arr = (capi.JpegFdctItem * len(items))(*items)

        def call(s):
            capi.check(L.ffhip_jpeg_fdct_items(arr, len(items), s), "ffhip_jpeg_fdct_items")
        rc = SO.run("jpeg_fdct_items", stall, stream, 128, call, pixels, [out])
        assert rc == 0, rc
        got = out.copied()
        for c, o in zip(cases, offs):
            for k, x in enumerate(o):
                if x is not None:
                    assert np.array_equal(got[x:x + 2 * c.key[0][k].size].view(np.int16), c.key[0][k]), (c.id, k)
    finally:
        L.ffhip_stream_destroy(stream)


# ---------------------------------------------------------------------------------------------------- coefficients to files
def huff_call(entries, caps=None, strict=True):
    """entries: (width, height, layout name, quality, restart, [coef y, u, v]) -> ([bytes written into each output's cap], lens, status);
    every output in a frame of 0xA5 that must be intact"""
    arena = Arena()
    places, outs = [], []
    for k, (w, h, layout, q, r, coef) in enumerate(entries):
        places.append([None if c is None else arena.add(c.nbytes, c) for c in coef])
        cap = ops.jpeg_encode_bound(w, h, layout, r) if caps is None or caps[k] is None else caps[k]
        outs.append((arena.add(cap), cap))
    base = arena.upload()
    items = []
    for (w, h, layout, q, r, coef), offs, (out, cap) in zip(entries, places, outs):
        it = capi.JpegHuffItem()
        it.width, it.height, it.layout, it.quality, it.restart = w, h, spec.LAYOUT_ID[layout], q, r
        it.d_coef_y, it.d_coef_u, it.d_coef_v = [None if o is None else base + o for o in offs]
        it.d_out, it.cap = base + out, cap
        items.append(it)
    lens, status = ops.jpeg_huff_encode_items(items, strict=strict)
    return framed(arena.read(), outs, lens), lens, status


def framed(flat, outs, lens):
    files = []
    for k, ((out, cap), n) in enumerate(zip(outs, lens)):
        used = min(n, cap)
        assert (flat[out + used:up(out + cap) + 256] == FILL).all() and (flat[out - 256:out] == FILL).all(), ("bytes beside a file", k)
        files.append(flat[out:out + used].tobytes())
    return files


def test_huff_encode_items_equal_the_writer_on_the_cases():
    """the cases' coefficient planes, all in ONE call: tests/jpeg_writer.encode's files (with the JFIF segment)"""
    capi.require_device()
    files, lens, status = huff_call([(c.width, c.height, c.layout, c.quality, c.restart, c.key[0]) for c in CASES])
    assert status == [0] * len(CASES)
    for c, f in zip(CASES, files):
        assert f == c.key[2], (c.id, len(f), len(c.key[2]))


def hand_made():
    """planes no picture gives: runs of 16, 32 and 48 zeros, a non-zero 63rd coefficient, DC differences of +-2047, magnitudes that are all
    ones (2^t - 1: the scan is dense in FF) -> entries of huff_call"""
    from jpeg_entropy import ZZ
    rng = np.random.default_rng(5)
    entries = []
    for layout, (w, h) in (("4:2:0", (40, 24)), ("4:4:4", (17, 13)), ("4:2:2", (33, 9)), ("grey", (9, 33))):
        hh, vv, ncomp = spec.LAYOUTS[layout]
        mcus = -(-w // (8 * hh)) * -(-h // (8 * vv))
        coef = []
        for comp in range(ncomp):
            n = mcus * (hh * vv if comp == 0 else 1)
            blocks = np.zeros((n, 64), np.int16)
            for b in range(n):
                zz = np.zeros(64, np.int64)
                kind = b % 6
                if kind == 0:                                   # runs of exactly 16, 32 and 48 zeros, and the 63rd coefficient
                    for pos in (1, 18, 51, 63):
                        zz[pos] = rng.choice([-1, 1]) * (2 ** int(rng.integers(1, 11)) - 1)
                elif kind == 1:                                 # every coefficient all ones: FF after FF
                    zz[1:] = 2 ** rng.integers(1, 11, 63) - 1
                elif kind == 2:                                 # 48 zeros, then the last coefficient
                    zz[14], zz[63] = 1023, -1023
                elif kind == 3:                                 # an empty block: EOB alone
                    pass
                elif kind == 4:
                    zz[1:] = rng.integers(-1023, 1024, 63)
                else:
                    zz[17], zz[50] = -1, 1                      # ZRL, then run 0: the 17th; two ZRL behind it
                blocks[b][ZZ] = zz
                blocks[b][0] = (1023, -1024, 1023, 0, -1, 1023)[b % 6]          # differences of +-2047 among them
            coef.append(np.ascontiguousarray(blocks.reshape(-1)))
        coef += [None] * (3 - ncomp)
        for restart in (0, 2):
            entries.append((w, h, layout, 90, restart, coef))
    return entries


def test_huff_encode_items_equal_the_writer_on_hand_made_planes():
    capi.require_device()
    entries = hand_made()
    files, lens, status = huff_call(entries)
    assert status == [0] * len(entries)
    dense, diffs, zrl = 0, [], 0
    for (w, h, layout, q, r, coef), f in zip(entries, files):
        stats = {}
        hh, vv, _ = spec.LAYOUTS[layout]
        import jpeg_writer
        want = spec.with_jfif(jpeg_writer.encode(w, h, hh, vv, coef, spec.tables(q), (0, 1, 1), r, stats=stats))
        assert f == want, (layout, r, len(f), len(want))
        diffs += list(stats["dc_diffs"])
        zrl = max(zrl, stats["zrl_in_a_row"])
        dense += want.count(b"\xff\x00")
    assert (min(diffs), max(diffs), zrl) == (-2047, 2047, 3) and dense > 500          # what the planes were made for


def test_a_coefficient_without_a_code_is_its_items_verdict():
    """an AC magnitude of 1024, a DC difference of 2048 and one of -2048: FFHIP_EJPEG_RANGE for those items, their neighbours' files whole"""
    capi.require_device()
    good = hand_made()[0]

    def spoiled(index, value, second=None):
        coef = [None if c is None else c.copy() for c in good[5]]
        coef[0][index] = value
        if second is not None:
            coef[0][second[0]] = second[1]
        return good[:5] + (coef,)
    entries = [good, spoiled(64 * 3 + 9, 1024), good, spoiled(64 * 3, 1024, (64 * 4, -1024)), spoiled(64 * 3, -1024, (64 * 4, 1024)), spoiled(64 * 2 + 63, -1024), good]
    files, lens, status = huff_call(entries, strict=False)
    assert status == [0, RANGE, 0, RANGE, RANGE, RANGE, 0]
    assert files[0] == files[2] == files[6] and len(files[0]) == lens[0]
    with pytest.raises(capi.FfhipError):
        huff_call(entries[:2])


# ---------------------------------------------------------------------------------------------------- the file call
def encode_call(cases, form="HWC", caps=None, strict=True, stream=None, one_by_one=False):
    arena = Arena()
    sources = [source_of(c, form, arena) for c in cases]
    outs = []
    for k, c in enumerate(cases):
        cap = ops.jpeg_encode_bound(c.width, c.height, c.layout, c.restart) if caps is None or caps[k] is None else caps[k]
        outs.append((arena.add(cap), cap))
    base = arena.upload()
    items = []
    for c, src, (out, cap) in zip(cases, sources, outs):
        it = capi.JpegEncodeItem()
        it.src, it.layout, it.quality, it.restart, it.d_out, it.cap = src(base), spec.LAYOUT_ID[c.layout], c.quality, c.restart, base + out, cap
        items.append(it)
    if one_by_one:
        lens, status = [], []
        for it in items:
            n, s = ops.jpeg_encode_items([it], stream, strict=strict)
            lens += n
            status += s
    else:
        lens, status = ops.jpeg_encode_items(items, stream, strict=strict)
    return framed(arena.read(), outs, lens), lens, status


def test_encode_items_all_cases_in_one_call():
    """every layout, size, quality, restart interval and content in ONE call: the witness's files, byte for byte"""
    capi.require_device()
    files, lens, status = encode_call(CASES)
    assert status == [0] * len(CASES)
    for c, f, n in zip(CASES, files, lens):
        assert n == len(c.key[2]) and f == c.key[2], (c.id, n, len(c.key[2]))


def test_encode_items_one_call_per_item_and_from_bgra():
    capi.require_device()
    files, _, status = encode_call(CASES, one_by_one=True)
    assert status == [0] * len(CASES) and files == [c.key[2] for c in CASES]
    colour = [c for c in CASES if c.layout != "grey"]
    files, _, status = encode_call(colour, form="BGRA")
    assert status == [0] * len(colour) and files == [c.key[2] for c in colour]


def test_a_cap_one_byte_short():
    """FFHIP_EJPEG_NOSPACE, the length the file needs, the 0xA5 behind cap intact (framed), the bytes below cap the file's, the neighbours whole"""
    capi.require_device()
    cases = SMALL[3:40:4]
    caps = [len(c.key[2]) - 1 if k % 3 == 1 else (len(c.key[2]) if k % 3 == 2 else None) for k, c in enumerate(cases)]
    files, lens, status = encode_call(cases, caps=caps, strict=False)
    assert status == [NOSPACE if k % 3 == 1 else 0 for k in range(len(cases))]
    for k, (c, f, n) in enumerate(zip(cases, files, lens)):
        assert n == len(c.key[2]), c.id
        assert f == (c.key[2][:-1] if k % 3 == 1 else c.key[2]), c.id
    files, lens, status = encode_call(cases[:2], caps=[0, 7], strict=False)       # no room at all; not even the header
    assert status == [NOSPACE, NOSPACE] and lens == [len(c.key[2]) for c in cases[:2]] and files[1] == cases[1].key[2][:7]


def test_the_scratch_is_no_input():
    """the protocol of tests/scratch_fill.py on a stream of its own: the library's scratch overwritten between calls, the files the same"""
    L = SF.lib()
    stream = L.ffhip_stream_create()
    try:
        def run(cases, form):
            def case():
                files, _, status = encode_call(cases, form=form, stream=stream)
                assert status == [0] * len(cases) and files == [c.key[2] for c in cases]
            return case
        small = SMALL[::9]
        SF.run_protocol("jpeg_encode", stream, [run(LARGE + SMALL[::3], "HWC")], [run(small, "CHW"), run(small[:3], "HWC")], kinds=("SCRATCH_JPEG_ENC",))
    finally:
        L.ffhip_stream_destroy(stream)


# ---------------------------------------------------------------------------------------------------- Python
def test_tensors_encode_jpeg_round_trips():
    """tensors.encode_jpeg on CHW, HWC and grey tensors of mixed sizes: the witness's files; and the library's own decode of them with
    pixels='libjpeg' is what the host function ffhip_jpeg_libjpeg_picture makes of the witness's coefficients (the function that
    test_jpeg_libjpeg.py holds to PIL on the CPU) and, where PIL is installed, what PIL decodes from the same bytes"""
    import torch
    capi.require_device()
    plain = [c for c in SMALL if c.quality == 75 and c.restart == 0]
    cases = sum(([c for c in plain if c.layout == layout][-2:] for layout in ("4:4:4", "4:2:2", "4:2:0", "grey")), [])
    dev = torch.device("cuda", torch.cuda.current_device())
    pictures = []
    for k, c in enumerate(cases):
        t = torch.from_numpy(np.ascontiguousarray(c.pixels)).to(dev)
        pictures.append(t[None] if t.dim() == 2 else (t if k % 2 else t.permute(2, 0, 1).contiguous()))
    files = tensors.encode_jpeg(pictures, quality=75, subsampling=[c.layout if c.layout != "grey" else "4:2:0" for c in cases], to_host=True)
    assert files == [c.key[2] for c in cases]
    on_device = tensors.encode_jpeg(pictures[:3], quality=75, subsampling=[c.layout for c in cases[:3]])
    assert [bytes(f.cpu().numpy()) for f in on_device] == files[:3] and all(f.is_cuda and f.dtype == torch.uint8 and f.dim() == 1 for f in on_device)
    noisy = next(c for c in CASES if c.id == "100x75-4:4:4-q100-r0-noise")          # larger than half its pixels: the second call
    t = torch.from_numpy(noisy.pixels).to(dev)
    assert tensors.encode_jpeg(t, quality=100, subsampling="4:4:4", to_host=True) == noisy.key[2]
    decoded = tensors.decode_jpeg_to_tensors(files, layout="HWC", pixels="libjpeg")
    for c, d in zip(cases, decoded):
        h, v, ncomp = spec.LAYOUTS[c.layout]
        geom = capi.jpeg_geom(-(-c.width // (8 * h)), -(-c.height // (8 * v)), ncomp, h, v, (0, 1, 1) if ncomp == 3 else (0, 0, 0))
        want = ops.jpeg_libjpeg_picture(geom, c.width, c.height, *c.key[0], c.key[1])[..., 2::-1]
        assert np.array_equal(d.cpu().numpy(), want), c.id
    try:                                                                           # where PIL is installed: libjpeg's own decode of the same files
        from PIL import Image
    except ImportError:
        Image = None
    for c, f, d in zip(cases, files, decoded) if Image is not None else ():
        import io
        assert np.array_equal(d.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))), c.id
    with pytest.raises(ValueError):
        tensors.encode_jpeg([torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)])
    with pytest.raises(ValueError):
        tensors.encode_jpeg([torch.zeros((3, 8, 8), dtype=torch.float32, device=dev)])
