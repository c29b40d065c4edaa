"""GPU: no call's output depends on what the library's kept memory held before it.

The library keeps, per (device, stream) and scratch kind, a device buffer and a pinned one that only grow (with a quarter of headroom) --
each thread's two slots of the JPEG file pipeline are such buffers, under slot streams the thread keeps per device: a fill reaches every
kind kept under them, the front end's included -- and per thread the Huffman decoder's header records.  In the rest of the suite a call finds there
either a fresh allocation or its own case's bytes from last time.  Here ffhip_debug_scratch_fill sets every byte of all of it -- 0xFF,
0x5A, 0x00 in turn -- between the calls of every family of entry points, by the protocol of scratch_fill.run_protocol: the family's
larger case first, then its small cases after each fill, then the larger case after a last fill of 0xFF.  Every output is compared, byte
for byte and with the 0xA5 around it, with an answer key that is no run of the library: the case modules' expected(), the numpy rules
of test_resize_gpu.py, the oracle (oracle_lib.py), the goldens, the witnesses (png_spec, vp8_spec, webp_alpha_spec) and, for planes and
libjpeg's pixels, the host functions the CPU tests hold to those.  No tolerance anywhere.

The entries that take a stream run on ONE created stream of the module (its state starts from nothing); the file-to-tensor helpers of
test_resize_gpu.py, ffhip_jpeg_decode_files, ffhip_jpeg_recon_batch_host and the block operations are the NULL stream's.  The module ends
with the condition that every kind of enum FfhipScratchKind was reported by a fill that a checked run followed."""
import ctypes as C
import threading

import numpy as np
import pytest

import exif_cases as X
import jpeg_scaled_rule as R
import oracle_lib as O
import png_cases
import progressive_cases as PC
import scratch_fill as SF
import stream_order as SO
import test_stream_order_gpu as TSO
import vp8_spec
import vp8l_cases
import webp_alpha_cases as AK
import webp_alpha_spec
import webp_pixels_cases as WP
from ffpic_amd import capi, ops, synth
from test_jpeg_mixed_gpu import LAYOUTS, _writer_file
from test_resize_gpu import AA, BIL, F16, U8, check_files, inner_rois, make_format, per_file_sizes, resize_rule
from test_vp8_gpu import oracle_residual
from test_webp_files_gpu import late_bad
from test_webp_front_capi import FRONT, NAMES, file_bytes

pytestmark = pytest.mark.gpu
EINVAL = capi.FFHIP_EINVAL
SWITCHES = ("FFHIP_JPEG_GPU_ENTROPY", "FFHIP_JPEG_PROGRESSIVE_GPU", "FFHIP_VP8_FRAMES", "FFHIP_WEBP_GPU_ENTROPY", "FFHIP_PNG_PART_BYTES",
            "FFHIP_VP8L_PART_BYTES", "FFHIP_WEBP_ALPHA_PART_BYTES", "FFHIP_TENSOR_PART_BYTES")


@pytest.fixture(scope="module")
def stream():
    L = capi.require_device(0)
    s = L.ffhip_stream_create()
    assert s
    yield s
    L.ffhip_stream_destroy(s)


@pytest.fixture(autouse=True)
def _switches_back():
    capi.require_device(0)
    yield
    for name in SWITCHES:
        capi.setenv(name, None)


# ---------------------------------------------------------------------------------------------------- cases of test_stream_order_gpu.py
_EXPECT = {}


def plain(case, s, retry_ok=False, memo=True):
    """a Case of test_stream_order_gpu.py as a checked run without a stall: the real inputs into the operands, the call, the consumer's
    copies, the sync, the outputs against the oracle's.  A side-by-side VP8 call the sync had to repeat is handled as it is there.
    `s` may be a scratch_fill.StreamBox (tests/concurrency.py): the buffers are then refilled on that stream too, not on the NULL stream, and
    run.prime() computes the answer key ahead of the first run.  run() -> the status of its sync (0, or FFHIP_RETRIED with retry_ok)"""
    def expect(which):
        if not memo:
            return case.expect(which)
        if case.name not in _EXPECT:
            _EXPECT[case.name] = [np.array(SO.as_bytes(e)) for e in case.expect(which)]     # once per case, shared by every run of it
        return _EXPECT[case.name]

    checked = TSO.Case(case.name, case.call, case.operands, case.outputs, expect)

    def run(s=s):
        L = capi.lib()
        own = isinstance(s, SF.StreamBox)
        s = SF.h(s)
        for o in case.outputs:
            o.refill(s if own else None)
        for ptr, value, nbytes in case.memsets:
            capi.check(L.ffhip_memset(ptr, value, nbytes, s), "ffhip_memset")
        for op in case.operands:
            SO.copy(op.dev.ptr, op.true.ptr, op.nbytes, s)
        case.call(s)
        for o in case.outputs:
            SO.copy(o.copy.ptr, o.dev.ptr, o.nbytes, s)
        rc = capi.sync(s)
        assert rc == 0 or (retry_ok and rc == capi.FFHIP_RETRIED), (case.name, rc)
        if rc == capi.FFHIP_RETRIED:
            TSO.assert_outputs(checked, "true", read="written")
            for o in case.outputs:
                SO.copy(o.copy.ptr, o.dev.ptr, o.nbytes, s)
            assert capi.sync(s) == 0
        TSO.assert_outputs(checked, "true")
        return rc
    run.prime = lambda: expect("true")
    return run


# ---------------------------------------------------------------------------------------------------- the hook itself
def test_the_hook_fills_what_it_says(stream):
    """control: behind a fill the first 64 bytes of a kind's device scratch, read through the library's own accessor, hold the value; the
    counts say something was written, the kind is reported, and a second fill with another value shows again"""
    L = SF.lib()
    plain(TSO.resize_case(AA), stream)()
    kind = SF.enum_kinds()["SCRATCH_RESIZE_ITEMS"][0]
    for value in (0xFF, 0x5A, 0x00, 0xC3):
        dev, host, kinds = SF.fill(stream, value)
        assert dev > 0 and host > 0 and kind in kinds and kinds == sorted(set(kinds)), (dev, host, kinds)
        assert (SF.scratch_head(kind, stream) == value).all(), value
    few = (C.c_int * 1)(-7)
    nbytes = (C.c_uint64 * 2)()
    assert L.ffhip_debug_scratch_fill(stream, 1, nbytes, few, 1) == len(kinds) and few[0] == kinds[0]      # the count, whatever cap is
    assert L.ffhip_debug_scratch_fill(stream, 1, None, few, 1) == EINVAL
    plain(TSO.resize_case(AA), stream)()                                                                   # and the entry still works behind it


# ---------------------------------------------------------------------------------------------------- JPEG reconstruction
def test_jpeg_reconstruction_items_and_batch(stream):
    s = stream
    larger = [plain(TSO.jpeg_items_case("fill jpeg_recon_items larger", TSO.JPEG_SPECS), s),
              plain(TSO.jpeg_items_case("fill jpeg_recon_items_scaled d2 larger", TSO.JPEG_SPECS, 2), s),
              plain(TSO.jpeg_items_case("fill jpeg_recon_items_scaled d8 larger", TSO.JPEG_SPECS, 8), s),
              plain(TSO.jpeg_items_libjpeg_case("fill jpeg_recon_items_libjpeg larger", TSO.JPEG_SPECS), s, memo=False)]
    small = [plain(TSO.jpeg_items_case("fill jpeg_recon_items small", TSO.JPEG_SMALL, many=True), s),
             plain(TSO.jpeg_items_case("fill jpeg_recon_items_scaled d2 small", TSO.JPEG_SMALL, 2, many=True), s),
             plain(TSO.jpeg_items_case("fill jpeg_recon_items_scaled d8 small", TSO.JPEG_SMALL, 8, many=True), s),
             plain(TSO.jpeg_items_libjpeg_case("fill jpeg_recon_items_libjpeg small", TSO.JPEG_SMALL), s, memo=False),
             plain(TSO.jpeg_batch_case(2, 2, 5, 4), s), plain(TSO.jpeg_batch_case(3, 1, 3, 2), s)]
    SF.run_protocol("jpeg reconstruction", s, larger, small, ["SCRATCH_JPEG_ITEMS", "SCRATCH_JPEG_SCALED", "SCRATCH_JPEG_LIBJPEG"])


def test_jpeg_host_entry_and_block_operations(golden):
    """ffhip_jpeg_recon_batch_host (the NULL stream's SCRATCH_JPEG_HOST) against the oracle; the per-block operations against the goldens"""
    q = synth.quant_tables()

    def host_case(mc, mr, n, h=2, v=2):
        planes = synth.coef_batch(n, mc, mr, 3, h, v, first=3)
        want = O.oracle_jpeg_recon(O.make_geom(mc, mr, 3, h, v), *planes, q, n_images=n)

        def run():
            got = ops.jpeg_recon_batch_host(capi.jpeg_geom(mc, mr, 3, h, v), n, *planes, q)
            assert np.array_equal(np.asarray(got).reshape(want.shape), want)
        return run

    def blocks():
        g8, g4 = golden("jpeg_blocks.npz"), golden("vp8_blocks.npz")
        for i in (0, 7, 39, 257, 505):
            b = g8["coef"][i].copy()
            ops.idct_8x8(b)
            assert np.array_equal(b, g8["idct"][i]), i
        for i in (0, 5, 31, 256, 504):
            b = g4["coef"][i].copy()
            ops.idct_4x4(b)
            assert np.array_equal(b, g4["idct"][i]), i
    SF.run_protocol("jpeg host entry", None, [host_case(13, 7, 3)], [host_case(1, 1, 1), host_case(5, 4, 2), host_case(3, 2, 2, 1, 1), blocks],
                    ["SCRATCH_JPEG_HOST"])


# ---------------------------------------------------------------------------------------------------- JPEG files
JPEG_BATCH = [(67, 35, "420", 0), (16, 16, "444", 0), (200, 31, "422", 3), (33, 70, "440", 0), (301, 47, "420", 7), (5, 3, "444", 1)]   # test_resize_gpu.jpeg_batch


class JpegFile:
    """a file of jpeg_writer.py with the coefficients it was written from: the answer keys are the oracle's (full size), the numpy rule's
    (a denominator) and the host function's (libjpeg's pixels) pictures of THOSE"""

    def __init__(self, data, coef, w, h, layout, quant):
        self.data, self.w, self.h, self.quant = data, w, h, quant
        self.ncomp, self.hh, self.vv = LAYOUTS[layout]
        self.mc, self.mr = -(-w // (8 * self.hh)), -(-h // (8 * self.vv))
        self.planes = [np.ascontiguousarray(c.reshape(-1)) if c is not None else None for c in coef]
        self.cw, self.ch = 8 * self.hh * self.mc, 8 * self.vv * self.mr
        self._keys = {}

    def key(self, rule="full", denom=1):
        k = (rule, denom)
        if k not in self._keys:
            if rule == "libjpeg":
                self._keys[k] = ops.jpeg_libjpeg_picture(capi.jpeg_geom(self.mc, self.mr, self.ncomp, self.hh, self.vv), self.w, self.h, *self.planes, self.quant)
            elif denom > 1:
                self._keys[k] = R.picture(self.mc, self.mr, self.ncomp, self.hh, self.vv, *self.planes, self.quant, denom)
            else:
                self._keys[k] = O.oracle_jpeg_recon(O.make_geom(self.mc, self.mr, self.ncomp, self.hh, self.vv), *self.planes, self.quant)[0]
        return self._keys[k]

    def shown(self):
        return self.key()[:self.h, :self.w]


def written_file(rng, w, h, layout, restart=0):
    q = synth.quant_tables()
    data, coef = _writer_file(rng, w, h, layout, restart=restart, q=q)
    return JpegFile(data, coef, w, h, layout, q)


def jpeg_batch_files(seed=6):
    """the files of test_resize_gpu.jpeg_batch's list with the truncated one in the middle -> ([JpegFile, None at the bad place], files, bad)"""
    rng = np.random.default_rng(seed)
    known = [written_file(rng, *spec) for spec in JPEG_BATCH]
    bad = len(known) // 2
    cut = known[4].data[:len(known[4].data) * 2 // 3]
    known.insert(bad, None)
    files = [cut if k is None else k.data for k in known]
    return known, files, bad


@pytest.fixture(scope="module")
def jpeg_batch():
    return jpeg_batch_files()


def mixed_runner(known, files, s, rule="full", denoms=None, flags=0, bad_code=EINVAL, n_threads=4):
    """ffhip_jpeg_decode_files_mixed_device / _scaled / _ex over framed outputs.  A bad file's place is as large as the file it was cut from"""
    L = capi.lib()
    n = len(files)
    denoms = denoms or [1] * n
    probed = [ops.jpeg_probe_any(f)[0] for f in files]
    places = [(4 * (g.width // d), g.height // d) for g, d in zip(probed, denoms)]
    keys = [None if k is None else k.key(rule, d) for k, d in zip(known, denoms)]
    den = (C.c_int * n)(*denoms)
    geoms = (capi.JpegGeom * n)()

    def call(ptrs, lens, n_, outs, pitches, status):
        if flags:
            return L.ffhip_jpeg_decode_files_mixed_device_ex(ptrs, lens, n_, n_threads, outs, pitches, den if rule == "scaled" else None, flags, geoms, status, SF.h(s))
        if rule == "scaled":
            return L.ffhip_jpeg_decode_files_mixed_device_scaled(ptrs, lens, n_, n_threads, outs, pitches, den, geoms, status, SF.h(s))
        return L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n_, n_threads, outs, pitches, geoms, status, SF.h(s))

    def run():
        SF.files_call(call, files, places, keys, {i: bad_code for i, k in enumerate(known) if k is None})
        return capi.sync(SF.h(s))
    return run


def uniform_runner(known, s, host_out=False, chunk=0, n_threads=3, device=0):
    """ffhip_jpeg_decode_files_device (pictures of one geometry into one device allocation) / ffhip_jpeg_decode_files (into pageable host
    memory through the calling thread's slots): a guard behind every row and behind every picture.  device: the one the run binds its
    thread to first, and allocates on"""
    L = capi.lib()
    n = len(known)
    W, H = known[0].cw, known[0].ch
    pitch, stride = 4 * W + 16, (4 * W + 16) * H + 32
    want = np.full(n * stride + 64, SF.FILL, np.uint8)
    for i, k in enumerate(known):
        TSO.place(want, i * stride, (H, W, 4), pitch, k.key())
    files = [k.data for k in known]

    def run():
        capi.require_device(device)
        bufs, ptrs, lens = ops.file_args(files)
        status, geom = (C.c_int * n)(), capi.JpegGeom()
        got = np.full(want.size, SF.FILL, np.uint8)
        if host_out:
            rc = L.ffhip_jpeg_decode_files(ptrs, lens, n, n_threads, chunk, C.byref(geom), got.ctypes.data, pitch, stride, status)
        else:
            dev = L.ffhip_malloc(got.nbytes)                # (not ops.DeviceBuffer: that binds device 0)
            assert dev
            try:
                capi.check(L.ffhip_memcpy_h2d(dev, got.ctypes.data, got.nbytes, None), "ffhip_memcpy_h2d")
                capi.sync(None)
                rc = L.ffhip_jpeg_decode_files_device(ptrs, lens, n, n_threads, C.byref(geom), dev, pitch, stride, status, SF.h(s))
                capi.sync(SF.h(s))
                capi.check(L.ffhip_memcpy_d2h(got.ctypes.data, dev, got.nbytes, None), "ffhip_memcpy_d2h")
                capi.sync(None)
            finally:
                L.ffhip_free(dev)
        assert rc == 0 and not any(status), (rc, list(status))
        assert (geom.mcu_cols, geom.mcu_rows) == (known[0].mc, known[0].mr)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    return run


def uniform_file_sets(seed=16):
    rng = np.random.default_rng(seed)
    small = [written_file(rng, 67, 35, "420", r) for r in (0, 3, 0, 7, 0)]
    larger = [written_file(rng, 301, 47, "420", 0) for _ in range(7)]         # no restart markers: the subsequence decoder's batch
    marked = [written_file(rng, 301, 47, "420", 2) for _ in range(4)]         # an interval every two MCUs: the interval kernel's
    return small, larger, marked


@pytest.fixture(scope="module")
def uniform_files():
    return uniform_file_sets()


@pytest.mark.parametrize("entropy", [None, "0"], ids=["device_huffman", "host_threads"])
def test_jpeg_files_of_one_geometry(stream, uniform_files, entropy):
    """ffhip_jpeg_decode_files_device: the device Huffman decoder (the subsequence decoder's sync arrays, the header records, the planes in
    SCRATCH_FILES_DEV), and with FFHIP_JPEG_GPU_ENTROPY=0 the host threads through the calling thread's slots (their planes in
    SCRATCH_FILES_PLANES of the slot streams, which a fill of any stream by this thread reaches)"""
    capi.setenv("FFHIP_JPEG_GPU_ENTROPY", entropy)
    small, larger, marked = uniform_files
    kinds = ["SCRATCH_HUFF", "SCRATCH_HUFF_SYNC", "SCRATCH_FILES_DEV"] if entropy is None else ["SCRATCH_FILES_PLANES"]
    SF.run_protocol(f"jpeg files, one geometry, {entropy}", stream, [uniform_runner(larger, stream), uniform_runner(marked, stream)],
                    [uniform_runner(small, stream), uniform_runner(small[:1], stream), uniform_runner(marked[:2], stream)], kinds)


@pytest.mark.parametrize("entropy", [None, "0"], ids=["device_huffman", "host_threads"])
def test_jpeg_files_through_the_pipeline_slots(uniform_files, entropy):
    """ffhip_jpeg_decode_files: two pictures a chunk, so that both slots take turns (and the second one a last partial chunk); the slots'
    pinned and device planes, tables and pixels -- and, with the device front end, its staging and sync arrays, which are the slot streams'
    too -- are filled with the NULL stream's scratch"""
    capi.setenv("FFHIP_JPEG_GPU_ENTROPY", entropy)
    small, larger, _ = uniform_files
    kinds = ["SCRATCH_FILES_PLANES", "SCRATCH_FILES_PIXELS"] + (["SCRATCH_HUFF", "SCRATCH_HUFF_SYNC"] if entropy is None else [])
    SF.run_protocol(f"jpeg pipeline slots, {entropy}", None, [uniform_runner(larger, None, True, 3)],
                    [uniform_runner(small, None, True, 2), uniform_runner(small[:1], None, True, 0)], kinds)


@pytest.mark.parametrize("entropy", [None, "0"], ids=["device_huffman", "host_threads"])
def test_jpeg_files_of_mixed_sizes_under_every_pixel_rule(stream, jpeg_batch, entropy):
    capi.setenv("FFHIP_JPEG_GPU_ENTROPY", entropy)
    known, files, bad = jpeg_batch
    n = len(files)
    rng = np.random.default_rng(26)
    big = [written_file(rng, 640, 200, "420", 0), written_file(rng, 333, 211, "444", 5), written_file(rng, 97, 203, "grey", 0)]
    larger = [mixed_runner(big, [k.data for k in big], stream),
              mixed_runner(big, [k.data for k in big], stream, "scaled", [2, 1, 2]),
              mixed_runner(big, [k.data for k in big], stream, "libjpeg", flags=capi.FFHIP_JPEG_PIXELS_LIBJPEG)]
    small = [mixed_runner(known, files, stream),
             mixed_runner(known, files, stream, "scaled", [(1, 2, 4, 8)[i % 4] for i in range(n)]),
             mixed_runner(known, files, stream, "libjpeg", flags=capi.FFHIP_JPEG_PIXELS_LIBJPEG)]
    SF.run_protocol(f"jpeg files, mixed, {entropy}", stream, larger, small, ["SCRATCH_FILES_MIXED"])


def progressive_file(c, use_twin=False):
    k = JpegFile(c["twin"] if use_twin else c["file"], c["planes"] + [None] * (3 - c["ncomp"]), c["width"], c["height"],
                 {(3, 2, 2): "420", (3, 1, 1): "444", (3, 2, 1): "422", (3, 4, 1): "h4v1", (1, 1, 1): "grey"}[(c["ncomp"], c["h"], c["v"])], PC.QUANT)
    return k


@pytest.mark.parametrize("gpu", ["1", None], ids=["device_front_end", "host_threads"])
def test_jpeg_progressive_files(stream, gpu):
    """the writer's progressive files and their baseline twins in one call; the 2048 x 1024 file is the larger case"""
    capi.setenv("FFHIP_JPEG_PROGRESSIVE_GPU", gpu)
    cases = PC.writer_cases()
    big = [progressive_file(c) for c in cases if c["width"] == 2048]
    known = [progressive_file(c) for c in cases if c["width"] != 2048] + [progressive_file(c, True) for c in cases[:4]]
    assert len(big) == 1 and len(known) == len(cases) - 1 + 4
    flags = capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE
    SF.run_protocol(f"jpeg progressive, {gpu}", stream, [mixed_runner(big, [k.data for k in big], stream, flags=flags)],
                    [mixed_runner(known, [k.data for k in known], stream, flags=flags)], ["SCRATCH_HUFF_PROG"] if gpu else ["SCRATCH_FILES_MIXED"])


def jpeg_tensor_runs(batch, stream=None, n_threads=4):
    """ffhip_jpeg_decode_files_tensor, _tensor_resized (test_resize_gpu.check_files on the oracle's pictures) and _tensor_oriented on the
    files of jpeg_batch_files -> (plain_tensors, resized, oriented); on the NULL stream unless one is given"""
    L = capi.lib()
    known, files, bad = batch
    n = len(files)
    images = [None if k is None else k.shown() for k in known]
    f16, u8 = make_format(F16, 1, 0), make_format(U8, 0, 1)

    def plain_tensors():
        shapes = [(1, 1) if im is None else im.shape[:2] for im in images]
        SF.tensor_files_call(lambda ptrs, lens, n_, fmt, outs, status: L.ffhip_jpeg_decode_files_tensor(ptrs, lens, n_, n_threads, fmt, outs, None, None, status,
                                                                                                        SF.h(stream)), files, f16, shapes, images, SF.h(stream))

    def resized():
        check_files("ffhip_jpeg_decode_files_tensor_resized", (files, images, bad), u8, AA, per_file_sizes(n), inner_rois(images, bad), stream=SF.h(stream),
                    n_threads=n_threads)
        check_files("ffhip_jpeg_decode_files_tensor_resized", (files, images, bad), f16, BIL, [(32, 32)] * n, stream=SF.h(stream), n_threads=n_threads)

    def oriented():
        for o, size in ((6, None), (5, (24, 40)), (3, (17, 9))):
            orient = (C.c_int * n)(*([o] * n))
            keys, shapes = [], []
            for im in images:
                if im is None:
                    keys.append(None)
                    shapes.append(size or (1, 1))
                    continue
                stored = im
                if size:                                                  # the resize works in stored axes: an upright h x w is w x h there from 5 on
                    sh, sw = (size[1], size[0]) if o >= 5 else size
                    stored = resize_rule(im, sh, sw, AA)
                keys.append(X.orient(stored, o))
                shapes.append(keys[-1].shape[:2])
            sizes = (capi.Size * n)(*[capi.Size(size[1], size[0]) for _ in range(n)]) if size else None
            SF.tensor_files_call(lambda ptrs, lens, n_, fmt, outs, status: L.ffhip_jpeg_decode_files_tensor_oriented(
                ptrs, lens, n_, n_threads, fmt, outs, None, sizes, AA, None, None, orient, None, None, status, SF.h(stream)), files, f16, shapes, keys,
                SF.h(stream))
    return plain_tensors, resized, oriented


def test_jpeg_files_to_tensors(jpeg_batch):
    """ffhip_jpeg_decode_files_tensor, _tensor_resized and _tensor_oriented: the NULL stream's"""
    plain_tensors, resized, oriented = jpeg_tensor_runs(jpeg_batch)

    def larger():
        capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
        resized()
        oriented()

    def parts():
        capi.setenv("FFHIP_TENSOR_PART_BYTES", 1)                            # every file a part of its own: the parts' pictures reuse the scratch
        plain_tensors()
        resized()
        capi.setenv("FFHIP_TENSOR_PART_BYTES", None)
    SF.run_protocol("jpeg files to tensors", None, [larger], [plain_tensors, resized, oriented, parts],
                    ["SCRATCH_TENSOR_ITEMS", "SCRATCH_TENSOR_BGRA", "SCRATCH_RESIZE_ITEMS", "SCRATCH_RESIZE_BGRA", "SCRATCH_ORIENT_ITEMS", "SCRATCH_ORIENT_BGRA"])


# ---------------------------------------------------------------------------------------------------- VP8 and lossy WebP
def test_vp8_stages(stream):
    """ffhip_vp8_residual_batch, _predict_recon, _loopfilter, _predict_loopfilter (both filter types) and ffhip_vp8_decode_items with the
    inputs of their stream-order cases"""
    s = stream

    def residual():
        lv, info = synth.vp8_macroblocks(9, seed=9, adversarial=True)
        q = synth.vp8_quant(seed=9)
        want = oracle_residual(lv, info, q)
        bufs = [ops.DeviceBuffer(host=np.ascontiguousarray(a)) for a in (lv, info, q)]
        out = ops.DeviceBuffer(host=np.full(want.nbytes + 64, SF.FILL, np.uint8))
        capi.check(capi.lib().ffhip_vp8_residual_batch(9, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, out.ptr, s), "ffhip_vp8_residual_batch")
        capi.sync(s)
        got = out.to_host((want.nbytes + 64,), np.uint8)
        assert np.array_equal(got[:want.nbytes], SO.as_bytes(want)) and (got[want.nbytes:] == SF.FILL).all()
    cases = [residual, plain(TSO.vp8_predict_case(), s), plain(TSO.vp8_loopfilter_case(), s), plain(TSO.vp8_side_by_side_case(1), s, retry_ok=True),
             plain(TSO.vp8_side_by_side_case(2), s, retry_ok=True), plain(TSO.vp8_items_case(), s)]
    SF.run_protocol("vp8 stages", s, cases, cases, ["SCRATCH_VP8_PRED", "SCRATCH_VP8_LF", "SCRATCH_VP8_RETRY", "SCRATCH_VP8_ITEMS"])


@pytest.mark.parametrize("form", ["fused", "rows"])
def test_vp8_decode_frames(stream, form):
    capi.setenv("FFHIP_VP8_FRAMES", form)
    case = plain(TSO.vp8_frames_case(form), stream, retry_ok=True)
    SF.run_protocol(f"vp8 decode_frames {form}", stream, [case], [case], ["SCRATCH_VP8_FRAMES"] if form == "fused" else ["SCRATCH_VP8_PRED", "SCRATCH_VP8_LF"])


def front_key(name):
    w, h, _ = [int(x) for x in FRONT[f"{name}_dims"]]
    return FRONT[f"{name}_bgra"][:h, :4 * w].reshape(h, w, 4)


_WITNESS = {}


def witness_bgr(data):
    """the colour of a lossy file under the libwebp rule by tests/vp8_spec.py, as BGR; once per stream of bytes"""
    if data not in _WITNESS:
        _WITNESS[data] = np.ascontiguousarray(vp8_spec.decode(data, vp8_spec.SPEC)["rgb"][:, :, ::-1])
    return _WITNESS[data]


def opaque(bgr, alpha=None):
    a = np.full(bgr.shape[:2] + (1,), 255, np.uint8) if alpha is None else alpha[..., None]
    return np.ascontiguousarray(np.concatenate([bgr, a], axis=2))


def webp_runner(files, keys, s, flags=0, statuses=None, n_threads=4):
    """ffhip_webp_decode_files_device[_ex] over framed outputs: the reference rule writes the macroblock grid, the libwebp rule width x height
    of it (the frame is the grid's either way: the call asks for a pitch of 64 bytes a macroblock column)"""
    L = capi.lib()
    pixels = "libwebp" if flags else "reference"
    places = []
    for f in files:
        try:
            w, h, c, r = ops.webp_probe(f, pixels)
        except capi.FfhipError:
            w = h = c = r = 1
        places.append((64 * c, 16 * r, 4 * w, h) if flags else (64 * c, 16 * r))

    def call(ptrs, lens, n, outs, pitches, status):
        if flags:
            return L.ffhip_webp_decode_files_device_ex(ptrs, lens, n, n_threads, outs, pitches, None, flags, None, status, SF.h(s))
        return L.ffhip_webp_decode_files_device(ptrs, lens, n, n_threads, outs, pitches, None, status, SF.h(s))

    def run():
        SF.files_call(call, files, places, keys, statuses)
        return capi.sync(SF.h(s))
    return run


@pytest.mark.parametrize("entropy", [1, 0], ids=["kernels", "host_threads"])
def test_webp_files_under_both_rules(stream, entropy):
    """the reference rule on the pinned fixtures against the reference's recorded pixels, the libwebp rule on webp_pixels_cases' files
    against PIL's recorded RGB, each with the file truncated inside its last partition in the middle; ffhip_webp_parse_device against the
    host parser"""
    capi.setenv("FFHIP_WEBP_GPU_ENTROPY", entropy)
    ref_files, ref_keys = [file_bytes(n) for n in NAMES], [front_key(n) for n in NAMES]
    mid = len(ref_files) // 2
    ref_files.insert(mid, late_bad())
    ref_keys.insert(mid, None)
    lw_files, lw_keys = [WP.data_of(n) for n in WP.NAMES], [opaque(WP.pil_rgb(n)[:, :, ::-1]) for n in WP.NAMES]
    lw_files.insert(3, late_bad())
    lw_keys.insert(3, None)

    def parse():
        names = NAMES[:6]
        dev, status = ops.webp_parse_device([file_bytes(n) for n in names] + [late_bad()], stream=stream)
        assert status[:-1] == [0] * len(names) and status[-1] == EINVAL
        for n, p in zip(names, dev):
            host = ops.webp_parse(file_bytes(n))
            assert all(np.array_equal(p[k], host[k]) for k in ("modes", "levels", "mbinfo", "resmap", "quant", "filters")), n
    reference = webp_runner(ref_files, ref_keys, stream, 0, {mid: EINVAL})
    libwebp = webp_runner(lw_files, lw_keys, stream, capi.FFHIP_WEBP_PIXELS_LIBWEBP, {3: EINVAL})
    small = [reference, libwebp] + ([parse] if entropy else [])
    SF.run_protocol(f"webp files {entropy}", stream, [reference, libwebp], small, ["SCRATCH_WEBP", "SCRATCH_VP8_ITEMS", "SCRATCH_VP8_LIBWEBP"])


def alpha_key(c):
    bgr = witness_bgr(c.data)
    return opaque(bgr, c.plane)


def test_webp_alpha_planes(stream):
    """FFHIP_WEBP_ALPHA: every case of webp_alpha_cases.py in one call, the damaged files among good ones, and the stream cut inside its
    last token, whose missing bits read as 0 whatever lies behind them"""
    flags = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA
    cs = AK.cases()
    everything = webp_runner([c.data for c in cs], [alpha_key(c) for c in cs], stream, flags)
    good = cs[:8]
    files, keys, statuses = [], [], {}
    for k, d in enumerate(AK.damaged_cases()):
        files += [good[k % 8].data, d.data]
        keys += [alpha_key(good[k % 8]), None]
        statuses[len(files) - 1] = EINVAL
    cut = AK.lenient_end()
    files.append(cut)
    keys.append(opaque(witness_bgr(cut), webp_alpha_spec.plane(cut)))
    damaged = webp_runner(files, keys, stream, flags, statuses)

    def in_parts():
        capi.setenv("FFHIP_WEBP_ALPHA_PART_BYTES", 1)                        # every plane a part of its own
        everything()
        capi.setenv("FFHIP_WEBP_ALPHA_PART_BYTES", None)
    SF.run_protocol("webp alpha", stream, [everything], [everything, damaged, in_parts], ["SCRATCH_WEBP_ALPHA"])


def webp_tensor_runs(stream=None, n_threads=4):
    """ffhip_webp_decode_files_tensor, _tensor_resized, _tensor_oriented (the reference rule, the reference's recorded pixels) and
    ffhip_webp_decode_files_tensor_ex under the libwebp rule (PIL's recorded RGB) -> [plain_tensors, resized, oriented, libwebp_rule]; on the
    NULL stream unless one is given"""
    L = capi.lib()
    files, images = [file_bytes(n) for n in NAMES], [front_key(n) for n in NAMES]
    bad = len(files) // 2
    files.insert(bad, late_bad())
    images.insert(bad, None)
    n = len(files)
    u8 = make_format(U8, 1, 0)
    lw_files, lw_images = [WP.data_of(x) for x in WP.NAMES], [opaque(WP.pil_rgb(x)[:, :, ::-1]) for x in WP.NAMES]

    def shapes_of(ims):
        return [(1, 1) if im is None else im.shape[:2] for im in ims]

    def plain_tensors():
        SF.tensor_files_call(lambda ptrs, lens, n_, fmt, outs, status: L.ffhip_webp_decode_files_tensor(ptrs, lens, n_, n_threads, fmt, outs, None, None, status,
                                                                                                        SF.h(stream)), files, u8, shapes_of(images), images, SF.h(stream))

    def resized():
        check_files("ffhip_webp_decode_files_tensor_resized", (files, images, bad), u8, AA, per_file_sizes(n), inner_rois(images, bad), stream=SF.h(stream),
                    n_threads=n_threads)

    def oriented():
        orient = (C.c_int * n)(*([8] * n))
        keys = [None if im is None else X.orient(im, 8) for im in images]
        SF.tensor_files_call(lambda ptrs, lens, n_, fmt, outs, status: L.ffhip_webp_decode_files_tensor_oriented(
            ptrs, lens, n_, n_threads, fmt, outs, None, None, AA, orient, None, None, status, SF.h(stream)), files, u8, shapes_of(keys), keys, SF.h(stream))

    def libwebp_rule():
        m = len(lw_files)
        orient = (C.c_int * m)(*([6] * m))
        keys = [X.orient(im, 6) for im in lw_images]
        SF.tensor_files_call(lambda ptrs, lens, n_, fmt, outs, status: L.ffhip_webp_decode_files_tensor_ex(
            ptrs, lens, n_, n_threads, fmt, outs, None, None, AA, orient, None, capi.FFHIP_WEBP_PIXELS_LIBWEBP, None, status, SF.h(stream)), lw_files, u8, shapes_of(keys),
            keys, SF.h(stream))
    return [plain_tensors, resized, oriented, libwebp_rule]


def test_webp_files_to_tensors():
    """the four WebP files-to-tensors entries: the NULL stream's"""
    small = webp_tensor_runs()
    SF.run_protocol("webp files to tensors", None, small, small, ["SCRATCH_TENSOR_BGRA", "SCRATCH_RESIZE_BGRA", "SCRATCH_ORIENT_BGRA"])


# ---------------------------------------------------------------------------------------------------- HEVC
def test_hevc_residual_and_intra(stream):
    s = stream
    small = [plain(TSO.hevc_residual_case(4, 777), s), plain(TSO.hevc_residual_case(32, 5), s), plain(TSO.hevc_intra_case(192, 128, 71), s),
             plain(TSO.hevc_intra_case(64, 64, 1), s), plain(TSO.heif_case(), s)]
    big = TSO.hevc_intra_case(*TSO.BIG)
    assert len(big.keep) >= 1 << 15                                          # the forked side stream
    SF.run_protocol("hevc intra", s, [plain(big, s)], small, ["SCRATCH_HEVC_INTRA"])
    TSO.assert_device_planner_took_the_list()


@pytest.mark.parametrize("decode", [False, True], ids=["recon_tiles", "decode_tiles"])
def test_hevc_tile_calls_back_to_back(stream, decode):
    """three calls on one list back to back: both one-chunk scratches and their guard events are crossed behind every fill"""
    run = tiles_runner(decode, stream)
    SF.run_protocol(f"hevc tiles {decode}", stream, [run], [run], ["SCRATCH_HEVC_TILES_ONE"])


def tiles_runner(decode, s, calls=3):
    """`calls` ffhip_hevc_intra_recon_tiles / ffhip_hevc_decode_tiles calls on one list back to back on `s`, every plane against the oracle's"""
    one, drs, sets, outputs_of, expect_of, keep = TSO.hevc_tiles_case(decode, calls)
    want = [[np.array(SO.as_bytes(e)) for e in expect_of(i, "true")] for i in range(calls)]

    def run(s=s):
        L = capi.lib()
        own = isinstance(s, SF.StreamBox)
        s = SF.h(s)
        for i in range(calls):
            for o in outputs_of(i):
                o.refill(s if own else None)
        for op in drs:
            SO.copy(op.dev.ptr, op.true.ptr, op.nbytes, s)
        for i in range(calls):
            for ptr, value, nbytes in sets[i][1]:
                capi.check(L.ffhip_memset(ptr, value, nbytes, s), "ffhip_memset")
            one(i, s)
        assert capi.sync(s) == 0
        for i in range(calls):
            for k, (o, e) in enumerate(zip(outputs_of(i), want[i])):
                got = o.written()
                assert np.array_equal(got, e), (i, k, np.flatnonzero(got != e)[:4].tolist())
    run.keep = keep
    return run


# ---------------------------------------------------------------------------------------------------- PNG and lossless WebP
def lossless_runner(entry, files, keys, sizes, s, statuses=None, n_threads=4):
    L = capi.lib()
    places = [(4 * w, h) for w, h in sizes]

    def run():
        SF.files_call(lambda ptrs, lens, n, outs, pitches, status: getattr(L, entry)(ptrs, lens, n, n_threads, outs, pitches, None, status, SF.h(s)),
                      files, places, keys, statuses)
        return capi.sync(SF.h(s))
    return run


def with_damaged(good_files, good_keys, damaged):
    """every damaged file (name, data, code) between good ones -> files, keys, {index: code}"""
    files, keys, statuses = [], [], {}
    for k, (_, data, code) in enumerate(damaged):
        files += [good_files[k % len(good_files)], data]
        keys += [good_keys[k % len(good_files)], None]
        statuses[len(files) - 1] = code
    return files, keys, statuses


def sizes_of(keys, default=(8, 8)):
    return [default if k is None else (k.shape[1], k.shape[0]) for k in keys]


def tensor_runs(entry, files, images, stream=None, n_threads=4):
    """the tensor entry of PNG / lossless WebP with a rectangle, both resize filters and an imposed orientation: the numpy rules on the
    witness's pictures; on the NULL stream unless one is given"""
    L = capi.lib()
    n = len(files)
    u8 = make_format(U8, 1, 0)

    def call(roi, sizes, filt, orient):
        rects = (capi.Rect * n)(*[capi.Rect(*r) for r in roi]) if roi else None
        out_size = (capi.Size * n)(*[capi.Size(w, h) for h, w in sizes]) if sizes else None
        turn = (C.c_int * n)(*(orient or [1] * n))                         # (NULL would be every file's own tag: one case has an EXIF chunk)
        return lambda ptrs, lens, n_, fmt, outs, status: getattr(L, entry)(ptrs, lens, n_, n_threads, fmt, outs, rects, out_size, filt, turn, None, 0, None, status,
                                                                           SF.h(stream))

    def roi():
        rois = [(w // 3, h // 4, w - w // 3 - w // 5, h - h // 4 - h // 6) for h, w in (im.shape[:2] for im in images)]
        keys = [im[y0:y0 + rh, x0:x0 + rw] for im, (x0, y0, rw, rh) in zip(images, rois)]
        SF.tensor_files_call(call(rois, None, AA, None), files, u8, [k.shape[:2] for k in keys], keys, SF.h(stream))

    def resized():
        for filt in (AA, BIL):
            keys = [resize_rule(im, 32, 32, filt) for im in images]
            SF.tensor_files_call(call(None, [(32, 32)] * n, filt, None), files, u8, [(32, 32)] * n, keys, SF.h(stream))

    def turned():
        keys = [X.orient(im, 6) for im in images]
        SF.tensor_files_call(call(None, None, AA, [6] * n), files, u8, [k.shape[:2] for k in keys], keys, SF.h(stream))
    return [roi, resized, turned]


def test_png_files(stream):
    cs = png_cases.cases()
    files, keys = [c.data for c in cs], list(png_cases.expected())
    everything = lossless_runner("ffhip_png_decode_files_device", files, keys, sizes_of(keys), stream)
    dfiles, dkeys, dcodes = with_damaged(files[:6], keys[:6], [(name, data, EINVAL) for name, data in png_cases.damaged()])
    damaged = lossless_runner("ffhip_png_decode_files_device", dfiles, dkeys, sizes_of(dkeys, (7, 6)), stream, dcodes)

    def in_parts():
        capi.setenv("FFHIP_PNG_PART_BYTES", 1)                               # every file a part of its own: they reuse the staging
        everything()
        assert ops.png_last()[0] == len(files)
        capi.setenv("FFHIP_PNG_PART_BYTES", None)
    SF.run_protocol("png files", stream, [everything], [everything, in_parts, damaged], ["SCRATCH_PNG"])


def test_png_files_to_tensors():
    cs = png_cases.cases()
    runs = tensor_runs("ffhip_png_decode_files_tensor", [c.data for c in cs], list(png_cases.expected()))
    SF.run_protocol("png files to tensors", None, runs, runs, ["SCRATCH_PNG", "SCRATCH_TENSOR_BGRA"])


def test_lossless_webp_files(stream):
    cs = vp8l_cases.cases()
    files, keys = [c.data for c in cs], list(vp8l_cases.expected())
    everything = lossless_runner("ffhip_vp8l_decode_files_device", files, keys, sizes_of(keys), stream)
    dfiles, dkeys, dcodes = with_damaged(files[:6], keys[:6], [(d.name, d.data, d.code) for d in vp8l_cases.damaged_cases()])
    damaged = lossless_runner("ffhip_vp8l_decode_files_device", dfiles, dkeys, sizes_of(dkeys, (5, 4)), stream, dcodes)

    def in_parts():
        capi.setenv("FFHIP_VP8L_PART_BYTES", 1)
        everything()
        assert ops.vp8l_last()[0] == len(files)
        capi.setenv("FFHIP_VP8L_PART_BYTES", None)
    SF.run_protocol("lossless webp files", stream, [everything], [everything, in_parts, damaged], ["SCRATCH_VP8L"])


def test_lossless_webp_files_to_tensors():
    cs = vp8l_cases.cases()
    big = [k for k, c in enumerate(cs) if c.argb.shape[1] >= 5 and c.argb.shape[0] >= 3]        # a rectangle inside them has pixels
    runs = tensor_runs("ffhip_vp8l_decode_files_tensor", [cs[k].data for k in big], [vp8l_cases.expected()[k] for k in big])
    SF.run_protocol("lossless webp files to tensors", None, runs, runs, ["SCRATCH_VP8L", "SCRATCH_TENSOR_BGRA"])


# ---------------------------------------------------------------------------------------------------- items sinks
def test_items_sinks(stream):
    s = stream
    small = [plain(TSO.resize_case(BIL), s), plain(TSO.resize_case(AA), s), plain(TSO.orient_case(), s), plain(TSO.tensor_case(F16, 1), s),
             plain(TSO.tensor_case(U8, 0), s)]
    larger = [plain(TSO.resize_case(AA, 400, 1), s), plain(TSO.orient_case(400, 1), s), plain(TSO.tensor_case(F16, 1, 400, 1), s)]
    SF.run_protocol("items sinks", s, larger, small, ["SCRATCH_RESIZE_ITEMS", "SCRATCH_ORIENT_ITEMS", "SCRATCH_TENSOR_ITEMS"])


# ---------------------------------------------------------------------------------------------------- two threads, a stream each
def test_two_threads_on_their_own_streams_for_the_three_newest_decoders():
    """PNG, lossless WebP and the alpha plane keep their state per (device, stream) like the older decoders: two threads, each with a stream
    it made, decode different halves of the three case lists in three rounds behind a barrier, every picture against its key, and each
    thread fills its own stream's scratch with 0xFF between the rounds"""
    L = capi.require_device(0)
    flags = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA
    png, png_keys = [c.data for c in png_cases.cases()], list(png_cases.expected())
    v8l, v8l_keys = [c.data for c in vp8l_cases.cases()], list(vp8l_cases.expected())
    alp, alp_keys = [c.data for c in AK.cases()], [alpha_key(c) for c in AK.cases()]
    barrier, errors = threading.Barrier(2), []

    def work(t):
        try:
            capi.require_device(0)
            s = L.ffhip_stream_create()
            assert s
            runs = [lossless_runner("ffhip_png_decode_files_device", png[t::2], png_keys[t::2], sizes_of(png_keys[t::2]), s),
                    lossless_runner("ffhip_vp8l_decode_files_device", v8l[t::2], v8l_keys[t::2], sizes_of(v8l_keys[t::2]), s),
                    webp_runner(alp[t::2], alp_keys[t::2], s, flags)]
            for rnd in range(3):
                barrier.wait(timeout=60)
                for run in runs:
                    run()
                if rnd < 2:
                    dev, host, kinds = SF.fill(s, 0xFF)
                    assert dev > 0 and host > 0
                    names = {SF.base_of(k) for k in kinds}
                    assert {"SCRATCH_PNG", "SCRATCH_VP8L", "SCRATCH_WEBP_ALPHA"} <= names, names
            L.ffhip_stream_destroy(s)
        except BaseException as e:  # noqa: BLE001 -- reported below, on the main thread
            errors.append((t, e))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---------------------------------------------------------------------------------------------------- coverage is a condition
def test_every_scratch_kind_was_filled_in_front_of_a_checked_run():
    """enum FfhipScratchKind against what the fills of this module reported in front of checked runs.  Every entry of the enum is reached: the
    one allocation the library does not keep -- what a part of ffhip_webp_decode_files_device larger than WEBP_SCRATCH_KEEP takes for itself
    and frees (ffhip_vp8_bool_gpu.hip, run_part) -- is no kind.  A kind added later without a case here fails this test."""
    table = SF.enum_kinds()
    reached = {SF.base_of(k, table) for k in SF.COVERED}
    assert None not in reached, sorted(SF.COVERED)
    missing = sorted(set(table) - reached)
    assert not missing, (missing, {k: sorted(v) for k, v in SF.COVERED.items()})
