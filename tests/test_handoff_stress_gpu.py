"""GPU: the in-launch hand-offs (VP8 rows, VP8 loop-filter rows, HEVC groups) under UNEVEN load -- a second stream
keeps the memory system busy with large copies while the dependency-scheduled kernels run, and every byte is still
the oracle's.  (MI355X_MICROARCH.md: idle chips and uniform load hide hand-off bugs.)"""
import threading

import numpy as np
import pytest

import oracle_lib as O
from ffpic_amd import capi, ops, synth

pytestmark = pytest.mark.gpu


class Hog:
    """copies 256 MB back and forth on its own stream until stopped"""

    def __init__(self):
        self.L = capi.require_device()
        self.st = self.L.ffhip_stream_create()
        self.a = ops.DeviceBuffer(nbytes=256 << 20)
        self.b = ops.DeviceBuffer(nbytes=256 << 20)
        self.stop = False
        self.count = 0
        self.t = threading.Thread(target=self.run, daemon=True)

    def run(self):
        while not self.stop:
            for _ in range(8):
                capi.check(self.L.ffhip_copy_calibrate(self.b.ptr, self.a.ptr, 256 << 20, self.st))
                capi.check(self.L.ffhip_copy_calibrate(self.a.ptr, self.b.ptr, 256 << 20, self.st))
            capi.check(self.L.ffhip_stream_sync(self.st))
            self.count += 16

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.t.join()
        self.L.ffhip_stream_destroy(self.st)


def test_vp8_rows_and_loopfilter_under_load():
    c, r, n = 120, 68, 3
    modes = np.stack([synth.vp8_modes(c, r, seed=900 + i) for i in range(n)])
    modes[..., 18] = np.random.default_rng(9).integers(0, 4, size=modes[..., 18].shape)
    resid = np.stack([synth.vp8_residual(c * r, seed=900 + i, amplitude=60) for i in range(n)])
    flt = synth.vp8_filters(seed=3)
    exp = [O.oracle_vp8_frame(c, r, modes[i], resid[i]) for i in range(n)]
    with Hog() as hog:
        for _ in range(3):
            got = ops.vp8_predict_recon(c, r, modes, resid)
            for i in range(n):
                for gp, e, name in zip(got, exp[i], "YUV"):
                    assert np.array_equal(gp[i], e), (i, name)
            lf = ops.vp8_loopfilter(c, r, 2, modes, flt, got[0], got[1], got[2])
            for i in range(n):
                p = [np.ascontiguousarray(x).copy() for x in exp[i]]
                O.ffo().ffo_vp8_loopfilter_frame(c, r, 2, np.ascontiguousarray(modes[i]).reshape(-1), np.ascontiguousarray(flt).reshape(-1),
                                                 p[0].reshape(-1), p[1].reshape(-1), p[2].reshape(-1))
                for gp, e, name in zip(lf, p, "YUV"):
                    assert np.array_equal(gp[i], e), ("lf", i, name)
    assert hog.count > 0


def test_hevc_groups_under_load():
    w, h = 512, 384
    tus, res = synth.hevc_intra_tus(w, h, 77, adversarial_masks=True)
    exp = O.oracle_hevc_intra(tus, res, w, h, True, 8, 8)
    with Hog() as hog:
        for _ in range(4):
            got = ops.hevc_intra_recon(tus, res, w, h, True, 8, 8)
            for gp, e, name in zip(got, exp, "YUV"):
                assert np.array_equal(gp, e), name
    assert hog.count > 0


def test_give_up_path_reports_eio_and_the_library_recovers(monkeypatch):
    """The bounded spin of the dependency-scheduled kernels: with the done flag of one TU withheld (test hook
    FFHIP_DEBUG_WITHHOLD_TU), the groups that wait for it run into SPIN_LIMIT, the launch drains (every wave sees the
    abort word), ffhip_stream_sync returns FFHIP_EIO exactly once, and after ffhip_shutdown the same list decodes to the
    oracle's picture again."""
    import oracle_lib as O
    from ffpic_amd import capi, ops, synth
    L = capi.require_device()
    w, h = 256, 192
    tus, res = synth.hevc_intra_tus(w, h, seed=91)
    # a TU of the first coding tree block that later groups read: the last luma TU of the first 64x64 window (the default scheduling window)
    first = [i for i, t in enumerate(tus) if t["cidx"] == 0 and t["x"] < 64 and t["y"] < 64]
    victim = first[-1]
    monkeypatch.setenv("FFHIP_DEBUG_WITHHOLD_TU", str(victim)); capi.reload_env()
    with pytest.raises(capi.FfhipError) as ei:
        ops.hevc_intra_recon(tus, res, w, h, True, 8, 8)           # the wrapper's stream sync sees the abort
    assert "-5" in str(ei.value)
    assert L.ffhip_stream_sync(None) == 0                           # reported once, then clear
    monkeypatch.delenv("FFHIP_DEBUG_WITHHOLD_TU"); capi.reload_env()
    L.ffhip_shutdown()
    capi.require_device()
    got = ops.hevc_intra_recon(tus, res, w, h, True, 8, 8)
    exp = O.oracle_hevc_intra(tus, res, w, h, True, 8, 8)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)


def test_side_by_side_vp8_call_is_repeated_by_the_sync(monkeypatch):
    """ffhip_vp8_predict_loopfilter on a device where the filter's wait for the prediction runs out (test hook FFHIP_DEBUG_VP8_LF_GIVEUP: the fused
    filter launch gives up half-way down every frame): ffhip_stream_sync puts the one column of the planes' former contents the prediction
    reads back, runs prediction and filter one after the other and returns FFHIP_RETRIED (> 0: outputs good, consumers behind the call stale)
    with the bytes of an undisturbed call -- H_PRED in the first column included, whose wrapped read sees that column.  The abort is reported in
    a word of the call's own: the process-wide word stays clear, and a later abort of ANOTHER kernel does not set the retry off again.  With
    FFHIP_VP8_NO_RETRY the sync says FFHIP_EIO, as before round 4."""
    import oracle_lib as O
    from ffpic_amd import capi, ops, synth
    from test_vp8_lf_gpu import oracle_lf
    L = capi.require_device()
    c, r, n = 21, 13, 3
    modes = np.stack([synth.vp8_modes(c, r, seed=1200 + i) for i in range(n)])
    modes.reshape(n, r, c, 20)[:, 1::2, 0, 0] = 3              # every other row starts with the wrapped H_PRED
    resid = np.stack([synth.vp8_residual(c * r, seed=1210 + i) for i in range(n)])
    flt = synth.vp8_filters(seed=31)
    exp = []
    for i in range(n):
        y0, u0, v0 = O.oracle_vp8_frame(c, r, modes[i], resid[i])
        exp.append(oracle_lf(c, r, 2, modes[i], flt, (y0, u0, v0)))
    want = ops.vp8_predict_loopfilter(c, r, modes, resid, 2, flt)          # undisturbed
    assert ops.last_sync_status == 0
    monkeypatch.setenv("FFHIP_DEBUG_VP8_LF_GIVEUP", "1"); capi.reload_env()
    got = ops.vp8_predict_loopfilter(c, r, modes, resid, 2, flt)           # gives up, is repeated inside the wrapper's ffhip_stream_sync
    assert ops.last_sync_status == capi.FFHIP_RETRIED
    for i in range(n):
        for gp, wp, e, name in zip(got, want, exp[i], "YUV"):
            assert np.array_equal(gp[i], e) and np.array_equal(wp[i], e), (i, name)
    assert L.ffhip_stream_sync(None) == 0
    # an abort of some OTHER dependency-scheduled kernel on the stream afterwards is that kernel's FFHIP_EIO, not a second repeat of this call
    tus, res = synth.hevc_intra_tus(256, 192, seed=91)
    first = [i for i, t in enumerate(tus) if t["cidx"] == 0 and t["x"] < 64 and t["y"] < 64]
    monkeypatch.setenv("FFHIP_DEBUG_WITHHOLD_TU", str(first[-1])); capi.reload_env()
    with pytest.raises(capi.FfhipError) as ei:
        ops.hevc_intra_recon(tus, res, 256, 192, True, 8, 8)
    assert "-5" in str(ei.value)
    monkeypatch.delenv("FFHIP_DEBUG_WITHHOLD_TU"); capi.reload_env()
    assert L.ffhip_stream_sync(None) == 0
    monkeypatch.setenv("FFHIP_VP8_NO_RETRY", "1"); capi.reload_env()
    with pytest.raises(capi.FfhipError) as ei:
        ops.vp8_predict_loopfilter(c, r, modes, resid, 2, flt)
    assert "-5" in str(ei.value)
    assert L.ffhip_stream_sync(None) == 0
    monkeypatch.delenv("FFHIP_VP8_NO_RETRY"); monkeypatch.delenv("FFHIP_DEBUG_VP8_LF_GIVEUP"); capi.reload_env()
    again = ops.vp8_predict_loopfilter(c, r, modes, resid, 2, flt)
    assert ops.last_sync_status == 0
    for i in range(n):
        for gp, e in zip(again, exp[i]):
            assert np.array_equal(gp[i], e)


@pytest.mark.parametrize("planes", [False, True])
def test_decode_frames_row_form_repeats_its_colour_conversion(monkeypatch, planes):
    """ffhip_vp8_decode_frames in its row form (prediction || filter, then the planar colour kernel on the same stream) with the filter giving up
    (FFHIP_DEBUG_VP8_LF_GIVEUP): the colour conversion has converted the ABORTED planes by the time ffhip_stream_sync repeats prediction and
    filter -- it belongs to the call, so the retry runs it again behind the filter, and the BGRA is the oracle's (round 4 returned FFHIP_OK with
    the broken run's pixels).  The status is FFHIP_RETRIED all the same: the caller may have enqueued consumers of the BGRA behind the call."""
    from ffpic_amd import capi, ops, synth
    from test_vp8_frames_gpu import oracle_chain
    capi.require_device()
    c, r, n = 21, 13, 3
    modes = np.stack([synth.vp8_modes(c, r, seed=1300 + i) for i in range(n)])
    modes.reshape(n, r, c, 20)[:, 1::2, 0, 0] = 3
    resid = np.stack([synth.vp8_residual(c * r, seed=1310 + i) for i in range(n)])
    flt = synth.vp8_filters(seed=32)
    exp = [oracle_chain(c, r, 2, modes[i], resid[i], flt)[0] for i in range(n)]
    monkeypatch.setenv("FFHIP_VP8_FRAMES", "rows"); capi.reload_env()
    out = ops.vp8_decode_frames(c, r, modes, resid, 2, flt, planes=planes)
    assert ops.last_sync_status == 0
    bgra = out[0] if planes else out
    for i in range(n):
        assert np.array_equal(bgra[i], exp[i]), i
    monkeypatch.setenv("FFHIP_DEBUG_VP8_LF_GIVEUP", "1"); capi.reload_env()
    out = ops.vp8_decode_frames(c, r, modes, resid, 2, flt, planes=planes)
    assert ops.last_sync_status == capi.FFHIP_RETRIED
    bgra = out[0] if planes else out
    for i in range(n):
        assert np.array_equal(bgra[i], exp[i]), i
    monkeypatch.delenv("FFHIP_DEBUG_VP8_LF_GIVEUP"); monkeypatch.delenv("FFHIP_VP8_FRAMES"); capi.reload_env()


class _Calls:
    """An HEVC tile call, a side-by-side VP8 call and (huff=True) a device Huffman batch, with their inputs and outputs in device memory of
    `device` and what each must produce.  Every method binds `device` first, and no ops helper is used: they bind device 0."""

    def __init__(self, device=0, huff=True, hevc_size=(512, 256)):
        from test_oracle_golden import FILES
        from test_vp8_lf_gpu import oracle_lf
        self.L, self.dev, self.ptrs = capi.require_device(device), device, []
        self.w, self.h = hevc_size
        tus, res = synth.hevc_intra_tus(self.w, self.h, seed=41, tu_mix="c5")
        self.tus, self.tf = np.ascontiguousarray(tus), np.zeros(1, np.int64)
        self.d_tus, self.d_res = self._up(self.tus), self._up(res)
        self.hevc_exp = O.oracle_hevc_intra(tus, res, self.w, self.h, True, 8, 8)
        self.hevc_out = [self._alloc(self.w * self.h * 2), self._alloc(self.w * self.h // 2), self._alloc(self.w * self.h // 2)]
        self.c, self.r, self.n = 21, 13, 2
        c, r, n = self.c, self.r, self.n
        self.modes = np.ascontiguousarray(np.stack([synth.vp8_modes(c, r, seed=1400 + i) for i in range(n)]))
        self.modes.reshape(n, r, c, 20)[:, 1::2, 0, 0] = 3
        resid = np.stack([synth.vp8_residual(c * r, seed=1410 + i) for i in range(n)])
        flt = synth.vp8_filters(seed=33)
        self.vp8_exp = [oracle_lf(c, r, 2, self.modes[i], flt, O.oracle_vp8_frame(c, r, self.modes[i], resid[i])) for i in range(n)]
        self.d_modes, self.d_resid, self.d_flt = self._up(self.modes), self._up(np.ascontiguousarray(resid)), self._up(np.ascontiguousarray(flt))
        self.ysz, self.csz = 256 * c * r, 64 * c * r
        self.vp8_out = [self._alloc(n * self.ysz), self._alloc(n * self.csz), self._alloc(n * self.csz)]
        self.huff = huff
        if huff:
            import ctypes as C
            import os
            data = open(os.path.join(os.path.dirname(__file__), "golden", FILES["q85_420_dri"]), "rb").read()
            files = [data] * 3
            self.g, cy, cu, cv, _ = ops.jpeg_entropy_batch(files, n_threads=2)
            self.huff_exp = (cy, cu, cv)
            self.bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
            self.fptrs = (C.c_void_p * len(files))(*[b.ctypes.data for b in self.bufs])
            self.lens = (C.c_size_t * len(files))(*[b.size for b in self.bufs])
            self.status = (C.c_int * len(files))()
            nf, g = len(files), self.g
            self.huff_out = [self._alloc(nf * g.y_blocks * 128), self._alloc(nf * g.c_blocks * 128), self._alloc(nf * g.c_blocks * 128), self._alloc(nf * 512)]
        capi.check(self.L.ffhip_stream_sync(None))

    def _bind(self):
        capi.check(self.L.ffhip_init(self.dev))

    def _alloc(self, nbytes):
        p = self.L.ffhip_malloc(max(nbytes, 16))
        assert p
        self.ptrs.append(p)
        return p

    def _up(self, a):
        p = self._alloc(a.nbytes)
        capi.check(self.L.ffhip_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        return p

    def _down(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        capi.check(self.L.ffhip_memcpy_d2h(out.ctypes.data, p, out.nbytes, None))
        capi.check(self.L.ffhip_stream_sync(None))
        return out

    def enqueue(self, s):
        import ctypes as C
        self._bind()
        L, w, h, c, r, n = self.L, self.w, self.h, self.c, self.r, self.n
        for p, nbytes in zip(self.hevc_out + self.vp8_out, (w * h * 2, w * h // 2, w * h // 2, n * self.ysz, n * self.csz, n * self.csz)):
            capi.check(L.ffhip_memset(p, 0, nbytes, s))
        y, u, v = self.hevc_out
        capi.check(L.ffhip_hevc_intra_recon_tiles(self.tus.ctypes.data, self.d_tus, len(self.tus), self.tf.ctypes.data, 1, self.d_res, y, u, v, w, h, w, w // 2,
                                                  h // 2, w // 2, 8, 8, s))
        y, u, v = self.vp8_out
        capi.check(L.ffhip_vp8_predict_loopfilter(c, r, n, self.modes.ctypes.data, self.d_modes, self.d_resid, c * r * 384, None, 2, self.d_flt, y, u, v,
                                                  self.ysz, self.csz, s))
        if self.huff:
            dy, du, dv, dq = self.huff_out
            capi.check(L.ffhip_jpeg_entropy_batch_gpu(self.fptrs, self.lens, len(self.bufs), 2, C.byref(self.g), dy, du, dv, dq, self.status, s))

    def check(self, tag):
        self._bind()
        w, h, c, r, n = self.w, self.h, self.c, self.r, self.n
        got = [self._down(p, sh, np.int16) for p, sh in zip(self.hevc_out, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))]
        for a, b, name in zip(got, self.hevc_exp, "YUV"):
            assert np.array_equal(a, b), (tag, "hevc", name)
        got = [self._down(p, sh, np.uint8) for p, sh in zip(self.vp8_out, ((n, 16 * r, 16 * c), (n, 8 * r, 8 * c), (n, 8 * r, 8 * c)))]
        for i in range(n):
            for a, b, name in zip(got, self.vp8_exp[i], "YUV"):
                assert np.array_equal(a[i], b), (tag, "vp8", i, name)
        if self.huff:
            assert list(self.status) == [0] * len(self.bufs), tag
            for p, e, name in zip(self.huff_out, self.huff_exp, "YUV"):
                assert np.array_equal(self._down(p, e.shape, np.int16), e), (tag, "huff", name)

    def close(self):
        self._bind()
        for p in self.ptrs:
            self.L.ffhip_free(p)
        self.ptrs = []


def test_stream_churn_frees_what_each_stream_held():
    """16 rounds of: create a stream, an HEVC tile call, a side-by-side VP8 call and a device Huffman batch on it, sync, destroy.  Every output is the
    oracle's, and free device memory after the last round is within one round's scratch of what it was after the first: ffhip_stream_destroy frees
    the stream's entries (scratch, retry record, tile guard) -- a new stream that gets the same handle starts from nothing.  One round's scratch is
    measured on a live stream and must be large (the 2048x1024 tile call's per-pixel programs alone are 8 bytes a sample, 25 MB): a library that
    kept each destroyed stream's scratch would lose 15 of them."""
    torch = pytest.importorskip("torch")
    calls = _Calls(hevc_size=(2048, 1024))
    L = calls.L
    s = L.ffhip_stream_create()                    # the thread's own streams and events are made here, not in the rounds
    calls.enqueue(s)
    assert capi.sync(s) == 0
    L.ffhip_stream_destroy(s)
    before = torch.cuda.mem_get_info(0)[0]
    s = L.ffhip_stream_create()
    calls.enqueue(s)
    assert capi.sync(s) == 0
    one_round = before - torch.cuda.mem_get_info(0)[0]   # the scratch of one live stream
    assert one_round >= 16 << 20, one_round
    L.ffhip_stream_destroy(s)
    free = []
    for rnd in range(16):
        s = L.ffhip_stream_create()
        assert s
        calls.enqueue(s)
        assert capi.sync(s) == 0, rnd
        calls.check(rnd)
        L.ffhip_stream_destroy(s)
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[-1] >= free[0] - one_round, (one_round, free)
    calls.close()


def test_stream_destroy_waits_for_queued_work():
    """ffhip_stream_destroy on a stream with work still queued (an HEVC tile call and a side-by-side VP8 call behind large copies; the Huffman batch
    is left out: it waits for its stream before it returns) returns once that work has run: an event recorded behind the work is pending when
    destroy is called and complete when it returns, and the outputs are complete.  A stream created next decodes bit for bit."""
    torch = pytest.importorskip("torch")
    calls = _Calls(huff=False)
    L = calls.L
    a, b = ops.DeviceBuffer(nbytes=256 << 20), ops.DeviceBuffer(nbytes=256 << 20)
    s = L.ffhip_stream_create()
    for _ in range(64):
        capi.check(L.ffhip_copy_calibrate(b.ptr, a.ptr, 256 << 20, s))
    calls.enqueue(s)
    done = torch.cuda.Event()
    done.record(torch.cuda.ExternalStream(s))
    assert not done.query()                        # the work is still queued ...
    L.ffhip_stream_destroy(s)                      # (no sync in front of it)
    assert done.query()                            # ... and has run when destroy returns
    calls.check("destroyed")
    s = L.ffhip_stream_create()
    calls.enqueue(s)
    assert capi.sync(s) == 0
    calls.check("next")
    L.ffhip_stream_destroy(s)
    calls.close()


def test_null_stream_calls_alternating_between_two_devices():
    """One thread, null-stream HEVC tile and side-by-side VP8 calls on device 0, then 1, then 0 ...: the library's state of the null stream is per
    device (scratch, retry record, tile guard), and so is the thread's side stream -- every output is the oracle's."""
    L = capi.lib()
    if L.ffhip_device_count() < 2:
        pytest.skip("needs two devices")
    calls = [_Calls(d, huff=False) for d in (0, 1)]
    for rnd in range(6):
        k = calls[rnd & 1]
        k.enqueue(None)
        assert capi.sync(None) == 0, rnd
        k.check(rnd)
    for k in calls:
        k.close()
    capi.require_device(0)


def test_jpeg_file_calls_alternating_between_two_devices():
    """One thread, ffhip_jpeg_decode_files (pageable destination, two pictures a chunk) and ffhip_jpeg_decode_files_device on device 0, then 1,
    then 0 ...: the thread's two slots -- their streams, and the planes, pixels and front-end scratch the library keeps under them -- are per
    device like the rest of its state.  Six rounds with the device front end and six with host threads; behind the third round every byte
    of what the library keeps on either device is set to 0xFF.  Every picture is the answer key's, with the 0xA5 around it intact."""
    import ctypes as C

    import test_scratch_fill_gpu as F
    L = capi.lib()
    if L.ffhip_device_count() < 2:
        pytest.skip("needs two devices")
    small, larger, _ = F.uniform_file_sets()
    runs = [[F.uniform_runner(larger, None, True, 2, device=d), F.uniform_runner(small, None, True, 2, device=d),
             F.uniform_runner(larger, None, device=d), F.uniform_runner(small, None, device=d)] for d in (0, 1)]
    try:
        for entropy in (None, "0"):
            capi.setenv("FFHIP_JPEG_GPU_ENTROPY", entropy)              # before the rounds start
            for rnd in range(6):
                for run in runs[rnd & 1]:
                    run()
                if rnd == 2:
                    for d in (0, 1):
                        capi.require_device(d)
                        nbytes, kinds = (C.c_uint64 * 2)(), (C.c_int * 256)()
                        assert L.ffhip_debug_scratch_fill(None, 0xFF, nbytes, kinds, 256) > 0 and nbytes[0] > 0 and nbytes[1] > 0, (entropy, d)
    finally:
        capi.setenv("FFHIP_JPEG_GPU_ENTROPY", None)
        capi.require_device(0)
