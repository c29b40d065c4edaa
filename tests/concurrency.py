"""What test_concurrent_gpu.py shares: the schedule by which every pair of families of entry points meets on different host threads, the
crew of caller threads, and the families' runners.  Importing this module needs neither a GPU nor the library (tests/test_concurrent.py).

The contract under test (include/ffpic_hip.h, "Threads and streams"): calls of different host threads, each on a stream of its own, may be
in flight together.  A FAMILY is a list of runners -- closures that make one call of the library on a given stream, wait for it and compare
every byte of the output, the 0xA5 around it included, with an answer key that is no run of the library (test_scratch_fill_gpu.py has
them; they are reused here).  Every thread has its own instances: its own device buffers, its own seed where the factory takes one.

Placement rules, which Crew holds and test_concurrent.py asserts with a recording stand-in for the library:
  stream  every runner of a thread runs on the ONE stream that thread created (a scratch_fill.StreamBox, filled in by the thread); no two
          threads share a stream, and none uses the NULL stream for a library call that takes a stream;
  device  a thread binds device 0 first (capi.require_device), creates its stream with ffhip_stream_create and destroys it with
          ffhip_stream_destroy when it ends.
Runners, inputs and answer keys are built on the main thread and run once there (`prime`) before any thread starts: the oracle, the
witnesses and PIL never run concurrently; threads only call run().  What a runner still computes when it runs is the numpy rule of
test_resize_gpu.py, whose tables that first run has filled.  The runners read their outputs back with blocking copies on the NULL stream,
which is the HIP runtime's business and touches no state of the library."""
import itertools
import threading
import time

# the families of test_concurrent_gpu.py's first test, in the order the schedule is made from
FAMILIES = [
    "jpeg_items", "jpeg_libjpeg", "jpeg_batch", "colour_heif", "hevc_residual", "hevc_intra", "hevc_tiles", "vp8_rows", "vp8_side_by_side",
    "vp8_frames", "vp8_items", "items_sinks", "jpeg_files_mixed", "jpeg_files_uniform", "jpeg_progressive", "webp_files", "webp_alpha", "png",
    "vp8l", "jpeg_tensors", "webp_tensors", "lossless_tensors", "host_entry_blocks",
]
THREADS = 4
N_THREADS = 2           # host threads inside a file call: four callers stay within 16 CPUs


def pair(a, b):
    return (a, b) if a <= b else (b, a)


def pairs_of(families):
    """every unordered pair, a family with itself included"""
    return {pair(a, b) for a in families for b in families}


def pairs_in(rnd):
    """the pairs that meet in a round: one per two PLACES, so that a family meets itself only where two threads run it"""
    return {pair(a, b) for a, b in itertools.combinations(rnd, 2)}


def schedule(families, threads=THREADS, need=None):
    """rounds [[family of thread 0, .., family of thread threads-1]] in which every pair of `need` (default: every unordered pair of
    `families`, a family with itself included) shares a round.  Greedy and deterministic: a round starts from the first pair still
    missing (in the order of `families`) and every further place goes to the family that adds most missing pairs, the first on a tie."""
    families = list(families)
    assert threads >= 2 and families and len(set(families)) == len(families)
    rank = {f: i for i, f in enumerate(families)}
    need = {pair(a, b) for a, b in (pairs_of(families) if need is None else need)}
    rounds = []
    while need:
        rnd = sorted(min(need, key=lambda p: sorted((rank[p[0]], rank[p[1]]))), key=rank.get)
        while len(rnd) < threads:
            left = need - pairs_in(rnd)
            gains = [len({pair(f, g) for g in rnd} & left) for f in families]
            rnd.append(families[gains.index(max(gains))])
        need -= pairs_in(rnd)
        rounds.append(rnd)
    return rounds


# ---------------------------------------------------------------------------------------------------- the crew of caller threads
class Api:
    """what a crew thread needs of the library; test_concurrent.py has a recording stand-in"""

    def require_device(self, device):
        from ffpic_amd import capi
        return capi.require_device(device)

    def stream_create(self):
        from ffpic_amd import capi
        s = capi.lib().ffhip_stream_create()
        assert s
        return s

    def stream_destroy(self, s):
        from ffpic_amd import capi
        capi.lib().ffhip_stream_destroy(s)


_SYNCED = threading.local()


class timed_syncs:
    """while it is entered, capi.sync notes on the calling thread when it returned: the end of a thread's interval is its last sync"""

    def __enter__(self):
        from ffpic_amd import capi
        self.capi, self.real = capi, capi.sync

        def sync(stream=None):
            rc = self.real(stream)
            _SYNCED.at = time.perf_counter()
            return rc
        capi.sync = sync
        return self

    def __exit__(self, *exc):
        self.capi.sync = self.real
        return False


class Crew:
    """`n` caller threads with a stream each.  boxes[t] is thread t's stream (a StreamBox, empty until the thread has made it).
    round(jobs, reps): thread t calls every callable of jobs[t] in turn, `reps` times over, all threads released by one barrier; ->
    [(start, end, [what the callables returned])] per thread, times by time.perf_counter(): the first call, and the last sync (or the last
    return where no runner synced).  An error in a thread aborts the barriers and is raised by round() on the main thread."""

    def __init__(self, n, api=None, boxes=None, wait=120):
        from scratch_fill import StreamBox
        self.n, self.api, self.wait = n, api or Api(), wait
        self.boxes = boxes or [StreamBox() for _ in range(n)]
        self.labels = None
        self.go, self.done = threading.Barrier(n + 1), threading.Barrier(n + 1)
        self.jobs, self.reps, self.results, self.errors = None, 1, [None] * n, []
        self.threads = [threading.Thread(target=self._work, args=(t,)) for t in range(n)]

    def __enter__(self):
        for th in self.threads:
            th.start()
        self._meet(self.done)                          # every thread has its stream
        return self

    def __exit__(self, *exc):
        self.jobs = None
        try:
            self.go.wait(timeout=self.wait)
        except threading.BrokenBarrierError:
            pass
        for th in self.threads:
            th.join()
        return False

    def _meet(self, barrier):
        try:
            barrier.wait(timeout=self.wait)
        except threading.BrokenBarrierError:
            pass
        if self.errors:
            raise AssertionError(f"caller threads failed: {self.errors}")
        assert not barrier.broken, "a barrier broke without an error: a thread did not arrive in time"

    def _work(self, t):
        s = None
        try:
            self.api.require_device(0)
            s = self.boxes[t].handle = self.api.stream_create()
            self.done.wait(timeout=self.wait)
            while True:
                self.go.wait(timeout=self.wait)
                if self.jobs is None:
                    break
                _SYNCED.at = None
                got, start = [], time.perf_counter()
                for _ in range(self.reps):
                    for run in self.jobs[t]:
                        got.append(run())
                end = time.perf_counter()
                self.results[t] = (start, _SYNCED.at or end, got)
                self.done.wait(timeout=self.wait)
        except threading.BrokenBarrierError:
            pass
        except BaseException as e:  # noqa: BLE001 -- raised by round(), on the main thread
            self.errors.append((t, self.labels[t] if self.labels else None, repr(e)))
            self.go.abort()
            self.done.abort()
        finally:
            if s is not None:
                self.api.stream_destroy(s)
                self.boxes[t].handle = None

    def round(self, jobs, reps=1, labels=None):
        assert len(jobs) == self.n
        self.jobs, self.reps, self.labels = [list(j) for j in jobs], reps, labels
        self._meet(self.go)
        self._meet(self.done)
        return list(self.results)


def overlap(a, b):
    """do the intervals (start, end, ..) intersect?"""
    return max(a[0], b[0]) <= min(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- the families' runners
def named(case, t):
    """a Case of test_stream_order_gpu.py under a name of thread t's own: the memo of answer keys (test_scratch_fill_gpu._EXPECT) is by name"""
    case.name = f"{case.name} [thread {t}]"
    return case


class Shared:
    """what the threads' runners share because it is only read: files and their answer keys, made once on the main thread"""

    def __init__(self):
        import png_cases
        import progressive_cases as PC
        import test_scratch_fill_gpu as F
        import vp8l_cases
        import webp_alpha_cases as AK
        import webp_pixels_cases as WP
        from test_webp_files_gpu import late_bad
        from test_webp_front_capi import NAMES, file_bytes
        cases = PC.writer_cases()
        self.progressive = [F.progressive_file(c) for c in cases if c["width"] != 2048] + [F.progressive_file(c, True) for c in cases[:4]]
        self.ref_files, self.ref_keys = [file_bytes(n) for n in NAMES], [F.front_key(n) for n in NAMES]
        self.ref_bad = len(self.ref_files) // 2
        self.ref_files.insert(self.ref_bad, late_bad())
        self.ref_keys.insert(self.ref_bad, None)
        self.lw_files, self.lw_keys = [WP.data_of(n) for n in WP.NAMES], [F.opaque(WP.pil_rgb(n)[:, :, ::-1]) for n in WP.NAMES]
        self.lw_files.insert(3, late_bad())
        self.lw_keys.insert(3, None)
        self.alpha_files, self.alpha_keys = [c.data for c in AK.cases()], [F.alpha_key(c) for c in AK.cases()]
        self.png_files, self.png_keys = [c.data for c in png_cases.cases()], list(png_cases.expected())
        cs = vp8l_cases.cases()
        self.vp8l_files, self.vp8l_keys = [c.data for c in cs], list(vp8l_cases.expected())
        self.vp8l_big = [k for k, c in enumerate(cs) if c.argb.shape[1] >= 5 and c.argb.shape[0] >= 3]


def host_entry_runner(t, calls=4):
    """ffhip_jpeg_recon_batch_host on planes of thread t's own against the oracle, and `calls` block operations of every kind on blocks of
    its own (block_calls)"""
    import numpy as np
    import oracle_lib as O
    from ffpic_amd import capi, ops, synth
    q = synth.quant_tables()
    mc, mr, n = 5, 4, 2
    planes = synth.coef_batch(n, mc, mr, 3, 2, 2, first=3 + 16 * t)
    want = O.oracle_jpeg_recon(O.make_geom(mc, mr, 3, 2, 2), *planes, q, n_images=n)
    blocks = block_calls(t, calls)

    def run():
        got = ops.jpeg_recon_batch_host(capi.jpeg_geom(mc, mr, 3, 2, 2), n, *planes, q)
        assert np.array_equal(np.asarray(got).reshape(want.shape), want), ("jpeg_recon_batch_host", t)
        blocks()
    return run


CS_PAIRS = ((1, 1), (2, 2), (1, 2), (2, 1), (1, 4), (4, 1), (1, 3))       # (v, h) of the colour table's calls


def block_calls(t, calls):
    """`calls` calls of each block operation -- idct_8x8 and idct_4x4 through ffhip_accl_ops_get(), both through the ffhip_get_dct_ops(16)
    table, YUV_to_BGRA32 of ffhip_get_cs_ops(16) at the (v, h) of CS_PAIRS, ffhip_idct_4x4_hevc at two bit depths -- each on a block that no
    other thread and no other call has (seeded by thread, kind and call), against the oracle's answer for THAT block, computed here: another
    thread's block, or a block transformed twice, is a different answer."""
    import numpy as np
    import oracle_lib as O
    from ffpic_amd import capi
    ffo = O.ffo()
    rng = np.random.default_rng(9000 + t)
    todo = []
    for k in range(calls):
        b8 = rng.integers(-300, 300, 64).astype(np.int16)
        b8[0] = 1024 + 8 * (t * calls + k)                                # (a DC of its own: no two blocks agree in many outputs)
        e8 = b8.copy()
        ffo.ffo_idct_8x8_16(e8)
        b4 = rng.integers(-500, 500, 16).astype(np.int16)
        e4 = b4.copy()
        ffo.ffo_vp8_idct_4x4(e4)
        bh = rng.integers(-400, 400, 16).astype(np.int16)
        bd, epp = (8, 10)[k % 2], (k // 2) % 2
        eh = np.zeros(16, np.int16)
        ffo.ffo_hevc_idct_4x4_dst(bh, eh, bd, epp)
        v, h = CS_PAIRS[(k + t) % len(CS_PAIRS)]
        Y = rng.integers(0, 256, 64 * v * h).astype(np.int16)
        U, V = rng.integers(0, 256, 64).astype(np.int16), rng.integers(0, 256, 64).astype(np.int16)
        ec = np.zeros((8 * v, 8 * h * 4), np.uint8)
        ffo.ffo_yuv_to_bgra32_mcu16(ec.reshape(-1), 8 * h * 4, Y, U, V, v, h)
        todo.append((b8, e8, b4, e4, bh, eh, bd, epp, Y, U, V, v, h, ec))

    def run():
        L = capi.lib()
        accl, dct, cs = L.ffhip_accl_ops_get(), L.ffhip_get_dct_ops(16), L.ffhip_get_cs_ops(16)
        assert accl and dct and cs
        for k, (b8, e8, b4, e4, bh, eh, bd, epp, Y, U, V, v, h, ec) in enumerate(todo):
            for table in (accl.contents, dct.contents):
                g8, g4 = b8.copy(), b4.copy()
                table.idct_8x8(g8.ctypes.data, 8)
                table.idct_4x4(g4.ctypes.data, 8)
                assert np.array_equal(g8, e8), ("idct_8x8", t, k)
                assert np.array_equal(g4, e4), ("idct_4x4", t, k)
            gh = np.full(16, 0x5a5a, np.int16)
            L.ffhip_idct_4x4_hevc(bh.ctypes.data, gh.ctypes.data, bd, bool(epp))
            assert np.array_equal(gh, eh), ("idct_4x4_hevc", t, k)
            gc = np.full_like(ec, 0xA5)
            cs.contents.YUV_to_BGRA32(gc.ctypes.data, 8 * h * 4, Y.ctypes.data, U.ctypes.data, V.ctypes.data, v, h)
            assert np.array_equal(gc, ec), ("YUV_to_BGRA32", t, k, v, h)
    return run


def build_families(t, s, shared):
    """{family: [runner]} of thread t on its stream `s` (a StreamBox); "vp8_frames" is {form: [runner]} for the two forms of
    ffhip_vp8_decode_frames, of which for_form() picks the configuration's.  Sizes are the small cases' of test_stream_order_gpu.py and
    test_scratch_fill_gpu.py; nothing larger is needed for this property."""
    import test_scratch_fill_gpu as F
    import test_stream_order_gpu as TSO
    from ffpic_amd import capi
    from test_resize_gpu import AA, BIL, F16, U8
    nt = N_THREADS

    def p(case, **kw):
        return F.plain(named(case, t), s, **kw)
    batch = F.jpeg_batch_files(6 + t)
    known, files, _ = batch
    small, _, marked = F.uniform_file_sets(16 + t)
    n = len(files)
    alpha = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA
    sh = shared
    prog = sh.progressive[t % 2::2] + sh.progressive[:2]                   # a progressive share of its own
    tiles = F.tiles_runner(bool(t & 1), s, calls=2)
    png_t = F.tensor_runs("ffhip_png_decode_files_tensor", sh.png_files[t::2], sh.png_keys[t::2], s, nt)
    big = sh.vp8l_big[t % 2::2]
    vp8l_t = F.tensor_runs("ffhip_vp8l_decode_files_tensor", [sh.vp8l_files[k] for k in big], [sh.vp8l_keys[k] for k in big], s, nt)
    fam = {
        "jpeg_items": [p(TSO.jpeg_items_case("jpeg_recon_items", TSO.JPEG_SPECS, seed=t)),
                       p(TSO.jpeg_items_case("jpeg_recon_items_scaled d2", TSO.JPEG_SMALL, 2, seed=t, many=True)),
                       p(TSO.jpeg_items_case("jpeg_recon_items_scaled d8", TSO.JPEG_SMALL, 8, seed=t, many=True))],
        "jpeg_libjpeg": [p(TSO.jpeg_items_libjpeg_case("jpeg_recon_items_libjpeg", TSO.JPEG_SMALL, seed=t), memo=False)],
        "jpeg_batch": [p(TSO.jpeg_batch_case(2, 2, 5, 4)), p(TSO.jpeg_batch_case(3, 1, 3, 2))],
        "colour_heif": [p(TSO.colour_case(8)), p(TSO.colour_case(16)), p(TSO.colour_case(400)), p(TSO.heif_case())],
        "hevc_residual": [p(TSO.hevc_residual_case(4, 777))],
        "hevc_intra": [p(TSO.hevc_intra_case(192, 128, 71 + t))],
        "hevc_tiles": [tiles],
        "vp8_rows": [p(TSO.vp8_predict_case()), p(TSO.vp8_loopfilter_case())],
        "vp8_side_by_side": [p(TSO.vp8_side_by_side_case(1), retry_ok=True), p(TSO.vp8_side_by_side_case(2), retry_ok=True)],
        "vp8_frames": {form: [p(TSO.vp8_frames_case(form), retry_ok=True)] for form in ("fused", "rows")},
        "vp8_items": [p(TSO.vp8_items_case())],
        "items_sinks": [p(TSO.resize_case(BIL, seed=t)), p(TSO.resize_case(AA, seed=t)), p(TSO.orient_case(seed=t)), p(TSO.tensor_case(F16, 1, seed=t)),
                        p(TSO.tensor_case(U8, 0, seed=t))],
        "jpeg_files_mixed": [F.mixed_runner(known, files, s, n_threads=nt),
                             F.mixed_runner(known, files, s, "scaled", [(1, 2, 4, 8)[(i + t) % 4] for i in range(n)], n_threads=nt),
                             F.mixed_runner(known, files, s, "libjpeg", flags=capi.FFHIP_JPEG_PIXELS_LIBJPEG, n_threads=nt)],
        "jpeg_files_uniform": [F.uniform_runner(small, s, n_threads=nt), F.uniform_runner(marked[:2], s, n_threads=nt)],
        "jpeg_progressive": [F.mixed_runner(prog, [k.data for k in prog], s, flags=capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE, n_threads=nt)],
        "webp_files": [F.webp_runner(sh.ref_files, sh.ref_keys, s, 0, {sh.ref_bad: capi.FFHIP_EINVAL}, n_threads=nt),
                       F.webp_runner(sh.lw_files, sh.lw_keys, s, capi.FFHIP_WEBP_PIXELS_LIBWEBP, {3: capi.FFHIP_EINVAL}, n_threads=nt)],
        "webp_alpha": [F.webp_runner(sh.alpha_files[t % 2::2], sh.alpha_keys[t % 2::2], s, alpha, n_threads=nt)],
        "png": [F.lossless_runner("ffhip_png_decode_files_device", sh.png_files[t % 2::2], sh.png_keys[t % 2::2], F.sizes_of(sh.png_keys[t % 2::2]), s,
                                  n_threads=nt)],
        "vp8l": [F.lossless_runner("ffhip_vp8l_decode_files_device", sh.vp8l_files[t % 2::2], sh.vp8l_keys[t % 2::2], F.sizes_of(sh.vp8l_keys[t % 2::2]), s,
                                   n_threads=nt)],
        "jpeg_tensors": list(F.jpeg_tensor_runs(batch, s, nt)),
        "webp_tensors": F.webp_tensor_runs(s, nt),
        "lossless_tensors": [png_t[0], png_t[2], vp8l_t[1]],
        "host_entry_blocks": [host_entry_runner(t)],
    }
    assert list(fam) == FAMILIES
    return fam


def for_form(families, form):
    return {name: (runs[form] if name == "vp8_frames" else runs) for name, runs in families.items()}


def prime(families, box, stream):
    """every runner once on the main thread, on the main thread's `stream`: the answer keys are computed, the numpy rules' tables filled, and a
    runner that is wrong on its own fails here, not under threads"""
    box.handle = stream
    try:
        for name, runs in families.items():
            for run in runs:
                if hasattr(run, "prime"):
                    run.prime()
                run()
    finally:
        box.handle = None


# ---------------------------------------------------------------------------------------------------- first use, in a process of its own
def first_use_inputs(path):
    """the inputs and answer keys of first_use_child as one .npz at `path`, made by the parent: a side-by-side VP8 call, an HEVC intra list, three
    files for the device Huffman decoder (keys: the host decoder's planes) and the PNG cases (keys: the witness's)"""
    import os

    import numpy as np
    import oracle_lib as O
    import png_cases
    from ffpic_amd import ops, synth
    from test_oracle_golden import FILES
    from test_vp8_lf_gpu import oracle_lf
    c, r, n = 21, 13, 2
    modes = np.ascontiguousarray(np.stack([synth.vp8_modes(c, r, seed=1400 + i) for i in range(n)]))
    modes.reshape(n, r, c, 20)[:, 1::2, 0, 0] = 3
    resid = np.ascontiguousarray(np.stack([synth.vp8_residual(c * r, seed=1410 + i) for i in range(n)]))
    flt = np.ascontiguousarray(synth.vp8_filters(seed=33))
    vp8 = [oracle_lf(c, r, 2, modes[i], flt, O.oracle_vp8_frame(c, r, modes[i], resid[i])) for i in range(n)]
    w, h = 192, 128
    tus, res = synth.hevc_intra_tus(w, h, 71)
    tus = np.ascontiguousarray(tus)
    hevc = O.oracle_hevc_intra(tus, res, w, h, True, 8, 8)
    jpeg = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FILES["q85_420_dri"]), "rb").read()
    _, cy, cu, cv, _ = ops.jpeg_entropy_batch([jpeg] * 3, n_threads=2)
    data = dict(vp8_dims=np.array([c, r, n]), vp8_modes=modes, vp8_resid=resid, vp8_flt=flt, hevc_dims=np.array([w, h]), hevc_tus=tus.view(np.uint8),
                hevc_res=res, jpeg=np.frombuffer(jpeg, np.uint8), huff_y=cy, huff_u=cu, huff_v=cv)
    for k in range(3):
        data[f"vp8_{k}"] = np.stack([p[k] for p in vp8])
        data[f"hevc_{k}"] = hevc[k]
    pngs, keys = png_cases.cases(), png_cases.expected()
    data["png_n"] = np.array(len(pngs))
    for i, (case, key) in enumerate(zip(pngs, keys)):
        data[f"png_file_{i}"], data[f"png_key_{i}"] = np.frombuffer(case.data, np.uint8), key
    np.savez(path, **data)


def first_use_child(path):
    """In a fresh process: the FIRST calls of the library are made by four threads that one barrier releases -- binding the device, the
    process-wide async error word, the registries' first entries, the staging of every decoder are all made under contention.  Each thread has a
    stream of its own and compares its output with the parent's key; one line per thread: "<name> ok" or "<name> FAILED ..."."""
    import ctypes as C

    import numpy as np
    import scratch_fill as SF
    from ffpic_amd import capi, ops
    d = dict(np.load(path))                                            # (read whole here: the archive's reader is not for four threads)
    L = capi.lib()                                                    # loads the library; no call of it yet
    barrier, lines, lock = threading.Barrier(4), [], threading.Lock()

    def download(buf, shape, dtype, s):
        out = np.empty(shape, dtype)
        capi.check(L.ffhip_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, s), "d2h")
        assert capi.sync(s) == 0
        return out

    def vp8(s):
        c, r, n = [int(x) for x in d["vp8_dims"]]
        modes = np.ascontiguousarray(d["vp8_modes"])
        dm, dr, df = ops.DeviceBuffer(host=modes), ops.DeviceBuffer(host=d["vp8_resid"]), ops.DeviceBuffer(host=d["vp8_flt"])
        ysz, csz = 256 * c * r, 64 * c * r
        outs = [ops.DeviceBuffer(nbytes=n * ysz), ops.DeviceBuffer(nbytes=n * csz), ops.DeviceBuffer(nbytes=n * csz)]
        for o in outs:
            capi.check(L.ffhip_memset(o.ptr, 0, o.nbytes, s), "memset")
        capi.check(L.ffhip_vp8_predict_loopfilter(c, r, n, modes.ctypes.data, dm.ptr, dr.ptr, c * r * 384, None, 2, df.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                  ysz, csz, s), "ffhip_vp8_predict_loopfilter")
        rc = capi.sync(s)
        assert rc in (0, capi.FFHIP_RETRIED), rc
        for k, o in enumerate(outs):
            want = d[f"vp8_{k}"]
            assert np.array_equal(download(o, want.shape, np.uint8, s), want), ("plane", k)

    def hevc(s):
        w, h = [int(x) for x in d["hevc_dims"]]
        tus = np.ascontiguousarray(d["hevc_tus"])
        dt, dr = ops.DeviceBuffer(host=tus), ops.DeviceBuffer(host=np.ascontiguousarray(d["hevc_res"]))
        outs = [ops.DeviceBuffer(nbytes=w * h * 2), ops.DeviceBuffer(nbytes=w * h // 2), ops.DeviceBuffer(nbytes=w * h // 2)]
        for o in outs:
            capi.check(L.ffhip_memset(o.ptr, 0, o.nbytes, s), "memset")
        capi.check(L.ffhip_hevc_intra_recon(tus.ctypes.data, dt.ptr, tus.size // 32, dr.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, w, h, w, w // 2, h // 2,
                                            w // 2, 8, 8, s), "ffhip_hevc_intra_recon")
        assert capi.sync(s) == 0
        for k, o in enumerate(outs):
            want = d[f"hevc_{k}"]
            assert np.array_equal(download(o, want.shape, np.int16, s), want), ("plane", k)

    def huff(s):
        files = [d["jpeg"].tobytes()] * 3
        g, _, _ = ops.jpeg_probe(files[0])
        bufs, ptrs, lens = ops.file_args(files)
        n = len(files)
        outs = [ops.DeviceBuffer(nbytes=n * g.y_blocks * 128), ops.DeviceBuffer(nbytes=n * g.c_blocks * 128), ops.DeviceBuffer(nbytes=n * g.c_blocks * 128),
                ops.DeviceBuffer(nbytes=n * 512)]
        status = (C.c_int * n)()
        capi.check(L.ffhip_jpeg_entropy_batch_gpu(ptrs, lens, n, 2, C.byref(g), outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, status, s),
                   "ffhip_jpeg_entropy_batch_gpu")
        assert capi.sync(s) == 0 and list(status) == [0] * n, list(status)
        for o, name in zip(outs, ("huff_y", "huff_u", "huff_v")):
            want = d[name]
            assert np.array_equal(download(o, want.shape, np.int16, s), want), name

    def png(s):
        n = int(d["png_n"])
        files, keys = [d[f"png_file_{i}"].tobytes() for i in range(n)], [d[f"png_key_{i}"] for i in range(n)]
        places = [(4 * k.shape[1], k.shape[0]) for k in keys]
        SF.files_call(lambda ptrs, lens, n_, outs, pitches, status: L.ffhip_png_decode_files_device(ptrs, lens, n_, 2, outs, pitches, None, status, s),
                      files, places, keys)
        assert capi.sync(s) == 0

    def work(name, call):
        try:
            barrier.wait(timeout=60)
            capi.require_device(0)
            s = L.ffhip_stream_create()
            assert s
            call(s)
            L.ffhip_stream_destroy(s)
            line = f"{name} ok"
        except BaseException as e:  # noqa: BLE001 -- the line says it
            line = f"{name} FAILED {e!r}"
            barrier.abort()
        with lock:
            lines.append(line)

    threads = [threading.Thread(target=work, args=(name, call)) for name, call in (("vp8", vp8), ("hevc", hevc), ("huff", huff), ("png", png))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    print("\n".join(sorted(lines)), flush=True)
