"""GPU: calls of several host threads, a stream each, in flight together (include/ffpic_hip.h, "Threads and streams").

a. every pair of families of entry points meets on two threads, by the schedule of tests/concurrency.py, under both front-end configurations;
b. the kernels whose waves wait for each other run beside each other at the sizes of test_handoff_stress_gpu.py;
c. the entries without a stream argument -- ffhip_jpeg_recon_batch_host and the block operations, which the library serialises itself, and
   ffhip_jpeg_decode_files, whose two slots each calling thread keeps for itself -- are called by four threads at once, each with data of
   its own; and threads that end give their slots back with their streams;
d. the first calls of a process are made by four threads at once (a child process);
e. the per-thread diagnostic records hold the calling thread's call while the other threads make theirs.
Every comparison is exact, against answer keys made on the main thread before a thread starts; no switch changes while threads run; the
give-up hooks are not used; GPU_MAX_HW_QUEUES is whatever the machine sets."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import concurrency as K
import oracle_lib as O
import scratch_fill as SF
import test_scratch_fill_gpu as F
from ffpic_amd import capi, ops, synth
from test_vp8_lf_gpu import oracle_lf

pytestmark = pytest.mark.gpu
REPS = 3
RETRIED = capi.FFHIP_RETRIED
RETRY_FAMILIES = ("vp8_side_by_side", "vp8_frames")
SWITCHES = F.SWITCHES + ("FFHIP_WEBP_PART_MB",)
CONFIGS = {         # the front ends of the file calls and the form of ffhip_vp8_decode_frames: set before the threads start, never while they run
    "device_front_ends": {"FFHIP_JPEG_GPU_ENTROPY": None, "FFHIP_WEBP_GPU_ENTROPY": 1, "FFHIP_JPEG_PROGRESSIVE_GPU": 1, "FFHIP_VP8_FRAMES": "fused"},
    "host_threads": {"FFHIP_JPEG_GPU_ENTROPY": 0, "FFHIP_WEBP_GPU_ENTROPY": 0, "FFHIP_JPEG_PROGRESSIVE_GPU": None, "FFHIP_VP8_FRAMES": "rows"},
}


@pytest.fixture(autouse=True)
def _switches_back():
    capi.require_device(0)
    yield
    for name in SWITCHES:
        capi.setenv(name, None)


@pytest.fixture(scope="module")
def main_stream():
    L = capi.require_device(0)
    s = L.ffhip_stream_create()
    assert s
    yield s
    L.ffhip_stream_destroy(s)


@pytest.fixture(scope="module")
def built(main_stream):
    """-> (boxes, [the families of thread t]): made, and run once, on the main thread"""
    t0 = time.perf_counter()
    shared = K.Shared()
    boxes = [SF.StreamBox() for _ in range(K.THREADS)]
    fams = [K.build_families(t, boxes[t], shared) for t in range(K.THREADS)]
    t1 = time.perf_counter()
    for t in range(K.THREADS):
        for form in ("fused", "rows"):
            capi.setenv("FFHIP_VP8_FRAMES", form)
            K.prime({"vp8_frames": fams[t]["vp8_frames"][form]} if form == "rows" else K.for_form(fams[t], form), boxes[t], main_stream)
    capi.setenv("FFHIP_VP8_FRAMES", None)
    print(f"\nconcurrent: families built in {t1 - t0:.2f} s, run once alone in {time.perf_counter() - t1:.2f} s")
    return boxes, fams


# ---------------------------------------------------------------------------------------------------- a. every pair of families meets
@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_pair_of_families_meets_on_two_threads(built, config):
    """Four threads, a barrier per round, tests/concurrency.schedule: in its round a thread runs its family's runners REPS times.  A pair has
    MET when the two threads' intervals -- first call to last sync -- intersect; pairs that did not are scheduled again, up to twice the
    schedule's length in all, and then none may be left.  A side-by-side VP8 call (and the row form of ffhip_vp8_decode_frames) that the sync
    repeated is a correct outcome and is counted; every other status but 0 fails."""
    boxes, built_fams = built
    for name, value in CONFIGS[config].items():
        capi.setenv(name, value)
    fams = [K.for_form(f, CONFIGS[config]["FFHIP_VP8_FRAMES"]) for f in built_fams]
    rounds = K.schedule(K.FAMILIES)
    unmet, first_pass, retried, done = K.pairs_of(K.FAMILIES), None, 0, 0
    t0 = time.perf_counter()
    with K.timed_syncs(), K.Crew(K.THREADS, boxes=boxes) as crew:
        todo = rounds
        while todo and done < 2 * len(rounds):
            for rnd in todo[:2 * len(rounds) - done]:
                res = crew.round([fams[t][f] for t, f in enumerate(rnd)], REPS, labels=rnd)
                done += 1
                for f, (_, _, got) in zip(rnd, res):
                    retried += sum(1 for rc in got if rc == RETRIED)
                    assert all(rc in (0, None) or (rc == RETRIED and f in RETRY_FAMILIES) for rc in got), (f, got)
                for (i, a), (j, b) in itertools.combinations(enumerate(rnd), 2):
                    if K.overlap(res[i], res[j]):
                        unmet.discard(K.pair(a, b))
            if first_pass is None:
                first_pass = len(unmet)
            todo = K.schedule(K.FAMILIES, need=unmet) if unmet else []
    n = len(K.pairs_of(K.FAMILIES))
    print(f"\nconcurrent {config}: {len(K.FAMILIES)} families, {n} pairs, {len(rounds)} rounds scheduled, {done} run x {REPS} reps in "
          f"{time.perf_counter() - t0:.2f} s; {n - first_pass} of {n} pairs met on the first pass; FFHIP_RETRIED {retried} times")
    assert not unmet, f"pairs whose calls never overlapped in {done} rounds: {sorted(unmet)}"


# ---------------------------------------------------------------------------------------------------- b. kernels that wait for each other
def upload(a):
    return ops.DeviceBuffer(host=np.ascontiguousarray(a))


def read(buf, shape, dtype, s):
    out = np.empty(shape, dtype)
    capi.check(capi.lib().ffhip_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, s), "ffhip_memcpy_d2h")
    assert capi.sync(s) == 0
    return out


def hevc_handoff_runner(t, box):
    """ffhip_hevc_intra_recon, 512 x 384 with adversarial masks (test_handoff_stress_gpu.py), a list per thread"""
    L = capi.lib()
    w, h = 512, 384
    tus, res = synth.hevc_intra_tus(w, h, 77 + t, adversarial_masks=True)
    tus = np.ascontiguousarray(tus)
    want = O.oracle_hevc_intra(tus, res, w, h, True, 8, 8)
    dt, dr = upload(tus.view(np.uint8)), upload(res)
    outs = [ops.DeviceBuffer(nbytes=w * h * 2), ops.DeviceBuffer(nbytes=w * h // 2), ops.DeviceBuffer(nbytes=w * h // 2)]

    def run():
        s = SF.h(box)
        for o in outs:
            capi.check(L.ffhip_memset(o.ptr, 0, o.nbytes, s), "ffhip_memset")
        capi.check(L.ffhip_hevc_intra_recon(tus.ctypes.data, dt.ptr, len(tus), dr.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, w, h, w, w // 2, h // 2, w // 2,
                                            8, 8, s), "ffhip_hevc_intra_recon")
        rc = capi.sync(s)                                               # (FFHIP_EIO raises: a bounded wait that ran out)
        assert rc == 0, ("hevc", t, rc)
        for o, e, name in zip(outs, want, "YUV"):
            assert np.array_equal(read(o, e.shape, np.int16, s), e), ("hevc", t, name)
        return rc
    return run


def vp8_handoff_runner(t, box):
    """120 x 68 macroblocks x 3 frames: ffhip_vp8_predict_recon, ffhip_vp8_loopfilter on its planes, and the side-by-side call; frames per thread"""
    L = capi.lib()
    c, r, n = 120, 68, 3
    n_mb = c * r
    modes = np.ascontiguousarray(np.stack([synth.vp8_modes(c, r, seed=900 + 10 * t + i) for i in range(n)]))
    modes[..., 18] = np.random.default_rng(9 + t).integers(0, 4, size=modes[..., 18].shape)
    resid = np.ascontiguousarray(np.stack([synth.vp8_residual(n_mb, seed=900 + 10 * t + i, amplitude=60) for i in range(n)]))
    flt = np.ascontiguousarray(synth.vp8_filters(seed=3 + t))
    pred = [O.oracle_vp8_frame(c, r, modes[i], resid[i]) for i in range(n)]
    filt = [oracle_lf(c, r, 2, modes[i], flt, pred[i]) for i in range(n)]
    want_pred, want_filt = [np.stack([p[k] for p in pred]) for k in range(3)], [np.stack([p[k] for p in filt]) for k in range(3)]
    dm, dr, df = upload(modes), upload(resid), upload(flt)
    ysz, csz = 256 * n_mb, 64 * n_mb
    a = [ops.DeviceBuffer(nbytes=n * ysz), ops.DeviceBuffer(nbytes=n * csz), ops.DeviceBuffer(nbytes=n * csz)]
    b = [ops.DeviceBuffer(nbytes=n * ysz), ops.DeviceBuffer(nbytes=n * csz), ops.DeviceBuffer(nbytes=n * csz)]

    def same(planes, want, s, what):
        for o, e, name in zip(planes, want, "YUV"):
            assert np.array_equal(read(o, e.shape, np.uint8, s), e), ("vp8", t, what, name)

    def run():
        s = SF.h(box)
        for o in a + b:
            capi.check(L.ffhip_memset(o.ptr, 0, o.nbytes, s), "ffhip_memset")
        capi.check(L.ffhip_vp8_predict_recon(c, r, n, modes.ctypes.data, dm.ptr, dr.ptr, n_mb * 384, None, a[0].ptr, a[1].ptr, a[2].ptr, ysz, csz, s),
                   "ffhip_vp8_predict_recon")
        assert capi.sync(s) == 0
        same(a, want_pred, s, "prediction")
        capi.check(L.ffhip_vp8_loopfilter(c, r, n, 2, dm.ptr, df.ptr, a[0].ptr, a[1].ptr, a[2].ptr, ysz, csz, s), "ffhip_vp8_loopfilter")
        assert capi.sync(s) == 0
        same(a, want_filt, s, "loop filter")
        capi.check(L.ffhip_vp8_predict_loopfilter(c, r, n, modes.ctypes.data, dm.ptr, dr.ptr, n_mb * 384, None, 2, df.ptr, b[0].ptr, b[1].ptr, b[2].ptr, ysz, csz,
                                                  s), "ffhip_vp8_predict_loopfilter")
        rc = capi.sync(s)                                               # 0, or FFHIP_RETRIED: the header allows the repeat for this call alone
        assert rc in (0, RETRIED), ("vp8", t, rc)
        same(b, want_filt, s, "side by side")
        return rc
    return run


HANDOFF_ROUNDS = {2: ("HH", "VV", "HV", "VH", "HV"), 4: ("HHVV", "VVHH", "HVHV", "VHVH", "HVVH")}


@pytest.fixture(scope="module")
def handoff(main_stream):
    boxes = [SF.StreamBox() for _ in range(4)]
    runners = [{"H": hevc_handoff_runner(t, boxes[t]), "V": vp8_handoff_runner(t, boxes[t])} for t in range(4)]
    for t in range(4):
        K.prime({k: [run] for k, run in runners[t].items()}, boxes[t], main_stream)
    return boxes, runners


@pytest.mark.parametrize("threads", [2, 4])
def test_kernels_that_wait_for_each_other_run_beside_each_other(handoff, threads):
    """Two threads, then four; five rounds behind a barrier each, the families rotated so that HEVC meets HEVC, VP8 meets VP8 and HEVC meets
    VP8.  Every byte is the oracle's; a sync gives 0, or FFHIP_RETRIED for the side-by-side call.  Nothing is tried again: every wait in these
    kernels is bounded, so a schedule that starves one of them ends in FFHIP_EIO, which fails here."""
    boxes, runners = handoff
    retried, t0 = 0, time.perf_counter()
    with K.Crew(threads, boxes=boxes[:threads]) as crew:
        for rnd in HANDOFF_ROUNDS[threads]:
            res = crew.round([[runners[t][f]] for t, f in enumerate(rnd)], labels=list(rnd))
            retried += sum(1 for _, _, got in res for rc in got if rc == RETRIED)
    print(f"\nconcurrent hand-offs, {threads} threads: {time.perf_counter() - t0:.2f} s; FFHIP_RETRIED {retried} times")


# ---------------------------------------------------------------------------------------------------- c. entries that serialise themselves
def test_host_entry_and_file_pipeline_from_four_threads():
    """ffhip_jpeg_recon_batch_host (one lock around the call) and ffhip_jpeg_decode_files (each thread on two slots of its own, no lock), four
    threads at once, planes and files of each thread's own: the oracle's pictures"""
    q = synth.quant_tables()
    jobs = []
    for t in range(4):
        small, _, _ = F.uniform_file_sets(40 + t)
        files = F.uniform_runner(small, None, True, 2, n_threads=K.N_THREADS)
        hosts = []
        for mc, mr, n, h, v in ((13, 7, 3, 2, 2), (5, 4, 2, 2, 2), (3, 2, 2, 1, 1)):
            planes = synth.coef_batch(n, mc, mr, 3, h, v, first=3 + 16 * t)
            want = O.oracle_jpeg_recon(O.make_geom(mc, mr, 3, h, v), *planes, q, n_images=n)

            def host(mc=mc, mr=mr, n=n, h=h, v=v, planes=planes, want=want, t=t):
                got = ops.jpeg_recon_batch_host(capi.jpeg_geom(mc, mr, 3, h, v), n, *planes, q)
                assert np.array_equal(np.asarray(got).reshape(want.shape), want), ("jpeg_recon_batch_host", t, mc, mr)
            hosts.append(host)
        jobs.append(hosts + [files])
    for job in jobs:                                                    # alone first
        for run in job:
            run()
    with K.Crew(4) as crew:
        for _ in range(3):
            crew.round(jobs, reps=4, labels=["host entry + files"] * 4)


def test_file_pipeline_slots_end_with_their_thread():
    """Six threads, one after another: each makes one ffhip_jpeg_decode_files call (two pictures a chunk; the device front end on the even
    threads, host threads on the odd ones) and one ffhip_jpeg_decode_files_device call on the host path, and ends -- its slot streams are
    destroyed, and what the library kept under them goes with them.  A slot stream made next may get a handle of theirs and must start
    from nothing: two fresh threads in turn find nothing to fill before their first call and, behind a one-picture call, their own
    slots' two kinds at the same byte counts and nothing an ended thread kept; the main thread then makes its own calls, sets every byte
    the library keeps for it to 0x5A, and makes them again.  Every picture is the answer key's, with the 0xA5 around it intact."""
    import threading
    capi.require_device(0)
    small, larger, _ = F.uniform_file_sets(50)
    files, device = F.uniform_runner(small, None, True, 2), F.uniform_runner(small, None)
    errors = []

    def work(t):
        try:
            capi.setenv("FFHIP_JPEG_GPU_ENTROPY", "0" if t & 1 else None)      # (no other thread runs meanwhile)
            files()
            capi.setenv("FFHIP_JPEG_GPU_ENTROPY", "0")
            device()
        except BaseException as e:  # noqa: BLE001 -- reported below, on the main thread
            errors.append((t, e))

    for t in range(6):
        th = threading.Thread(target=work, args=(t,))
        th.start()
        th.join()
        assert not errors, errors

    # no entry of an ended thread's is left for a later thread to find: a fresh thread with a fresh stream has nothing to fill before its
    # first call; behind one host-threads call of ONE picture a fill finds its slots' two kinds and nothing else -- not the device front
    # end's kinds the even threads kept under their slot streams, not their two-picture capacities -- twice over, the same bytes
    one, seen = F.uniform_runner(small[:1], None, True, 1), []

    def fresh(t):
        try:
            L = capi.require_device(0)
            s = L.ffhip_stream_create()
            assert s
            before = SF.fill(s, 0x5A)
            assert before == (0, 0, []), before
            capi.setenv("FFHIP_JPEG_GPU_ENTROPY", "0")
            one()
            dev, host, kinds = SF.fill(s, 0x5A)
            assert dev > 0 and host > 0 and {SF.base_of(k) for k in kinds} == {"SCRATCH_FILES_PLANES", "SCRATCH_FILES_PIXELS"}, (dev, host, kinds)
            seen.append((dev, host, kinds))
            one()
            L.ffhip_stream_destroy(s)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, e))

    for t in (6, 7):
        th = threading.Thread(target=fresh, args=(t,))
        th.start()
        th.join()
        assert not errors, errors
    assert seen[0] == seen[1], seen
    own = [F.uniform_runner(larger, None, True, 2), files, device]
    for entropy in (None, "0"):
        capi.setenv("FFHIP_JPEG_GPU_ENTROPY", entropy)
        for run in own:
            run()
        dev, host, kinds = SF.fill(None, 0x5A)
        assert dev > 0 and host > 0 and {"SCRATCH_FILES_PLANES", "SCRATCH_FILES_PIXELS"} <= {SF.base_of(k) for k in kinds}, (dev, host, kinds)
        for run in own:
            run()


def test_block_operations_from_four_threads():
    """200 calls of every block operation per thread -- idct_8x8 and idct_4x4 through ffhip_accl_ops_get() and through ffhip_get_dct_ops(16),
    YUV_to_BGRA32 of ffhip_get_cs_ops(16) at seven (v, h), ffhip_idct_4x4_hevc -- all at once, every block distinct and compared with the
    oracle's answer for it.  They share one staging buffer on the device; ffhip_blockops.hip holds one lock from a call's first copy to
    its last.  (Without it: A's copy in, B's copy in, A's kernel, B's kernel, A's copy out -- A gets B's block transformed twice.)"""
    capi.require_device(0)
    jobs = [[K.block_calls(t, 200)] for t in range(4)]
    for job in jobs:
        job[0]()
    with K.Crew(4) as crew:
        crew.round(jobs, labels=["block operations"] * 4)


# ---------------------------------------------------------------------------------------------------- d. first use
def test_first_use_from_four_threads_at_once(tmp_path):
    path = str(tmp_path / "first_use.npz")
    K.first_use_inputs(path)
    tests = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{tests!r}, {os.path.dirname(tests)!r}]; import concurrency; concurrency.first_use_child({path!r})"
    done = subprocess.run([sys.executable, "-c", code], timeout=120, capture_output=True, text=True)
    lines = [line for line in done.stdout.splitlines() if line.strip()]
    assert done.returncode == 0 and lines == ["hevc ok", "huff ok", "png ok", "vp8 ok"], (done.returncode, lines, done.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------- e. per-thread records
def record_jobs(t, box, shared):
    """[(name, run, read)] of thread t: calls whose diagnostic record is the batch's own -- file counts, shares and lists differ by thread --
    and the reader of that record"""
    L = capi.lib()
    nt = K.N_THREADS
    alpha = capi.FFHIP_WEBP_PIXELS_LIBWEBP | capi.FFHIP_WEBP_ALPHA
    sh = shared
    n_png, n_v8l, n_alpha, n_webp = 5 + 3 * t, 4 + 2 * t, 3 + 2 * t, 2 + t

    def cut(files, keys, n):
        return files[:n], keys[:n]
    png, v8l, alp = cut(sh.png_files, sh.png_keys, n_png), cut(sh.vp8l_files, sh.vp8l_keys, n_v8l), cut(sh.alpha_files, sh.alpha_keys, n_alpha)
    good = [(f, k) for f, k in zip(sh.ref_files, sh.ref_keys) if k is not None]
    webp = [f for f, _ in good[t:t + n_webp]], [k for _, k in good[t:t + n_webp]]
    prog = sh.progressive[t:t + 2 + t]
    batch = F.jpeg_batch_files(60 + t)
    few = ([k for k in batch[0] if k is not None][:2 + t],)
    few = (few[0], [k.data for k in few[0]], -1)
    plain_tensors, _, oriented = F.jpeg_tensor_runs(few, box, nt)
    w, h = ((192, 128), (256, 128), (128, 128), (256, 192))[t]          # another count of scheduling windows, and so of groups, per thread
    intra = F.plain(K.named(F.TSO.hevc_intra_case(w, h, 90 + t), f"{t} records"), box)

    def plan():
        out = (C.c_uint32 * 8)()
        capi.check(L.ffhip_debug_hevc_plan_result(out), "ffhip_debug_hevc_plan_result")
        return tuple(out)
    return [
        ("png", F.lossless_runner("ffhip_png_decode_files_device", *png, F.sizes_of(png[1]), box, n_threads=nt), ops.png_last),
        ("vp8l", F.lossless_runner("ffhip_vp8l_decode_files_device", *v8l, F.sizes_of(v8l[1]), box, n_threads=nt), ops.vp8l_last),
        ("webp alpha", F.webp_runner(*alp, box, alpha, n_threads=nt), ops.webp_alpha_last),
        ("webp parts", F.webp_runner(*webp, box, 0, n_threads=nt), ops.webp_last_parts),
        ("tensor parts", plain_tensors, ops.tensor_last_parts),
        ("orient items", oriented, ops.orient_last_items),
        ("progressive", F.mixed_runner(prog, [k.data for k in prog], box, flags=capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE, n_threads=nt), ops.progressive_last),
        ("hevc plan", intra, plan),
    ]


def test_per_thread_records_stay_per_thread(main_stream):
    """Right behind its own call each thread reads the record of it -- ffhip_debug_webp_last_parts, _tensor_last_parts, _orient_last_items,
    _png_last, _vp8l_last, _webp_alpha_last, _progressive_last, _hevc_plan_result -- while the other three make their calls, and finds what the
    same call leaves when it runs alone (taken on the main thread first).  The part budgets make every file a part of its own, so the records
    count the batch, and the batches differ by thread: for every record at least three threads must differ, or this test would show nothing."""
    for name in ("FFHIP_PNG_PART_BYTES", "FFHIP_VP8L_PART_BYTES", "FFHIP_WEBP_ALPHA_PART_BYTES", "FFHIP_TENSOR_PART_BYTES", "FFHIP_WEBP_PART_MB",
                 "FFHIP_WEBP_GPU_ENTROPY", "FFHIP_JPEG_PROGRESSIVE_GPU"):
        capi.setenv(name, 1)
    shared = K.Shared()
    boxes = [SF.StreamBox() for _ in range(4)]
    jobs = [record_jobs(t, boxes[t], shared) for t in range(4)]
    alone = []
    for t in range(4):
        boxes[t].handle = main_stream
        alone.append({})
        for name, run, rd in jobs[t]:
            if hasattr(run, "prime"):
                run.prime()
            run()
            alone[t][name] = rd()
        boxes[t].handle = None
    for name, _, _ in jobs[0]:
        assert len({alone[t][name] for t in range(4)}) >= 3, (name, [alone[t][name] for t in range(4)])

    def checked(t, k):
        name, run, rd = jobs[t][k]

        def go():
            run()
            got = rd()
            assert got == alone[t][name], (name, t, got, alone[t][name])
        return go
    n = len(jobs[0])
    with K.Crew(4, boxes=boxes) as crew:
        for rnd in range(3):
            crew.round([[checked(t, (k + 2 * t + rnd) % n) for k in range(n)] for t in range(4)], labels=["records"] * 4)
