"""No GPU: the schedule of test_concurrent_gpu.py lets every pair of families meet, and the crew of caller threads holds the two placement
rules of tests/concurrency.py -- shown with a stand-in for the library that records which thread did what."""
import threading

import pytest

import concurrency as K


def test_every_pair_of_families_shares_a_round():
    rounds = K.schedule(K.FAMILIES)
    assert all(len(r) == K.THREADS and set(r) <= set(K.FAMILIES) for r in rounds)
    want = K.pairs_of(K.FAMILIES)
    n = len(K.FAMILIES)
    assert len(want) == n * (n + 1) // 2 and all((f, f) in want for f in K.FAMILIES)
    met = set().union(*[K.pairs_in(r) for r in rounds])
    assert met == want, sorted(want - met)
    assert all(r.count(f) >= 2 for f in K.FAMILIES for r in rounds if (f, f) in K.pairs_in(r))     # a family meets itself on two threads
    assert rounds == K.schedule(list(K.FAMILIES))                                                    # deterministic
    assert len(rounds) >= -(-len(want) // 6) and len(rounds) <= len(want) // 4                       # four places hold six pairs at the most


@pytest.mark.parametrize("threads,n", [(2, 3), (3, 5), (4, 1), (4, 7)])
def test_the_schedule_for_other_sizes(threads, n):
    fams = [f"f{i}" for i in range(n)]
    rounds = K.schedule(fams, threads)
    assert set().union(*[K.pairs_in(r) for r in rounds]) == K.pairs_of(fams)
    again = K.schedule(fams, threads, need={("f0", "f0")})
    assert len(again) == 1 and again[0].count("f0") >= 2


class Recorder:
    """stands in for the library: notes the calls and the thread that made them"""

    def __init__(self):
        self.lock, self.log, self.next = threading.Lock(), [], 100

    def note(self, what, arg=None):
        with self.lock:
            self.log.append((threading.get_ident(), what, arg))

    def require_device(self, device):
        self.note("require_device", device)

    def stream_create(self):
        with self.lock:
            self.next += 1
            s = self.next
        self.note("stream_create", s)
        return s

    def stream_destroy(self, s):
        self.note("stream_destroy", s)


def test_a_thread_binds_the_device_makes_its_stream_and_every_runner_gets_that_stream():
    rec = Recorder()
    with K.Crew(4, api=rec) as crew:
        boxes = crew.boxes
        assert all(b.handle for b in boxes) and len({b.handle for b in boxes}) == 4      # a stream each, none the NULL stream

        def runner(t, name):
            def run():
                rec.note("run", (t, name, boxes[t].handle))
                return name
            return run
        for rnd in K.schedule(["a", "b", "c"], 4):
            got = crew.round([[runner(t, f), runner(t, f + "'")] for t, f in enumerate(rnd)], reps=2, labels=rnd)
            for t, (start, end, names) in enumerate(got):
                assert start <= end and names == [rnd[t], rnd[t] + "'"] * 2
    by_thread = {}
    for ident, what, arg in rec.log:
        by_thread.setdefault(ident, []).append((what, arg))
    assert len(by_thread) == 4 and threading.get_ident() not in by_thread
    streams = set()
    for calls in by_thread.values():
        assert calls[0] == ("require_device", 0) and calls[1][0] == "stream_create" and calls[-1] == ("stream_destroy", calls[1][1])
        s = calls[1][1]
        runs = [arg for what, arg in calls[2:-1]]
        assert runs and all(what == "run" for what, _ in calls[2:-1])
        assert {r[2] for r in runs} == {s} and len({r[0] for r in runs}) == 1            # its runners, on its stream
        streams.add(s)
    assert len(streams) == 4 and all(b.handle is None for b in boxes)


def test_an_error_in_a_thread_is_raised_on_the_main_thread_and_nothing_waits():
    rec = Recorder()

    def bad():
        raise ValueError("wrong bytes")
    with pytest.raises(AssertionError, match="wrong bytes"):
        with K.Crew(3, api=rec, wait=20) as crew:
            crew.round([[lambda: 0], [bad], [lambda: 0]], labels=["x", "y", "z"])
    assert sum(1 for _, what, _ in rec.log if what == "stream_destroy") == 3


def test_overlap_is_an_intersection_of_intervals():
    assert K.overlap((0.0, 2.0), (1.0, 3.0)) and K.overlap((1.0, 3.0), (0.0, 2.0)) and K.overlap((0.0, 5.0), (1.0, 2.0))
    assert not K.overlap((0.0, 1.0), (1.5, 2.0)) and not K.overlap((1.5, 2.0), (0.0, 1.0))
