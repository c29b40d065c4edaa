"""The stalled-stream scenario of test_stream_order_gpu.py: an entry point is called on a stream that is still busy with large copies, with
its stream-ordered inputs PRODUCED on that stream behind the copies and overwritten again behind the call, and its outputs CONSUMED on that
stream behind the call -- nothing waits anywhere between the first copy and the last enqueue.  What the consumer's copy then holds is the
call's output for the real inputs only if the library ordered every read and write of its own -- side streams, early pre-passes, staging --
as the stream does.

Every stream-ordered input is an Operand: the buffer the library is given (`dev`) holds a DECOY when the call is made -- a valid input of
the same shape and other values -- and the real input arrives by a device-to-device copy that the stall holds back.  A read that runs ahead
of the stream sees the decoy; a read that is still running after the call's place in the stream sees the decoy again (the overwrite).
Every output is an Output: `dev` (0xA5) is what the library writes, `copy` (0xA5) what the consumer copies it to.

All copies are ffhip_copy_calibrate launches: no copy from pageable host memory, which may block the host until the stream reaches it."""
import gc
import time

import numpy as np

from ffpic_amd import capi, ops

FILL = 0xA5
STALL_BYTES = 256 << 20
HOST_SECONDS = {}           # case name -> host time of its enqueue sequence (stall .. overwrite), for the stall-length measurement
OWN = object()              # "the scenario's own stream" where a stream may be given (None is a stream too: the NULL stream)


def pad16(n):
    return (n + 15) & ~15


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _padded(a, fill=0):
    a = as_bytes(a)
    out = np.full(max(pad16(a.size), 16), fill, np.uint8)
    out[:a.size] = a
    return out


def copy(dst, src, nbytes, s):
    """device to device, `nbytes` rounded up to the 16 the buffers here are padded to"""
    capi.check(capi.lib().ffhip_copy_calibrate(dst, src, pad16(nbytes), s), "ffhip_copy_calibrate")


def torch_stream(s):
    import torch
    return torch.cuda.default_stream() if s is None else torch.cuda.ExternalStream(s)


class Stall:
    """the two 256 MiB buffers of the stall; one per module"""

    def __init__(self):
        self.L = capi.require_device()
        self.a, self.b, self.probe = ops.DeviceBuffer(nbytes=STALL_BYTES), ops.DeviceBuffer(nbytes=STALL_BYTES), ops.DeviceBuffer(nbytes=64)
        capi.check(self.L.ffhip_memset(self.a.ptr, 1, STALL_BYTES, None))
        capi.check(self.L.ffhip_stream_sync(None))
        import torch                         # torch's own start-up happens here, not behind a stall: an event on the NULL stream and
        torch.cuda.init()                    # one on a created stream's ExternalStream, as every scenario records them
        s = self.L.ffhip_stream_create()
        assert s
        for ts in (torch.cuda.default_stream(), torch.cuda.ExternalStream(s)):
            e = torch.cuda.Event()
            e.record(ts)
            e.synchronize()
            e.query()
        self.L.ffhip_stream_destroy(s)

    def runs_beside(self, s, other, k=32):
        """Does work on `s` run while `other` is stalled?  Not when the runtime has put the two streams on one hardware queue (a process
        may have more streams than the device gives it queues): work on `s` then starts behind what `other` holds."""
        import torch
        marker = torch.cuda.Event()
        self.enqueue(other, k)
        marker.record(torch_stream(other))
        capi.check(self.L.ffhip_memset(self.probe.ptr, 0, 64, s))
        capi.sync(s)
        beside = not marker.query()
        capi.sync(other)
        return beside

    def enqueue(self, s, k):
        for _ in range(k):
            capi.check(self.L.ffhip_copy_calibrate(self.b.ptr, self.a.ptr, STALL_BYTES, s), "ffhip_copy_calibrate")

    def copy_ms(self, s, reps=16):
        """milliseconds one 256 MiB copy takes on `s` (ffhip_event_elapsed_ms over `reps` of them, after one untimed)"""
        L = self.L
        e0, e1 = L.ffhip_event_create(), L.ffhip_event_create()
        self.enqueue(s, 1)
        capi.check(L.ffhip_event_record(e0, s))
        self.enqueue(s, reps)
        capi.check(L.ffhip_event_record(e1, s))
        ms = L.ffhip_event_elapsed_ms(e0, e1)
        L.ffhip_event_destroy(e0)
        L.ffhip_event_destroy(e1)
        assert ms > 0
        return ms / reps


class Operand:
    """A stream-ordered input.  dev: what the library reads (the decoy until the producer's copy has run); true: the real input;
    decoy: the decoy a second time, for the overwrite behind the call."""

    def __init__(self, true, decoy):
        t, d = as_bytes(true), as_bytes(decoy)
        assert t.size == d.size and t.size and not np.array_equal(t, d), "a decoy has the input's shape and other values"
        self.nbytes = t.size
        self.h_true, self.h_decoy = _padded(t), _padded(d)
        self.dev, self.true, self.decoy = ops.DeviceBuffer(host=self.h_decoy), ops.DeviceBuffer(host=self.h_true), ops.DeviceBuffer(host=self.h_decoy)

    @property
    def ptr(self):
        return self.dev.ptr

    def reset(self):
        """the decoy back into dev, by a blocking copy (after the warm-up of an entry that writes its input in place)"""
        L = capi.lib()
        capi.check(L.ffhip_memcpy_h2d(self.dev.ptr, self.h_decoy.ctypes.data, self.h_decoy.nbytes, None))
        capi.check(L.ffhip_stream_sync(None))


class Output:
    """An output of `nbytes`.  dev: what the library writes, copy: where the consumer copies it; both 0xA5.  of=<Operand>: the entry writes
    that operand in place, and the consumer copies from there."""

    def __init__(self, nbytes, of=None):
        self.nbytes, self.of = nbytes, of
        self.fill = np.full(max(pad16(nbytes), 16), FILL, np.uint8)
        self.dev = of.dev if of is not None else ops.DeviceBuffer(host=self.fill)
        self.copy = ops.DeviceBuffer(host=self.fill)

    @property
    def ptr(self):
        return self.dev.ptr

    def refill(self, s=None):
        """0xA5 back into the buffers, by a blocking copy on `s` (the NULL stream unless a thread with a stream of its own gives that)"""
        L = capi.lib()
        for b in ([self.copy] if self.of is not None else [self.dev, self.copy]):
            capi.check(L.ffhip_memcpy_h2d(b.ptr, self.fill.ctypes.data, self.fill.nbytes, s))
        capi.check(L.ffhip_stream_sync(s))

    def copied(self):
        return self.copy.to_host((self.nbytes,), np.uint8)

    def written(self):
        return self.dev.to_host((self.nbytes,), np.uint8)


class Scenario:
    """One stalled stream, as a context: entering it enqueues the stall and the marker; produce / consume / overwrite enqueue the copies;
    still_stalled() is the pending assertion; finish() synchronises.  Nothing between the entry and finish() waits for the device.  The
    collector is off inside the context (a buffer it freed behind the stall would wait for the device) and on again however it is left."""

    def __init__(self, name, stall, s, k):
        self.name, self.stall, self.s, self.k = name, stall, s, k
        self.L = capi.lib()

    def __enter__(self):
        import torch
        self.marker, ts = torch.cuda.Event(), torch_stream(self.s)
        gc.collect()
        gc.disable()
        try:
            self.t0 = time.perf_counter()
            self.stall.enqueue(self.s, self.k)
            self.marker.record(ts)
        except BaseException:
            gc.enable()
            raise
        return self

    def __exit__(self, *exc):
        gc.enable()
        return False

    def _stream(self, s):
        return self.s if s is OWN else s

    def produce(self, operands=(), memsets=(), s=OWN):
        s = self._stream(s)
        for op in operands:
            copy(op.dev.ptr, op.true.ptr, op.nbytes, s)
        for ptr, value, nbytes in memsets:
            capi.check(self.L.ffhip_memset(ptr, value, nbytes, s), "ffhip_memset")

    def consume(self, outputs, s=OWN):
        s = self._stream(s)
        for o in outputs:
            copy(o.copy.ptr, o.dev.ptr, o.nbytes, s)

    def overwrite(self, operands, s=OWN):
        s = self._stream(s)
        for op in operands:
            copy(op.dev.ptr, op.decoy.ptr, op.nbytes, s)

    def still_stalled(self):
        """right behind the last enqueue: the stall in front of everything has not finished, so nothing enqueued behind it has run"""
        pending, t1 = not self.marker.query(), time.perf_counter()
        HOST_SECONDS[self.name] = max(HOST_SECONDS.get(self.name, 0.0), t1 - self.t0)
        assert pending, f"{self.name}: inconclusive -- the stall ({self.k} copies) had finished before the last enqueue returned"

    def finish(self):
        return capi.sync(self.s)


def warm_up(s, call, operands=(), outputs=(), memsets=()):
    """the call once on the idle stream with the decoy (scratch grows here, not under the stall: growing synchronises), then everything
    back to its state before"""
    L = capi.lib()
    for ptr, value, nbytes in memsets:
        capi.check(L.ffhip_memset(ptr, value, nbytes, s), "ffhip_memset")
    call(s)
    capi.sync(s)
    for o in outputs:
        o.refill()
    for op in operands:
        op.reset()


def run(name, stall, s, k, call, operands=(), outputs=(), memsets=(), overwrite=True):
    """The scenario for one call: warm-up, stall, marker, producer, call, consumer, overwrite, pending assertion, sync -> the sync's status"""
    warm_up(s, call, operands, outputs, memsets)
    with Scenario(name, stall, s, k) as sc:
        sc.produce(operands, memsets)
        call(s)
        sc.consume(outputs)
        if overwrite:
            sc.overwrite(operands)
        sc.still_stalled()
    return sc.finish()


def run_broken(name, stall, s, other, k, call, operands=(), outputs=(), memsets=()):
    """The negative control: the CALLER breaks the contract.  The call and its consumer go on `s`, which has no stall; the producer goes
    on `other`, behind that stream's own stall.  The call then reads the decoy, and its output is the decoy's -- provided the stall
    outlasts the call, which the marker shows: it is still pending when `s` has drained."""
    warm_up(s, call, operands, outputs, memsets)
    with Scenario(name + "/broken", stall, other, k) as sc:
        sc.produce(operands)
        sc.produce((), memsets, s=s)
        call(s)
        sc.consume(outputs, s=s)
        rc = capi.sync(s)
        sc.still_stalled()
        sc.overwrite(operands)
    capi.sync(other)
    return rc
