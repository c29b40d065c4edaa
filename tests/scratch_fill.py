"""What test_scratch_fill_gpu.py shares: the hook that overwrites what the library keeps between calls (ffhip_debug_scratch_fill), the
protocol every family of entry points is put through, the record of which scratch kinds a fill reported in front of a checked run, and
sentinel-framed outputs for the file calls.

The protocol (run_protocol): the family's larger cases, so that its scratch is as big as it gets; fill(0xFF); the small cases; fill(0x5A);
the small cases; fill(0x00); the small cases; fill(0xFF); the larger cases again.  A case is a callable that runs the entry and asserts its
output against an answer key that does not come from the library, with the 0xA5 around the output untouched.  0xFF is what today's zeroed
fresh allocations hide, 0x5A a second value (a dependence also shows as a difference between runs), 0x00 today's situation."""
import ctypes as C
import os
import re

import numpy as np

from ffpic_amd import capi, ops

FILL = 0xA5
VALUES = (0xFF, 0x5A, 0x00)
INTERNAL_H = os.path.join(capi.CSRC, "ffhip_internal.h")

COVERED = {}            # scratch kind -> the families whose fill reported it in front of a checked run


class StreamBox:
    """a stream that is made later: a runner built on one thread for a stream that the thread that runs it creates (tests/concurrency.py)"""
    handle = None


def h(s):
    """the stream handle a runner was given: itself, or what its StreamBox holds by now"""
    return s.handle if isinstance(s, StreamBox) else s


def lib():
    L = capi.require_device(0)
    L.ffhip_scratch.argtypes = [C.c_int, C.c_void_p, C.c_size_t]          # exported, not public: ffhip_internal.h
    L.ffhip_scratch.restype = C.c_void_p
    return L


def fill(stream, value):
    """ffhip_debug_scratch_fill on (current device, stream) -> (device bytes, host bytes, [kinds that had a buffer])"""
    nbytes, kinds = (C.c_uint64 * 2)(), (C.c_int * 256)()
    n = lib().ffhip_debug_scratch_fill(stream, value, nbytes, kinds, 256)
    assert 0 <= n <= 256, n
    return int(nbytes[0]), int(nbytes[1]), list(kinds[:n])


def scratch_head(kind, stream, n=64):
    """the first n bytes of the device scratch of (kind, stream), through the library's own accessor: one word is asked for, which never
    grows a buffer that exists"""
    L = lib()
    p = L.ffhip_scratch(kind, stream, 1)
    assert p
    out = np.zeros(n, np.uint8)
    capi.check(L.ffhip_memcpy_d2h(out.ctypes.data, p, n, stream), "ffhip_memcpy_d2h")
    capi.sync(stream)
    return out


def enum_kinds():
    """enum FfhipScratchKind of ffhip_internal.h -> {name: (base, sub-slots behind it)}; ".. + n" in an entry's comment is its range"""
    text = open(INTERNAL_H).read()
    parts = int(re.search(r"#define FFHIP_HUFF_PARTS (\d+)", text).group(1))
    body = re.search(r"enum FfhipScratchKind \{(.*?)\n\};", text, re.S).group(1)
    out = {}
    for line in body.split("\n"):
        m = re.match(r"\s*(SCRATCH_\w+) = (\d+),(.*)", line)
        if not m:
            continue
        span = re.search(r"/\* \.\. \+ ([^:*]+)", m.group(3))                       # "1", "FFHIP_HUFF_PARTS - 1", up to ':' or the comment's end
        extra = eval(span.group(1).strip(), {"__builtins__": {}}, {"FFHIP_HUFF_PARTS": parts}) if span else 0
        out[m.group(1)] = (int(m.group(2)), int(extra))
    assert len(out) >= 25 and len({b for b, _ in out.values()}) == len(out), out
    return out


def base_of(kind, table=None):
    """the enum entry a kind belongs to (a sub-slot belongs to the nearest base at or below it whose range reaches it), None: to none"""
    table = table or enum_kinds()
    best = None
    for name, (base, extra) in table.items():
        if base <= kind <= base + extra and (best is None or base > table[best][0]):
            best = name
    return best


def run_protocol(family, stream, larger, small, kinds=()):
    """The protocol of the module docstring.  `larger`, `small`: lists of callables; kinds: names of enum entries the family's scratch must show
    up under in the first fill.  Every kind a fill reports in front of a checked run goes into COVERED."""
    table = enum_kinds()

    def filled(value, must=()):
        capi.sync(stream)
        dev, host, got = fill(stream, value)
        assert dev + host > 0, (family, value)
        names = {base_of(k, table) for k in got}
        assert None not in names, (family, got)
        missing = [k for k in must if k not in names]
        assert not missing, (family, missing, sorted(names))
        return got

    def checked(cases, got):
        for case in cases:
            case()
        if cases:
            for k in got:
                COVERED.setdefault(k, set()).add(family)

    for case in larger:
        case()
    for i, value in enumerate(VALUES):
        checked(small, filled(value, kinds if i == 0 else ()))
    checked(larger, filled(0xFF))


class Framed:
    """Pictures of a file call, each in a frame of 0xA5 of its own: `guard` bytes behind every row (the pitch is the row rounded up to 16,
    plus the guard) and one row of the pitch above and below.  places[i] = (row bytes, rows) of file i's place, which the call may write all
    of, or (row bytes, rows, written row bytes, written rows) where it may only write the top left of it."""

    def __init__(self, places, guard=16):
        self.places, self.pitches, self.offs, total = [], [], [], 0
        for place in places:
            wb, rows = max(int(place[0]), 4), max(int(place[1]), 1)         # a file without a picture still gets a place
            pitch = ((wb + 15) & ~15) + guard
            self.places.append((wb, rows) + ((int(place[2]), int(place[3])) if len(place) == 4 else (wb, rows)))
            self.pitches.append(pitch)
            self.offs.append(total + pitch)
            total += pitch * (rows + 2)
        self.total = total
        self.dev = ops.DeviceBuffer(host=np.full(total, FILL, np.uint8))
        n = len(places)
        self.outs = (C.c_void_p * n)(*[self.dev.ptr + o for o in self.offs])
        self.pitch_arr = (C.c_int64 * n)(*self.pitches)

    def read(self):
        """-> [rows x row bytes of every file]; asserts that every frame still holds its 0xA5 around them"""
        flat = self.dev.to_host((self.total,), np.uint8)
        out = []
        for k, ((wb, rows, wwb, wrows), pitch, off) in enumerate(zip(self.places, self.pitches, self.offs)):
            frame = flat[off - pitch:off + pitch * (rows + 1)].reshape(rows + 2, pitch)
            assert (frame[0] == FILL).all() and (frame[wrows + 1:] == FILL).all() and (frame[1:wrows + 1, wwb:] == FILL).all(), ("bytes beside picture", k)
            out.append(frame[1:rows + 1, :wb])
        return out


def files_call(call, files, places, keys, statuses=None):
    """One file call into framed outputs.  call(ptrs, lens, n, outs, pitches, status) -> rc; keys[i]: the answer key [h][w][4] of file i (compared
    with the top-left h x w pixels of its place) or None for a file that must fail; statuses: {i: the code file i must have} for those.
    -> (rc, [status])"""
    n = len(files)
    fr = Framed(places)
    bufs, ptrs, lens = ops.file_args(files)
    status = (C.c_int * n)()
    rc = call(ptrs, lens, n, fr.outs, fr.pitch_arr, status)
    status = list(status)
    got = fr.read()
    for i, (key, rows) in enumerate(zip(keys, got)):
        if key is None:
            assert status[i] != 0, (i, status)
            if statuses and i in statuses:
                assert status[i] == statuses[i], (i, status[i], statuses[i])
            continue
        assert status[i] == 0, (i, status)
        h, w = key.shape[:2]
        pic = rows[:h, :4 * w].reshape(h, w, 4)
        assert np.array_equal(pic, key), (i, np.argwhere(pic != key)[:4].tolist(), int((pic != key).sum()))
    firsts = [s for s in status if s]
    assert rc == (firsts[0] if firsts else 0), (rc, status)
    return rc, status


def tensor_files_call(call, files, fmt, shapes, keys, stream=None):
    """One files-to-tensors call into test_resize_gpu.Outputs (one 0xA5 allocation, ragged offsets and strides).  call(ptrs, lens, n, fmt, outs,
    status) -> rc; shapes[i] = (h, w) of file i's tensor; keys[i]: the BGRA picture [h][w][4] the tensor is made of, None: the file must fail.
    stream: the one `call` runs on (it is waited for before the tensors are read)"""
    from test_resize_gpu import Outputs
    n = len(files)
    outs = Outputs(fmt, shapes)
    for k, key in enumerate(keys):
        if key is not None:
            outs.expect(k, key)
    bufs, ptrs, lens = ops.file_args(files)
    o = (capi.TensorOut * n)(*[capi.TensorOut(*outs.out(k)) for k in range(n)])
    status = (C.c_int * n)()
    rc = call(ptrs, lens, n, C.byref(fmt), o, status)
    status = list(status)
    assert [bool(s) for s in status] == [key is None for key in keys], status
    firsts = [s for s in status if s]
    assert rc == (firsts[0] if firsts else 0), (rc, status)
    if stream is not None:
        capi.sync(stream)
    got = outs.read()
    assert np.array_equal(got, outs.exp), np.flatnonzero(got != outs.exp)[:8].tolist()
    return status
