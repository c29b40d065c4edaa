"""GPU: ffhip_deflate_streams_device (k_deflate_chunks) against the host entry ffhip_deflate, which compiles the same body
and which tests/test_deflate.py holds to zlib on the CPU: every deflate case in ONE call and one call per case, byte for byte, inside an
arena of 0xA5; a stream that does not fit between two that do; the argument checks."""
import ctypes as C

import numpy as np
import pytest

from ffpic_amd import capi, ops
from png_encode_cases import DEFLATE_CASES

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xA5, 256
NOSPACE = capi.FFHIP_EDEFLATE_NOSPACE
HOST = {}


def host(name, data):
    if name not in HOST:
        HOST[name] = ops.deflate(data)
    return HOST[name]


def check(names, datas, caps, streams, lens, status, flat, offs):
    for k, (name, data) in enumerate(zip(names, datas)):
        want = host(name, data)
        cap = ops.deflate_bound(len(data)) if caps is None or caps[k] is None else caps[k]
        assert lens[k] == len(want), (name, lens[k], len(want))
        assert status[k] == (0 if len(want) <= cap else NOSPACE), (name, status[k])
        assert streams[k] == want[:cap], (name, next((i for i, (a, b) in enumerate(zip(streams[k], want)) if a != b), None))
        end = offs[k] + min(len(want), cap)
        assert (flat[end:offs[k] + cap + GUARD] == FILL).all() and (flat[offs[k] - GUARD:offs[k]] == FILL).all(), ("bytes beside a stream", name)


def test_every_case_in_one_call():
    capi.require_device()
    names, datas = [c[0] for c in DEFLATE_CASES], [c[1] for c in DEFLATE_CASES]
    streams, lens, status, flat, offs = ops.deflate_streams_device(datas, guard=GUARD, fill=FILL)
    assert status == [0] * len(datas)
    check(names, datas, None, streams, lens, status, flat, offs)


def test_one_call_per_case():
    capi.require_device()
    for name, data in DEFLATE_CASES:
        streams, lens, status, flat, offs = ops.deflate_streams_device([data], guard=GUARD, fill=FILL)
        check([name], [data], None, streams, lens, status, flat, offs)


def test_a_stream_that_does_not_fit_between_two_that_do():
    capi.require_device()
    cases = dict(DEFLATE_CASES)
    names = ["period7", "noise16", "zeros", "len3", "noise"]
    datas = [cases[n] for n in names]
    caps = [None, len(host("noise16", cases["noise16"])) - 1, len(host("zeros", cases["zeros"])), 0, 7]
    streams, lens, status, flat, offs = ops.deflate_streams_device(datas, caps=caps, strict=False, guard=GUARD, fill=FILL)
    assert status == [0, NOSPACE, 0, NOSPACE, NOSPACE]
    check(names, datas, caps, streams, lens, status, flat, offs)
    with pytest.raises(capi.FfhipError):
        ops.deflate_streams_device(datas[:2], caps=caps[:2], guard=GUARD, fill=FILL)


def test_arguments_come_before_the_device():
    L = capi.lib()
    one = (C.c_void_p * 1)(16)
    nul = (C.c_void_p * 1)(None)
    sz = (C.c_size_t * 1)(5)
    zero = (C.c_size_t * 1)(0)
    got, status = (C.c_size_t * 1)(), (C.c_int * 1)()
    E = capi.FFHIP_EINVAL
    assert L.ffhip_deflate_streams_device(one, sz, -1, one, sz, got, status, None) == E
    assert L.ffhip_deflate_streams_device(None, sz, 1, one, sz, got, status, None) == E
    assert L.ffhip_deflate_streams_device(one, sz, 1, one, sz, None, status, None) == E
    assert L.ffhip_deflate_streams_device(one, sz, 1, one, sz, got, None, None) == E
    assert L.ffhip_deflate_streams_device(nul, sz, 1, one, sz, got, status, None) == E        # bytes without a buffer
    assert L.ffhip_deflate_streams_device(one, sz, 1, nul, sz, got, status, None) == E        # room without a buffer
    big = (C.c_size_t * 1)((1 << 32) - 8)
    assert L.ffhip_deflate_streams_device(one, big, 1, nul, zero, got, status, None) == E     # the bound reaches 2^32
    capi.require_device()
    assert L.ffhip_deflate_streams_device(None, None, 0, None, None, None, None, None) == 0
