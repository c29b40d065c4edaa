"""CPU: the host deflate (ffhip_deflate) on every deflate case of tests/png_encode_cases.py: zlib inflates its streams to the
input, a strict decoder too, the library's own ffhip_inflate and the model of k_inflate too; the bound, the cap, the length rule alone, and
the size conditions of the rule."""
import ctypes as C
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

from ffpic_amd import capi, ops
from png_encode_cases import CHUNK, DEFLATE_CASES

IDS = [c[0] for c in DEFLATE_CASES]
STREAMS = {}


def stream_of(name, data):
    if name not in STREAMS:
        STREAMS[name] = ops.deflate(data)
    return STREAMS[name]


def test_the_chunk_is_the_headers():
    assert capi.FFHIP_DEFLATE_CHUNK == CHUNK
    text = open(os.path.join(os.path.dirname(os.path.dirname(capi.CSRC)), "include", "ffpic_hip.h")).read()
    assert f"#define FFHIP_DEFLATE_CHUNK {CHUNK}\n" in text


@pytest.mark.parametrize("name,data", DEFLATE_CASES, ids=IDS)
def test_streams_inflate_to_the_input(name, data):
    z = stream_of(name, data)
    assert z[:2] == b"\x78\x01" and len(z) <= ops.deflate_bound(len(data))
    assert zlib.decompress(z) == data
    d = zlib.decompressobj(wbits=15)                                      # strict: a distance beyond 32768 or in front of the stream is an error
    assert d.decompress(z) + d.flush() == data and d.eof and d.unused_data == b""
    assert ops.inflate(z, len(data)) == data
    assert ops.inflate_model(z, len(data)) == data
    assert ops.deflate(data) == z                                         # a function of the input alone


@pytest.mark.parametrize("name,data", DEFLATE_CASES, ids=IDS)
def test_a_cap_one_byte_short(name, data):
    z = stream_of(name, data)
    L = capi.lib()
    src = np.frombuffer(data, np.uint8)
    for cap in (len(z), len(z) - 1, 0):
        out = np.full(len(z) + 64, 0xA5, np.uint8)
        n = C.c_size_t()
        rc = L.ffhip_deflate(src.ctypes.data if src.size else None, src.size, out.ctypes.data, cap, C.byref(n))
        assert rc == (0 if cap == len(z) else capi.FFHIP_EDEFLATE_NOSPACE) and n.value == len(z), (cap, rc, n.value)
        assert out[:cap].tobytes() == z[:cap] and (out[cap:] == 0xA5).all()


def test_arguments():
    L = capi.lib()
    n = C.c_size_t()
    buf = np.zeros(64, np.uint8)
    assert L.ffhip_deflate(None, 5, buf.ctypes.data, 64, C.byref(n)) == capi.FFHIP_EINVAL
    assert L.ffhip_deflate(buf.ctypes.data, 5, None, 64, C.byref(n)) == capi.FFHIP_EINVAL
    assert L.ffhip_deflate(buf.ctypes.data, 5, buf.ctypes.data, 64, None) == capi.FFHIP_EINVAL
    assert L.ffhip_deflate(None, 0, None, 0, C.byref(n)) == capi.FFHIP_EDEFLATE_NOSPACE and n.value == 11   # 78 01, 01 00 00 FF FF, Adler
    assert ops.deflate(b"") == b"\x78\x01\x01\x00\x00\xff\xff\x00\x00\x00\x01"
    assert "zlib stream" in L.ffhip_strerror(capi.FFHIP_EDEFLATE_NOSPACE).decode() and "PNG" in L.ffhip_strerror(capi.FFHIP_EPNG_NOSPACE).decode()
    f = np.ones(4, np.uint32)
    out = np.zeros(400, np.uint8)
    for args in ((None, 4, 15, out.ctypes.data), (f.ctypes.data, 4, 15, None), (f.ctypes.data, 0, 15, out.ctypes.data), (f.ctypes.data, 289, 15, out.ctypes.data),
                 (f.ctypes.data, 4, 0, out.ctypes.data), (f.ctypes.data, 4, 16, out.ctypes.data), (f.ctypes.data, 4, 1, out.ctypes.data)):
        assert L.ffhip_deflate_code_lengths(*args) == capi.FFHIP_EINVAL, args


def test_the_bound_holds_the_chunks():
    for n, chunks in ((0, 1), (1, 1), (CHUNK, 1), (CHUNK + 1, 2), (5 * CHUNK, 5)):
        assert ops.deflate_bound(n) == 2 + n + 5 * chunks + 5 * (chunks - 1) + 4


def test_blocks_and_joints():
    """every chunk but the last ends in an empty stored block at a byte boundary: the stream cut behind chunk k's 00 00 FF FF inflates, as a
    raw deflate stream, to exactly the first k chunks"""
    data = dict(DEFLATE_CASES)["len%d" % (2 * CHUNK + 300)]
    z = stream_of("len%d" % (2 * CHUNK + 300), data)
    marks = [i + 4 for i in range(2, len(z) - 4) if z[i:i + 4] == b"\x00\x00\xff\xff"]
    cuts = []
    for m in marks:
        d = zlib.decompressobj(wbits=-15)
        got = d.decompress(z[2:m])
        if len(got) % CHUNK == 0 and got == data[:len(got)] and len(got):
            cuts.append(len(got))
    assert CHUNK in cuts and 2 * CHUNK in cuts


def kraft(lengths):
    return sum(Fraction(1, 1 << int(l)) for l in lengths if l)


def fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


@pytest.mark.parametrize("freq,limit", [(fib(40), 15), (fib(19), 7), ([0, 0, 7, 0], 15), ([0, 3, 0, 9, 0], 15), ([5] * 19, 7), ([5] * 286, 15),
                                        ([1] * 30, 15), (fib(30)[::-1] + [0] * 10, 15)],
                         ids=["fib40", "fib19", "one", "two", "equal19", "equal286", "equal30", "fib-reversed"])
def test_code_lengths(freq, limit):
    lengths = ops.deflate_code_lengths(freq, limit)
    used = [k for k, f in enumerate(freq) if f]
    assert all((lengths[k] > 0) == (freq[k] > 0) for k in range(len(freq)))
    assert max(lengths) <= limit
    if len(used) >= 2:
        assert kraft(lengths) == 1
    else:
        assert [lengths[k] for k in used] == [1]
    order = sorted(used, key=lambda k: (freq[k], k))                      # a more frequent symbol never has the longer code
    assert all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]))


def test_code_lengths_without_a_limit_in_the_way_are_huffmans():
    freq = [1, 1, 2, 4, 8, 16, 32]
    assert list(ops.deflate_code_lengths(freq, 15)) == [6, 6, 5, 4, 3, 2, 1]
    assert max(ops.deflate_code_lengths(fib(40), 15)) == 15 and kraft(ops.deflate_code_lengths(fib(40), 15)) == 1


def test_sizes():
    cases = dict(DEFLATE_CASES)
    n16 = stream_of("noise16", cases["noise16"])
    assert len(cases["noise16"]) == 65536 and len(n16) <= 0.625 * 65536, len(n16)       # a 17-symbol code: fixed codes and stored blocks cannot
    noise = stream_of("noise", cases["noise"])
    assert len(noise) <= ops.deflate_bound(len(cases["noise"]))
    zeros = stream_of("zeros", cases["zeros"])
    assert len(zeros) <= 200, len(zeros)                                  # 258-byte matches: some 130 tokens a chunk
