"""CPU: ffhip_inflate_model (ops.inflate_model), the host model of k_inflate -- the body the kernel compiles with the wave's 64 lanes emulated,
every step as all 64 loads, then all 64 stores -- against zlib.decompress and the host decoder (ops.inflate, ops.inflate_upto): bytes
where a stream is accepted, the verdict everywhere, `partial` included.  Every call has to RETURN: the loops of the body are what the
kernel runs, and one that does not end has to show here, not on a card."""
import time
import zlib

import pytest

import inflate_cases as IC
from ffpic_amd import capi, ops
from test_inflate import CASES, Bits, deflate, mixed, zwrap


def verdict(fn, *args, **kw):
    """-> the bytes, or None for FFHIP_EINVAL"""
    try:
        return fn(*args, **kw)
    except capi.FfhipError as e:
        assert str(capi.FFHIP_EINVAL) in str(e)
        return None


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_zlib_and_the_host_decoder(name):
    data, how = CASES[name]
    z = deflate(data, **how)
    assert zlib.decompress(z) == data
    for cap in (len(data), len(data) + 100):
        assert ops.inflate_model(z, cap) == data and ops.inflate(z, cap) == data
    if data:
        assert verdict(ops.inflate_model, z, len(data) - 1) is None and verdict(ops.inflate, z, len(data) - 1) is None
    for cap in sorted({max(len(data) - 1, 0), len(data) // 2, 0}):
        want = verdict(ops.inflate_upto, z, cap, True)
        assert verdict(ops.inflate_model, z, cap, True) == want, cap
        if cap < len(data):
            assert want == data[:cap]


def test_every_prefix_and_every_bit_flip_gets_the_host_decoders_verdict():
    z, data, bad = IC.damaged()
    assert len(bad) == 9 * len(z) and ops.inflate_model(z, len(data)) == data
    t0 = time.monotonic()
    accepted = 0
    for k, s in enumerate(bad):
        want = verdict(ops.inflate, s, len(data) + 64)
        assert verdict(ops.inflate_model, s, len(data) + 64) == want, k
        assert verdict(ops.inflate_model, s, 100, True) == verdict(ops.inflate_upto, s, 100, True), k
        accepted += want is not None
    assert time.monotonic() - t0 < 60                                  # about 0.1 s; a turn cap that did not hold would run into this
    assert accepted < len(bad) // 100                                  # Adler-32 and the code structure catch nearly everything


@pytest.mark.parametrize("name", sorted(IC.refused_by_hand()))
def test_hand_written_streams_that_are_refused(name):
    z = IC.refused_by_hand()[name]
    assert verdict(ops.inflate, z, 1 << 16) is None and verdict(ops.inflate_model, z, 1 << 16) is None
    assert verdict(ops.inflate_model, z, 2, True) == verdict(ops.inflate_upto, z, 2, True)
    with pytest.raises(zlib.error):
        zlib.decompress(z)


@pytest.mark.parametrize("name", ["one_code_distance_tree", "long_codes", "distances_and_lengths", "stored_lengths", "two_hundred_blocks"])
def test_hand_written_streams_that_are_good(name):
    z, data = IC.valid()[name]                                        # valid() has held each against zlib
    assert ops.inflate_model(z, len(data)) == data and ops.inflate(z, len(data)) == data
    assert verdict(ops.inflate_model, z, len(data) - 1) is None
    for cap in (len(data) - 1, len(data) // 2, 0):
        assert ops.inflate_model(z, cap, True) == ops.inflate_upto(z, cap, True) == data[:cap]


def test_what_the_hand_written_streams_hold():
    z, data = IC.valid()["long_codes"]
    assert data[:13] == b"ABCDEFGHIJK\x00L" and data[13:16] == b"LLL" and data[16:274] == b"LL" * 129 and len(data) == 274 + 3 * 14
    z, data = IC.valid()["distances_and_lengths"]
    assert len(data) == 32768 + 8 * (3 + 4 + 63 + 64 + 65 + 257 + 258 + 7)
    assert data[32768:32771] == data[32767:32768] * 3                 # length 3 at distance 1
    z, data = IC.valid()["stored_lengths"]
    assert z[2:7] == b"\x00\x00\x00\xff\xff" and z[7:12] == b"\x00\x01\x00\xfe\xff" and z[13:18] == b"\x01\xff\xff\x00\x00"
    z, data = IC.valid()["two_hundred_blocks"]
    assert z.count(b"\x00\x00\xff\xff") >= 100                        # the empty stored block of every full flush


def test_the_step_emulation_sees_a_hazard_within_a_step():
    """The kernel's match addresses, dst[match - distance + ((k0 + k) % distance)], lie in front of the match, so a step of them has no
    load that reads another lane's store, and running them lane after lane (mode 3) changes nothing.  What shows that the emulation --
    all 64 loads, then all 64 stores -- WOULD see such a dependence is the address a byte-by-byte copy uses, dst[to - distance + k]: with
    distance < 64 its loads read bytes that stores of the same step write.  Run as steps (mode 1) it gives wrong bytes; run lane after
    lane (mode 2) it is the byte-by-byte copy and right again."""
    b = Bits().field(1, 1).field(1, 2)
    for v in b"ABC":
        b.fixed_literal(v)
    IC.fixed_match(b, 258, 3)
    b.fixed_literal(256)
    key = b"ABC" * 87
    z = zwrap(b.done(), key)
    assert zlib.decompress(z) == key
    assert ops.inflate_model(z, len(key)) == key
    assert ops.inflate_model(z, len(key), mode=3) == key and ops.inflate_model(z, len(key), mode=2) == key
    got = verdict(ops.inflate_model, z, len(key), mode=1)             # the wrong bytes fail the check value, or come back
    assert got != key
    got = ops.inflate_model(z, len(key) - 1, partial=True, mode=1)    # partial: no check value, the bytes themselves
    assert got[:6] == key[:6] and got != key[:len(key) - 1]
