"""GPU: ffhip_inflate_streams_device (k_inflate, a wave per stream) on the streams of inflate_cases.py: the good ones against
zlib.decompress in batches of 1, 63, 64, 65 and 300, the damaged ones -- every prefix and every single-bit flip of one stream, good
streams among them -- against the host decoder's verdicts, in one launch each.  Every destination is a piece of one allocation filled
with 0xA5, 64 guard bytes between the pieces: the guards and the bytes beyond out_len have to stay as they were."""
import zlib

import numpy as np
import pytest

import inflate_cases as IC
from ffpic_amd import capi, ops

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64


def run(streams, caps):
    """-> (outputs, status); asserts that nothing outside an accepted stream's out_len bytes, or a refused one's cap bytes, was written"""
    outputs, status, flat, offs = ops.inflate_streams_device(streams, caps, strict=False, guard=GUARD, fill=FILL)
    keep = np.ones(flat.size, bool)
    for out, code, off, cap in zip(outputs, status, offs, caps):
        keep[off:off + (cap if code else len(out))] = False
    assert (flat[keep] == FILL).all(), np.flatnonzero(keep & (flat != FILL))[:8].tolist()
    return outputs, status


@pytest.fixture(scope="module")
def good():
    capi.require_device(0)
    return [IC.valid()[name] for name in sorted(IC.valid())]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_good_streams_in_one_call(good, n):
    batch = [good[k % len(good)] for k in range(n)]
    caps = [len(data) + (k % 3) * 50 for k, (_, data) in enumerate(batch)]     # exact, and with room behind the output
    if n == 300:
        batch[7], caps[7] = (b"", b""), 40                            # an empty stream: refused, nothing written
        batch[11], caps[11] = (IC.valid()["empty"][0], b""), 0        # a stream of no bytes into no buffer at all
        batch[13], caps[13] = batch[13], 0                            # a stream of bytes into no buffer: refused
    outputs, status = run([z for z, _ in batch], caps)
    for k, ((z, data), cap) in enumerate(zip(batch, caps)):
        if len(z) == 0 or cap < len(data):
            assert status[k] == capi.FFHIP_EINVAL and outputs[k] is None, k
        else:
            assert status[k] == 0 and outputs[k] == data == zlib.decompress(z), k


def test_damaged_streams_get_the_host_decoders_verdicts(good):
    """the error exits and the turn cap: one launch, every wave has to come back with its verdict"""
    z, data, bad = IC.damaged()
    streams, step = [], len(bad) // 32
    for k, s in enumerate(bad):
        if k % step == 0 and k // step < 32:
            streams.append(good[(k // step) % len(good)][0])
        streams.append(s)
    want = []
    for s in streams:
        try:
            want.append(ops.inflate(s, 1 << 18))
        except capi.FfhipError:
            want.append(None)
    assert sum(w is not None for w in want) >= 32
    caps = [len(w) if w is not None and len(w) > len(data) + 64 else len(data) + 64 for w in want]
    outputs, status = run(streams, caps)
    assert [s != 0 for s in status] == [w is None for w in want]
    assert all(s in (0, capi.FFHIP_EINVAL) for s in status)
    assert outputs == want


def test_strict_raises_and_caps_are_found(good):
    z, data = good[0]
    outputs, status = ops.inflate_streams_device([z, IC.valid()["level_9"][0]])
    assert status == [0, 0] and outputs[0] == data and outputs[1] == IC.valid()["level_9"][1]
    with pytest.raises(capi.FfhipError):
        ops.inflate_streams_device([z[:-1]], [len(data) + 8])
