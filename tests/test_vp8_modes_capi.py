"""The rule for a VP8 mode record, without a GPU: ffhip_vp8_modes_ok_host (vp8_mode_record_valid, the one predicate of every check) against
the rule stated in numpy."""
import ctypes as C
import os

import numpy as np

from ffpic_amd import capi


def test_mode_record_rule():
    """byte 0 <= 4, byte 1 <= 3, and bytes 2..17 <= 9 only when byte 0 is 4 (B_PRED); bytes 18 and 19 are free.  All 256 values in each of
    the 18 positions of an otherwise valid B_PRED record and of an otherwise valid record that is not B_PRED: 2 x 18 x 256 single records."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = capi.lib()
    L.ffhip_vp8_modes_ok_host.argtypes = [C.c_void_p, C.c_longlong]
    L.ffhip_vp8_modes_ok_host.restype = C.c_int
    bases = [np.array([4, 2] + [(3 * k) % 10 for k in range(16)] + [3, 0xee], np.uint8),
             np.array([1, 3] + [(7 * k) % 10 for k in range(16)] + [0xff, 0x80], np.uint8)]
    recs = np.stack([np.broadcast_to(b, (18, 256, 20)) for b in bases]).copy()              # [base][position][value][byte]
    for p in range(18):
        recs[:, p, :, p] = np.arange(256)
    recs = recs.reshape(-1, 20)
    want = (recs[:, 0] <= 4) & (recs[:, 1] <= 3) & ((recs[:, 0] != 4) | (recs[:, 2:18] <= 9).all(axis=1))
    assert len(recs) == 2 * 18 * 256 and want.sum() not in (0, len(want))
    got = np.array([L.ffhip_vp8_modes_ok_host(r.ctypes.data, 1) for r in recs], bool)
    assert np.array_equal(got, want), recs[got != want][:4]
    for free in (18, 19):                                                                     # any value there, either record kind
        for b in bases:
            r = np.broadcast_to(b, (256, 20)).copy()
            r[:, free] = np.arange(256)
            assert L.ffhip_vp8_modes_ok_host(r.ctypes.data, 256) == 1
    both = np.stack([bases[0], recs[~want][0]])                                              # a bad record behind a good one
    assert L.ffhip_vp8_modes_ok_host(both.ctypes.data, 2) == 0 and L.ffhip_vp8_modes_ok_host(both.ctypes.data, 1) == 1
