"""GPU: the lossless WebP encoder's scratch is no input.  The protocol of tests/scratch_fill.py on
ffhip_vp8l_encode_items: SCRATCH_VP8L_ENC overwritten with a pattern between calls, the files the host entry's every time.  This module
runs in front of tests/test_scratch_fill_gpu.py, whose last test asks that every scratch kind was filled in front of a checked run."""
import pytest

import scratch_fill as SF
from test_vp8l_encode_gpu import encode_call, host_file
from vp8l_encode_cases import LARGE, SMALL

pytestmark = pytest.mark.gpu


def test_the_scratch_is_no_input():
    L = SF.lib()
    stream = L.ffhip_stream_create()
    try:
        def run(cases, form):
            def case():
                files, _, status = encode_call(cases, form=form, stream=stream)
                assert status == [0] * len(cases) and files == [host_file(c) for c in cases]
            return case
        small = SMALL[::4]
        SF.run_protocol("vp8l_encode", stream, [run(LARGE + SMALL[::3], "HWC")], [run(small, "CHW"), run(small[:3], "mixed")], kinds=("SCRATCH_VP8L_ENC",))
    finally:
        L.ffhip_stream_destroy(stream)
