"""GPU: the protocol of tests/scratch_fill.py on ffhip_vp8_encode_items: SCRATCH_VP8_ENC overwritten with a pattern between
calls, the files the host entry's every time.  This module runs in front of tests/test_scratch_fill_gpu.py, whose last test asks that every
scratch kind was filled in front of a checked run; tests/test_vp8_encode_scratch_gpu.py, which runs behind it, has the encoder's other
scratch and thread tests."""
import pytest

import scratch_fill as SF
from test_vp8_encode_gpu import encode_call, host_file
from vp8_encode_cases import CASES

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
        SF.run_protocol("vp8_encode", stream, [run(CASES, "mixed")], [run(CASES[::3], "CHW"), run(CASES[1:4], "HWC")], kinds=("SCRATCH_VP8_ENC",))
    finally:
        L.ffhip_stream_destroy(stream)
