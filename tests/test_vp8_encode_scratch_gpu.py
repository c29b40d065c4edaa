"""GPU: the lossy WebP encoder's scratch is no input, and two threads may encode at once.  ffhip_debug_scratch_fill sets
every byte the library keeps for the stream to 0xA5, then to 0x00, between calls of ffhip_vp8_encode_items: the files are the host
entry's every time.  Two threads, a stream each, encode the whole batch at once: their files are the serial ones."""
import threading

import pytest

import scratch_fill as SF
from test_vp8_encode_gpu import encode_call, host_file
from vp8_encode_cases import CASES

pytestmark = pytest.mark.gpu


def test_the_same_bytes_whatever_the_scratch_held():
    L = SF.lib()
    stream = L.ffhip_stream_create()
    try:
        wants = [host_file(c) for c in CASES]
        table = SF.enum_kinds()
        for value in (None, 0xA5, 0x00):
            if value is not None:
                SF.capi.sync(stream)
                dev, host, kinds = SF.fill(stream, value)
                assert dev > 0 and "SCRATCH_VP8_ENC" in {SF.base_of(k, table) for k in kinds}
            files, _, status = encode_call(CASES, form="mixed", stream=stream)
            assert status == [0] * len(CASES) and files == wants, value
    finally:
        L.ffhip_stream_destroy(stream)


def test_two_threads_a_stream_each():
    L = SF.lib()
    wants = [host_file(c) for c in CASES]
    serial, _, _ = encode_call(CASES, form="mixed")
    assert serial == wants
    results, errors = {}, []
    barrier = threading.Barrier(2)

    def work(k):
        stream = L.ffhip_stream_create()
        try:
            barrier.wait()
            for _ in range(2):
                files, _, status = encode_call(CASES, form="mixed", stream=stream)
                assert status == [0] * len(CASES)
                results.setdefault(k, []).append(files)
        except BaseException as e:                                           # the main thread reports it
            errors.append(e)
        finally:
            L.ffhip_stream_destroy(stream)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(files == serial for k in range(2) for files in results[k])
