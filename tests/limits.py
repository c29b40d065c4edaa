"""What test_limits_gpu.py and test_limits.py share: device allocations that are almost entirely 0xA5 padding, and the answer keys that the
existing rules cannot give at the limits -- the resize rule per output index in Python integers (axis_matrix is dense: 16384 x 16383 does
not fit), the tensor stage's float keys at the edges of F16 and F32.  Nothing here calls the library."""
import numpy as np

FILL = 0xA5
MARGIN = 1 << 20                                  # bytes of 0xA5 in front of and behind every region a kernel is given
BIL, AA = 0, 1                                    # FFHIP_RESIZE_BILINEAR, FFHIP_RESIZE_ANTIALIAS
U8, F16, F32 = 0, 1, 2                            # FFHIP_TENSOR_*
NP_DTYPE = {U8: np.uint8, F16: np.float16, F32: np.float32}


# ---------------------------------------------------------------------------------------------------- device memory
class Layout:
    """Regions of one allocation, each with MARGIN bytes of padding in front of it; allocate() adds the last margin"""

    def __init__(self):
        self.at = 0

    def add(self, nbytes):
        off = (self.at + MARGIN + 255) // 256 * 256
        self.at = off + nbytes
        return off

    def allocate(self):
        return Arena(self.at + MARGIN)


class Arena:
    """One torch uint8 tensor on the device filled with 0xA5; never mirrored on the host: rows go up and come back rectangle by rectangle,
    everything else is counted on the device"""

    def __init__(self, nbytes):
        import torch
        self.torch, self.nbytes = torch, nbytes
        self.t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        assert self.ptr % 256 == 0

    def rows(self, off, pitch, h, row_bytes):
        assert 0 <= off and off + pitch * (h - 1) + row_bytes <= self.nbytes
        return self.t[off:].as_strided((h, row_bytes), (pitch, 1))

    def put(self, off, pitch, host):
        """host [h][row_bytes] uint8 to rows `pitch` apart"""
        host = np.ascontiguousarray(host)
        self.rows(off, pitch, host.shape[0], host.shape[1]).copy_(self.torch.from_numpy(host))

    def get(self, off, pitch, h, row_bytes):
        return self.rows(off, pitch, h, row_bytes).cpu().numpy()

    def changed(self):
        """bytes of the whole allocation that are not 0xA5, counted on the device a GiB at a time"""
        self.torch.cuda.synchronize()
        return sum(int((self.t[a:a + (1 << 30)] != FILL).sum()) for a in range(0, self.nbytes, 1 << 30))

    def check(self, rects):
        """rects (off, pitch, expected [h][row_bytes] uint8): each holds its bytes, and nothing else of the allocation changed"""
        for k, (off, pitch, exp) in enumerate(rects):
            got = self.get(off, pitch, exp.shape[0], exp.shape[1])
            assert np.array_equal(got, exp), f"rectangle {k} at {off:#x}, pitch {pitch:#x}"
        assert self.changed() == sum(int((exp != FILL).sum()) for _, _, exp in rects)

    def free(self):
        self.t = None
        self.torch.cuda.empty_cache()


def pixel_rows(pic):
    """[h][w][4] uint8 -> [h][4 w]"""
    return np.ascontiguousarray(pic).reshape(pic.shape[0], -1)


def tensor_rects(off, es, planar, row_stride, plane_stride, exp):
    """the rectangles of a tensor output at byte `off` (strides in elements of `es` bytes): exp [3][h][w] or [h][w][3] of the output's type"""
    exp = np.ascontiguousarray(exp)
    if planar:
        return [(off + c * plane_stride * es, row_stride * es, exp[c].view(np.uint8).reshape(exp.shape[1], -1)) for c in range(3)]
    return [(off, row_stride * es, exp.view(np.uint8).reshape(exp.shape[0], -1))]


def tensor_span(es, planar, row_stride, plane_stride, h, w):
    """bytes from the first to behind the last element of a tensor output"""
    return ((2 * plane_stride if planar else 0) + row_stride * (h - 1) + (w if planar else 3 * w)) * es


# ---------------------------------------------------------------------------------------------------- the resize rule, one output at a time
_TAPS = {}


def axis_taps(n_in, n_out, filt, o):
    """(first, q int64) of output o: the header's rule in Python integers, over the run alone -- no [n_out][n_in] matrix"""
    S = 2 * max(n_in, n_out) if filt == AA else 2 * n_out
    c = (2 * o + 1) * n_in
    # d_k = |(2 k + 1) n_out - c| < S  <=>  (c - S - n_out) / (2 n_out) < k < (c + S - n_out) / (2 n_out)
    k_lo = max(0, (c - S - n_out) // (2 * n_out) + 1)
    k_hi = min(n_in - 1, -((-(c + S - n_out)) // (2 * n_out)) - 1)
    assert k_lo <= k_hi
    k = np.arange(k_lo, k_hi + 1, dtype=np.int64)
    d = np.abs((2 * k + 1) * n_out - c)
    assert np.all(d < S)
    assert k_lo == 0 or abs((2 * k_lo - 1) * n_out - c) >= S
    assert k_hi == n_in - 1 or abs((2 * k_hi + 3) * n_out - c) >= S
    r = S - d
    R = int(r.sum())
    q = (r * 4096 + R // 2) // R
    m = int(np.argmax(r))                                       # the lowest k on a tie
    q[m] += 4096 - int(q.sum())
    if q[m] < 0:                                                # step 5: the next taps in the same order pay
        owed, q[m] = -int(q[m]), 0
        rest = np.lexsort((np.arange(len(r)), -r))[1:]
        before = np.cumsum(q[rest]) - q[rest]
        q[rest] -= np.clip(owed - before, 0, q[rest])
    assert int(q.sum()) == 4096 and int(q.min()) >= 0
    return k_lo, q


def axis_runs(n_in, n_out, filt):
    key = (n_in, n_out, filt)
    if key not in _TAPS:
        _TAPS[key] = [axis_taps(n_in, n_out, filt, o) for o in range(n_out)]
    return _TAPS[key]


def resize_sparse(v, oh, ow, filt):
    """[h][w][C] uint8 -> [oh][ow][C] uint8 by the rule, run by run: (sum_y qy sum_x qx v + 2^23) >> 24"""
    h, w = v.shape[:2]
    v = v.astype(np.int64)
    hor = np.empty((h, ow, v.shape[2]), np.int64)
    for ox, (first, q) in enumerate(axis_runs(w, ow, filt)):
        hor[:, ox] = np.einsum("ynC,n->yC", v[:, first:first + len(q)], q)
    out = np.empty((oh, ow, v.shape[2]), np.int64)
    for oy, (first, q) in enumerate(axis_runs(h, oh, filt)):
        out[oy] = np.einsum("nxC,n->xC", hor[first:first + len(q)], q)
    out = (out + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# the side limits of a resize item (include/ffpic_hip.h): (source w, h, output w, h)
SIDE_CASES = [(16384, 2, 16384, 2), (16384, 2, 1, 1), (2, 16384, 1, 1), (1, 1, 16384, 1), (1, 1, 1, 16384), (16383, 1, 16384, 1), (16384, 1, 16383, 1)]


# ---------------------------------------------------------------------------------------------------- the JPEG recon items' limits
# per fused layout class: (ncomp, h, v, MCUs of one unit) -- a quad of 4:2:0, two strips of 4:4:4, 4:2:2 and 4:4:0, one strip otherwise.
# a JPEG recon item may have 4096 units in a picture row and 2^20 in a picture (include/ffpic_hip.h)
JPEG_CLASSES = {"420": (3, 2, 2, 4), "444": (3, 1, 1, 16), "422": (3, 2, 1, 8), "440": (3, 1, 2, 8), "h4v1": (3, 4, 1, 4), "h1v4": (3, 1, 4, 4),
                "grey": (1, 1, 1, 8)}
JPEG_UNITS_PER_ROW, JPEG_UNITS_PER_PICTURE = 4096, 1 << 20
JPEG_MAX_PITCH = 0x7fffff0                        # the largest multiple of 16 with pitch x 16 <= 2^31 - 1


def jpeg_max_cols(layout):
    return JPEG_UNITS_PER_ROW * JPEG_CLASSES[layout][3]


# ---------------------------------------------------------------------------------------------------- the tensor stage's floats at their edges
# (scale, bias) for all three channels, and what the key must hold for the case to say anything
FLOAT_EDGES = [
    (300.0, 0.0, "inf"), (-300.0, 0.0, "-inf"), (2.0 ** -24, 0.0, "f16 subnormal"), (2.0 ** -25, 0.0, "f16 tie"),
    (1e-40, 0.0, "f32 subnormal"), (1e-38, -1e-38, "f32 subnormal sum"), (-1.0, 0.0, "zero"), (-1.0, -0.0, "-zero"),
]


def byte_ramps():
    """[2][256][4]: every byte value in every channel (test_all_byte_values_in_every_channel's picture)"""
    src = np.zeros((2, 256, 4), np.uint8)
    for c in range(3):
        src[0, :, c] = (np.arange(256) + 37 * c) % 256
        src[1, :, c] = (255 - np.arange(256) + 91 * c) % 256
    src[..., 3] = np.arange(256) * 7 % 256
    return src


def float_key(bgra, dtype, planar, bgr, scale, bias):
    """numpy float32 arithmetic, the product and the sum as separate operations, then astype"""
    v = bgra[..., [0, 1, 2] if bgr else [2, 1, 0]].astype(np.float32)
    prod = v * np.float32(scale)
    assert prod.dtype == np.float32
    total = prod + np.float32(bias)
    assert total.dtype == np.float32
    with np.errstate(over="ignore"):                           # F16 overflow to inf is what some cases are there for
        out = total.astype(NP_DTYPE[dtype])
    return np.ascontiguousarray(out.transpose(2, 0, 1) if planar else out)


def float_key_holds(key, what):
    """does the key contain what the edge case is there for"""
    bits = key.view(np.uint16 if key.dtype == np.float16 else np.uint32).astype(np.int64).ravel()
    nbits = 16 if key.dtype == np.float16 else 32
    mant = 10 if key.dtype == np.float16 else 23
    sign, body = bits >> (nbits - 1), bits & ((1 << (nbits - 1)) - 1)
    subnormal = (body > 0) & (body < (1 << mant))
    if what == "inf":
        return key.dtype != np.float16 or bool(np.any(np.isposinf(key)))
    if what == "-inf":
        return key.dtype != np.float16 or bool(np.any(np.isneginf(key)))
    if what == "f16 subnormal":
        return key.dtype != np.float16 or bool(np.any(subnormal))
    if what == "f16 tie":                                      # 2^-25 x 1 rounds to even: 0; x 3 to 2 x 2^-24
        return key.dtype != np.float16 or (bool(np.any(body == 2)) and bool(np.any(subnormal)) and int((body == 0).sum()) >= 6)
    if what in ("f32 subnormal", "f32 subnormal sum"):
        return key.dtype != np.float32 or bool(np.any(subnormal))
    if what == "zero":
        return bool(np.any((body == 0) & (sign == 0))) and not np.any((body == 0) & (sign == 1))
    if what == "-zero":
        return bool(np.any((body == 0) & (sign == 1)))
    raise ValueError(what)
