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


# ---------------------------------------------------------------------------------------------------- the batch entry points' layouts
# What test_batch_limits_gpu.py runs and test_batch_limits.py asks the argument checks about: a layout is the strides, offsets and sizes
# of one call; `place` lays its operands out (in an arena or at made-up addresses) and `call` passes them to the library
class Planar:
    """one call of ffhip_yuv420_to_bgra (bits 8), ffhip_yuv420_to_bgra_16 (bits 16) or ffhip_yuv400_to_bgra_16 (bits 16, chroma False).
    Strides in samples, offsets in bytes added to the 256-aligned start of a region; None is the tightest value, pitch and image_stride
    None are 4 W + 16 and H pitch + 48"""

    def __init__(self, bits, rows, cols, unit, n, chroma=True, y_off=0, u_off=0, v_off=0, y_stride=None, uv_stride=None, plane_y=None,
                 plane_uv=None, pitch=None, image_stride=None):
        self.bits, self.es, self.chroma, self.rows, self.cols, self.unit, self.n = bits, bits // 8, chroma, rows, cols, unit, n
        self.W, self.H = cols * unit, rows * unit
        self.y_off, self.u_off, self.v_off = y_off, u_off, v_off
        self.y_stride = self.W if y_stride is None else y_stride
        self.uv_stride = self.W // 2 if uv_stride is None else uv_stride
        self.plane_y = self.H * self.y_stride if plane_y is None else plane_y
        self.plane_uv = self.H // 2 * self.uv_stride if plane_uv is None else plane_uv
        self.pitch = 4 * self.W + 16 if pitch is None else pitch
        self.image_stride = self.H * self.pitch + 48 if image_stride is None else image_stride

    def spans(self):
        """bytes of the regions y, u, v, bgra"""
        n1, es = self.n - 1, self.es
        y = self.y_off + (n1 * self.plane_y + (self.H - 1) * self.y_stride + self.W) * es
        c = (n1 * self.plane_uv + (self.H // 2 - 1) * self.uv_stride + self.W // 2) * es
        return y, self.u_off + c, self.v_off + c, n1 * self.image_stride + (self.H - 1) * self.pitch + 4 * self.W

    def place(self, add):
        """add(nbytes) -> offset of a region; -> offsets of y, u, v, bgra (u and v None without chroma)"""
        y, u, v, o = self.spans()
        return (add(y) + self.y_off, add(u) + self.u_off if self.chroma else None, add(v) + self.v_off if self.chroma else None, add(o))

    def call(self, L, base, at):
        y, u, v, o = [None if a is None else base + a for a in at]
        if self.bits == 8:
            return L.ffhip_yuv420_to_bgra(o, self.pitch, y, u, v, self.y_stride, self.uv_stride, self.rows, self.cols, self.n, self.plane_y,
                                          self.plane_uv, self.image_stride, None)
        if self.chroma:
            return L.ffhip_yuv420_to_bgra_16(o, self.pitch, y, u, v, self.y_stride, self.uv_stride, self.rows, self.cols, self.unit, self.n,
                                             self.plane_y, self.plane_uv, self.image_stride, None)
        return L.ffhip_yuv400_to_bgra_16(o, self.pitch, y, self.y_stride, self.rows, self.cols, self.unit, self.n, self.plane_y,
                                         self.image_stride, None)

    def packed(self):
        """the 8-bit call's alignment predicate, restated: does it take the packed kernel"""
        return not (self.y_off & 3 or self.y_stride & 3 or self.plane_y & 3 or self.u_off & 1 or self.v_off & 1 or self.uv_stride & 1
                    or self.plane_uv & 1)


def planar_product(y_off, y_stride_extra):
    """A1's product for one d_y offset and one y_stride: the other settings, at 3 x 2 macroblocks and three images"""
    W, H = 48, 32
    out = []
    for u_off in (0, 1):
        for v_off in (0, 1):
            for uv_extra in (0, 1):
                for odd in (1, 0):                           # plane strides larger than a plane, odd or even
                    ys, uvs = W + y_stride_extra, W // 2 + uv_extra
                    out.append(Planar(8, 2, 3, 16, 3, y_off=y_off, u_off=u_off, v_off=v_off, y_stride=ys, uv_stride=uvs,
                                      plane_y=H * ys + (5 if odd else 8), plane_uv=H // 2 * uvs + (3 if odd else 6)))
    return out


PLANAR_Y_OFFS, PLANAR_Y_EXTRAS = (0, 1, 2), (0, 1, 2, 4)
# ctbsize, rows, cols: height / 2 % 4 != 0, height % 4 != 0 and width / 4 % 64 != 0, two workgroups in x and three or more in y
PLANAR_CTBS = [(2, 11, 134), (6, 3, 46), (10, 3, 26)]
PLANAR_DOMAINS = [(0, 256), (0, 1024), (0, 8192), (-32768, 32768)]          # test_hevc_planes_domains_and_ctb_sizes'


def planar_16(chroma, ctb, rows, cols, **kw):
    W = cols * ctb
    return Planar(16, rows, cols, ctb, 2, chroma=chroma, y_stride=W + 3, uv_stride=W // 2 + 1, **kw)


def planar_far(bits, chroma, y_off=0):
    """B1: two pictures of 3 x 2 macroblocks (or CTBs of 16), the second one's planes past 2^31 bytes, its pixels past 2^32"""
    far = (1 << 31) + 4 if bits == 8 else (1 << 30) + 2
    return Planar(bits, 2, 3, 16, 2, chroma=chroma, y_off=y_off, y_stride=52, uv_stride=26, plane_y=far, plane_uv=far - 2,
                  image_stride=(1 << 32) + 16)


class Grid:
    """one call of ffhip_heif_grid_compose; offsets in bytes added to the 256-aligned start of a region"""

    def __init__(self, rows, cols, tw, th, ow, oh, canvas_pitch=None, tile_pitch=None, tile_stride=None, canvas_off=0, tiles_off=0):
        self.rows, self.cols, self.tw, self.th, self.ow, self.oh = rows, cols, tw, th, ow, oh
        self.canvas_pitch = 4 * ow if canvas_pitch is None else canvas_pitch
        self.tile_pitch = 4 * tw if tile_pitch is None else tile_pitch
        self.tile_stride = self.tile_pitch * th if tile_stride is None else tile_stride
        self.canvas_off, self.tiles_off = canvas_off, tiles_off

    def spans(self):
        tiles = (self.rows * self.cols - 1) * self.tile_stride + (self.th - 1) * self.tile_pitch + 4 * self.tw
        return self.tiles_off + tiles, self.canvas_off + (self.oh - 1) * self.canvas_pitch + 4 * self.ow

    def place(self, add):
        t, c = self.spans()
        return add(t) + self.tiles_off, add(c) + self.canvas_off

    def call(self, L, base, at):
        return L.ffhip_heif_grid_compose(base + at[1], self.canvas_pitch, self.ow, self.oh, base + at[0], self.tile_pitch, self.tile_stride,
                                         self.tw, self.th, self.rows, self.cols, None)

    def vector(self):
        """the entry's choice, restated: the four-pixel kernel"""
        return not (self.tw & 3 or (self.canvas_off | self.tiles_off | self.canvas_pitch | self.tile_pitch | self.tile_stride) & 15)


def up16(v):
    return (v + 15) // 16 * 16


# the vector tail: tiles of 64 x 8, three across and two down, the last row and the last column overhanging
GRID_TAIL = {ow: Grid(2, 3, 64, 8, ow, 13, canvas_pitch=up16(4 * ow) + 16) for ow in (177, 178, 179)}
# the per-pixel kernel by each alignment input in turn, on the layout of the tail case
_G = dict(rows=2, cols=3, tw=64, th=8, ow=178, oh=13)
GRID_UNALIGNED = {"canvas": Grid(**_G, canvas_pitch=736, canvas_off=4), "tiles": Grid(**_G, canvas_pitch=736, tiles_off=4),
                  "canvas_pitch": Grid(**_G, canvas_pitch=740), "tile_pitch": Grid(**_G, canvas_pitch=736, tile_pitch=260),
                  "tile_stride": Grid(**_G, canvas_pitch=736, tile_stride=256 * 8 + 4)}
# the stride gaps, tiles of a width the vector kernel could take and of one it could not
GRID_GAPS = {tw: Grid(3, 2, tw, 18, 2 * tw - 13, 40, canvas_pitch=4 * (2 * tw - 13) + 20, tile_pitch=4 * tw + 32,
                      tile_stride=(4 * tw + 32) * 18 + 64) for tw in (64, 30)}
# B1: the third tile past 2^32, the third canvas row past 2^32
GRID_FAR = {"tile_stride": Grid(1, 3, 64, 8, 178, 5, canvas_pitch=736, tile_stride=(1 << 31) + 16),
            "canvas_pitch": Grid(1, 3, 64, 8, 178, 3, canvas_pitch=(1 << 31) + 16)}


class Fake:
    """made-up addresses for a layout's regions, 256-aligned like an arena's: what the argument checks see without a device"""

    def __init__(self):
        self.lay = Layout()
        self.base = 1 << 40

    def add(self, nbytes):
        return self.lay.add(nbytes)


# the two-pass geometries of ffhip_jpeg_recon_batch, one of each kind: grey with 2 x 2 blocks per MCU, a three-block pair
JPEG_TWO_PASS = {"grey2x2": (1, 2, 2), "h3": (3, 3, 1)}


def jpeg_batch_sizes(name):
    """(mcu_cols, mcu_rows): 5 x 3, and one whole unit and three MCUs of the next in a row"""
    return [(5, 3), (JPEG_CLASSES[name][3] + 3 if name in JPEG_CLASSES else 9, 2)]


# B2: counts whose byte offsets pass 2^31 and 2^32.  The smallest n_mb whose levels (800 bytes a macroblock) pass 2^31 bytes, plus 9;
# (nTbS, n_tu) of the HEVC residual stage: 2^31 bytes of levels and a few units more
VP8_RESIDUAL_FAR = -(-(1 << 31) // 800) + 9
HEVC_RESIDUAL_FAR = [(32, (1 << 20) + 8), (4, (1 << 26) + 300)]
FAR_ENDS = 64                                     # units at either end that come from the host; zeros in between
