"""Operator-level host mirror of the reference interface for the hot path.

Names and argument meaning follow the reference (format/jpg.c:540-560,
utils/idct.h:14-25, utils/colorspace.h:29-33, arch/accl.h:20-25); every function
runs on the GPU through the C ABI of libffpic_hip.so and raises FfhipError when
the library or a gfx950 device is missing (no CPU fallback, by design).
"""
import ctypes as C

import numpy as np

from . import capi


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def jpeg_recon_batch_host(geom, n_images, coef_y, coef_u, coef_v, quant):
    """dequant + idct_8x8 + YUV_to_BGRA32 for a batch held in host numpy arrays
    (the per-picture call a patched format/jpg.c would make).  Returns BGRA
    uint8 [n, H, W, 4]."""
    L = capi.require_device()
    H, W = geom.height, geom.width
    out = np.empty((n_images, H, W, 4), dtype=np.uint8)
    quant = np.ascontiguousarray(quant, dtype=np.uint16)
    qstride = 0 if quant.ndim == 2 else 256
    capi.check(L.ffhip_jpeg_recon_batch_host(C.byref(geom), n_images, _vp(coef_y), _vp(coef_u), _vp(coef_v),
                                              _vp(quant), qstride, _vp(out), W * 4, H * W * 4),
               "ffhip_jpeg_recon_batch_host")
    return out


def jpeg_recon_batch(geom, n_images, d_coef_y, d_coef_u, d_coef_v, d_quant, quant_stride, d_bgra, pitch,
                     image_stride, d_workspace=None, workspace_bytes=0, stream=None):
    """Device-pointer form (ints / c_void_p); only enqueues on `stream`."""
    L = capi.lib()
    capi.check(L.ffhip_jpeg_recon_batch(C.byref(geom), n_images, d_coef_y, d_coef_u, d_coef_v, d_quant,
                                        quant_stride, d_bgra, pitch, image_stride, d_workspace, workspace_bytes,
                                        stream), "ffhip_jpeg_recon_batch")


def idct_8x8(block, bitdepth=8):
    """get_dct_ops(16)->idct_8x8 (utils/idct.c:512-534): in-place on int16[64]."""
    L = capi.require_device()
    ops = L.ffhip_get_dct_ops(16)
    if not ops:
        raise capi.FfhipError("ffhip_get_dct_ops(16) returned NULL")
    assert block.dtype == np.int16 and block.size == 64 and block.flags.c_contiguous
    ops.contents.idct_8x8(block.ctypes.data, bitdepth)
    return block


def idct_4x4(block, bitdepth=8):
    """get_dct_ops(16)->idct_4x4 == VP8 IDCT (utils/idct.c:100-151), in place."""
    L = capi.require_device()
    ops = L.ffhip_get_dct_ops(16)
    if not ops:
        raise capi.FfhipError("ffhip_get_dct_ops(16) returned NULL")
    assert block.dtype == np.int16 and block.size == 16 and block.flags.c_contiguous
    ops.contents.idct_4x4(block.ctypes.data, bitdepth)
    return block


def idct_4x4_hevc(block, bitdepth=8, epp=False):
    """idct_4x4_hevc (utils/idct.c:36-55)."""
    L = capi.require_device()
    out = np.empty(16, dtype=np.int16)
    L.ffhip_idct_4x4_hevc(block.ctypes.data, out.ctypes.data, bitdepth, epp)
    return out


def yuv_to_bgra32(Y, U, V, v, h, pitch=None):
    """get_cs_ops(16)->YUV_to_BGRA32 for one MCU (utils/colorspace.c:133-172)."""
    L = capi.require_device()
    ops = L.ffhip_get_cs_ops(16)
    if not ops:
        raise capi.FfhipError("ffhip_get_cs_ops(16) returned NULL")
    pitch = pitch or 8 * h * 4
    out = np.zeros((8 * v, pitch), dtype=np.uint8)
    ops.contents.YUV_to_BGRA32(out.ctypes.data, pitch, Y.ctypes.data, U.ctypes.data, V.ctypes.data, v, h)
    return out


class DeviceBuffer:
    """Tiny RAII wrapper over ffhip_malloc/ffhip_free for host-driven calls (no torch)."""

    def __init__(self, host=None, nbytes=None):
        L = capi.require_device()
        self.nbytes = host.nbytes if host is not None else nbytes
        self.ptr = L.ffhip_malloc(max(self.nbytes, 16))
        if not self.ptr:
            raise capi.FfhipError("ffhip_malloc failed")
        if host is not None and host.nbytes:
            capi.check(L.ffhip_memcpy_h2d(self.ptr, host.ctypes.data, host.nbytes, None), "h2d")
            capi.check(L.ffhip_stream_sync(None))

    def to_host(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        L = capi.lib()
        capi.check(L.ffhip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, None), "d2h")
        capi.check(L.ffhip_stream_sync(None))
        return out

    def __del__(self):
        try:
            capi.lib().ffhip_free(self.ptr)
        except Exception:
            pass


def yuv420_to_bgra(y, u, v, mbrows, mbcols, pitch=None):
    """YUV420_to_BGRA32 (utils/colorspace.c:291-329): uint8 planes [n][H][W], [n][H/2][W/2]."""
    L = capi.require_device()
    n, H, W = y.shape
    assert (H, W) == (16 * mbrows, 16 * mbcols) and u.shape == (n, H // 2, W // 2) == v.shape
    pitch = pitch or W * 4
    dy, du, dv = DeviceBuffer(np.ascontiguousarray(y)), DeviceBuffer(np.ascontiguousarray(u)), DeviceBuffer(np.ascontiguousarray(v))
    do = DeviceBuffer(nbytes=n * H * pitch)
    capi.check(L.ffhip_memset(do.ptr, 0, do.nbytes, None))
    capi.check(L.ffhip_yuv420_to_bgra(do.ptr, pitch, dy.ptr, du.ptr, dv.ptr, W, W // 2, mbrows, mbcols, n,
                                      H * W, H * W // 4, H * pitch, None), "ffhip_yuv420_to_bgra")
    return do.to_host((n, H, pitch), np.uint8)


def yuv420_to_bgra_16(y, u, v, ctbrows, ctbcols, ctbsize, pitch=None):
    """YUV420_to_BGRA32_16bit (utils/colorspace.c:628-669): int16 planes."""
    L = capi.require_device()
    n, H, W = y.shape
    assert (H, W) == (ctbsize * ctbrows, ctbsize * ctbcols)
    pitch = pitch or W * 4
    dy, du, dv = DeviceBuffer(np.ascontiguousarray(y)), DeviceBuffer(np.ascontiguousarray(u)), DeviceBuffer(np.ascontiguousarray(v))
    do = DeviceBuffer(nbytes=n * H * pitch)
    capi.check(L.ffhip_memset(do.ptr, 0, do.nbytes, None))
    capi.check(L.ffhip_yuv420_to_bgra_16(do.ptr, pitch, dy.ptr, du.ptr, dv.ptr, W, W // 2, ctbrows, ctbcols, ctbsize,
                                         n, H * W, H * W // 4, H * pitch, None), "ffhip_yuv420_to_bgra_16")
    return do.to_host((n, H, pitch), np.uint8)


def yuv400_to_bgra_16(y, ctbrows, ctbcols, ctbsize, pitch=None):
    """YUV400_to_BGRA32_16bit (utils/colorspace.c:715-742)."""
    L = capi.require_device()
    n, H, W = y.shape
    pitch = pitch or W * 4
    dy = DeviceBuffer(np.ascontiguousarray(y))
    do = DeviceBuffer(nbytes=n * H * pitch)
    capi.check(L.ffhip_memset(do.ptr, 0, do.nbytes, None))
    capi.check(L.ffhip_yuv400_to_bgra_16(do.ptr, pitch, dy.ptr, W, ctbrows, ctbcols, ctbsize, n, H * W, H * pitch,
                                         None), "ffhip_yuv400_to_bgra_16")
    return do.to_host((n, H, pitch), np.uint8)


def vp8_residual_batch(levels, mbinfo, quant):
    """Per-macroblock residual of vp8_decode_residual_block (format/webp.c:1147-1196):
    levels int16 [n][25][16], mbinfo uint8 [n][32], quant uint16 [4][8] -> int16 [n][384]."""
    L = capi.require_device()
    n = levels.shape[0]
    assert levels.shape == (n, 25, 16) and mbinfo.shape == (n, 32) and quant.shape == (4, 8)
    dl, di, dq = DeviceBuffer(np.ascontiguousarray(levels)), DeviceBuffer(np.ascontiguousarray(mbinfo)), \
        DeviceBuffer(np.ascontiguousarray(quant))
    do = DeviceBuffer(nbytes=n * 384 * 2)
    capi.check(L.ffhip_vp8_residual_batch(n, dl.ptr, di.ptr, dq.ptr, do.ptr, None), "ffhip_vp8_residual_batch")
    return do.to_host((n, 384), np.int16)


def hevc_residual_batch(n, level, tuinfo, bitdepth=8, epp=False, scaling=None):
    """scale_and_transform (coding/hevc.c:4172-4251) for a batch of n x n TUs:
    level int16 [n_tu][n*n] row-major, tuinfo uint8 [n_tu][4] -> residual int16 [n_tu][n*n]."""
    L = capi.require_device()
    n_tu = level.shape[0]
    assert level.shape == (n_tu, n * n) and tuinfo.shape == (n_tu, 4)
    dl, di = DeviceBuffer(np.ascontiguousarray(level)), DeviceBuffer(np.ascontiguousarray(tuinfo))
    ds = DeviceBuffer(np.ascontiguousarray(scaling)) if scaling is not None else None
    do = DeviceBuffer(nbytes=max(n_tu * n * n * 2, 16))
    capi.check(L.ffhip_hevc_residual_batch(n, n_tu, dl.ptr, di.ptr, ds.ptr if ds else None, bitdepth, int(epp),
                                           do.ptr, None), "ffhip_hevc_residual_batch")
    return do.to_host((n_tu, n * n), np.int16)


def vp8_predict_recon(mbcols, mbrows, modes, residual, resmap=None):
    """vp8_prerdict_mb over whole key frames (format/webp.c:1833-1851, format/predict.c:426-645).
    modes uint8 [n][n_mb][20], residual int16 [n][rows][384], resmap int32 [n][n_mb] or None.
    Returns zero-initialised planes after reconstruction: (Y [n][16r][16c], U, V)."""
    L = capi.require_device()
    n, n_mb = modes.shape[0], mbcols * mbrows
    assert modes.shape == (n, n_mb, 20) and residual.shape[0] == n and residual.shape[2] == 384
    modes = np.ascontiguousarray(modes)
    dm, dr = DeviceBuffer(modes), DeviceBuffer(np.ascontiguousarray(residual))
    dmap = DeviceBuffer(np.ascontiguousarray(resmap, dtype=np.int32)) if resmap is not None else None
    ysz, csz = 256 * n_mb, 64 * n_mb
    dy, du, dv = DeviceBuffer(nbytes=n * ysz), DeviceBuffer(nbytes=n * csz), DeviceBuffer(nbytes=n * csz)
    for d in (dy, du, dv):
        capi.check(L.ffhip_memset(d.ptr, 0, d.nbytes, None))
    capi.check(L.ffhip_vp8_predict_recon(mbcols, mbrows, n, modes.ctypes.data, dm.ptr, dr.ptr, residual.shape[1] * 384,
                                         dmap.ptr if dmap else None, dy.ptr, du.ptr, dv.ptr, ysz, csz, None),
               "ffhip_vp8_predict_recon")
    return (dy.to_host((n, 16 * mbrows, 16 * mbcols), np.uint8), du.to_host((n, 8 * mbrows, 8 * mbcols), np.uint8),
            dv.to_host((n, 8 * mbrows, 8 * mbcols), np.uint8))


last_sync_status = 0     # what the stream sync of the last vp8_predict_loopfilter / vp8_decode_frames call returned (0 or capi.FFHIP_RETRIED)


def vp8_predict_loopfilter(mbcols, mbrows, modes, residual, filter_type, filters, resmap=None):
    """ffhip_vp8_predict_loopfilter: prediction + reconstruction and the loop filter of whole key frames as one call
    (format/webp.c:1833-1866), the two row kernels side by side.  Arguments as vp8_predict_recon / vp8_loopfilter;
    returns the filtered planes (Y [n][16r][16c], U, V)."""
    L = capi.require_device()
    n, n_mb = modes.shape[0], mbcols * mbrows
    assert modes.shape == (n, n_mb, 20) and residual.shape[0] == n and residual.shape[2] == 384
    modes = np.ascontiguousarray(modes)
    dm, dr, df = DeviceBuffer(modes), DeviceBuffer(np.ascontiguousarray(residual)), DeviceBuffer(np.ascontiguousarray(filters))
    dmap = DeviceBuffer(np.ascontiguousarray(resmap, dtype=np.int32)) if resmap is not None else None
    ysz, csz = 256 * n_mb, 64 * n_mb
    dy, du, dv = DeviceBuffer(nbytes=n * ysz), DeviceBuffer(nbytes=n * csz), DeviceBuffer(nbytes=n * csz)
    for d in (dy, du, dv):
        capi.check(L.ffhip_memset(d.ptr, 0, d.nbytes, None))
    capi.check(L.ffhip_vp8_predict_loopfilter(mbcols, mbrows, n, modes.ctypes.data, dm.ptr, dr.ptr, residual.shape[1] * 384,
                                              dmap.ptr if dmap else None, filter_type, df.ptr, dy.ptr, du.ptr, dv.ptr, ysz, csz, None),
               "ffhip_vp8_predict_loopfilter")
    global last_sync_status
    last_sync_status = capi.sync(None)
    return (dy.to_host((n, 16 * mbrows, 16 * mbcols), np.uint8), du.to_host((n, 8 * mbrows, 8 * mbcols), np.uint8),
            dv.to_host((n, 8 * mbrows, 8 * mbcols), np.uint8))


def vp8_decode_frames(mbcols, mbrows, modes, residual, filter_type, filters, resmap=None, planes=False, pitch=None, host_modes=True):
    """ffhip_vp8_decode_frames: the frame loop of vp8_decode (format/webp.c:1833-1868) for a batch -- prediction, loop filter and
    colour conversion as one call.  Returns BGRA uint8 [n][16r][pitch] and, with planes=True, the filtered (Y, U, V) too."""
    L = capi.require_device()
    n, n_mb = modes.shape[0], mbcols * mbrows
    assert modes.shape == (n, n_mb, 20) and residual.shape[0] == n and residual.shape[2] == 384
    modes = np.ascontiguousarray(modes)
    dm, dr = DeviceBuffer(modes), DeviceBuffer(np.ascontiguousarray(residual))
    df = DeviceBuffer(np.ascontiguousarray(filters)) if filters is not None else None
    dmap = DeviceBuffer(np.ascontiguousarray(resmap, dtype=np.int32)) if resmap is not None else None
    H, W = 16 * mbrows, 16 * mbcols
    pitch = pitch or W * 4
    do = DeviceBuffer(nbytes=n * H * pitch)
    capi.check(L.ffhip_memset(do.ptr, 0, do.nbytes, None))
    ysz, csz = 256 * n_mb, 64 * n_mb
    dy = du = dv = None
    if planes:
        dy, du, dv = DeviceBuffer(nbytes=n * ysz), DeviceBuffer(nbytes=n * csz), DeviceBuffer(nbytes=n * csz)
        for d in (dy, du, dv):
            capi.check(L.ffhip_memset(d.ptr, 0, d.nbytes, None))
    capi.check(L.ffhip_vp8_decode_frames(mbcols, mbrows, n, modes.ctypes.data if host_modes else None, dm.ptr, dr.ptr, residual.shape[1] * 384,
                                         dmap.ptr if dmap else None, filter_type, df.ptr if df else None, do.ptr, pitch, H * pitch,
                                         dy.ptr if planes else None, du.ptr if planes else None, dv.ptr if planes else None, ysz, csz, None),
               "ffhip_vp8_decode_frames")
    global last_sync_status
    last_sync_status = capi.sync(None)
    bgra = do.to_host((n, H, pitch), np.uint8)
    if not planes:
        return bgra
    return bgra, (dy.to_host((n, H, W), np.uint8), du.to_host((n, H // 2, W // 2), np.uint8), dv.to_host((n, H // 2, W // 2), np.uint8))


def hevc_decode_tiles(tus, residual, width, height, tile_first=None, bd=8, pitch=None):
    """ffhip_hevc_decode_tiles on a 4:2:0 plane set: intra reconstruction of the (concatenated) TU lists and the colour conversion as one call.
    Returns (bgra uint8 [height][pitch], (Y, U, V) int16 planes)."""
    L = capi.require_device()
    tus = np.ascontiguousarray(tus)
    dt, dr = DeviceBuffer(tus.view(np.uint8)), DeviceBuffer(np.ascontiguousarray(residual))
    cw, ch = width // 2, height // 2
    dy, du, dv = DeviceBuffer(nbytes=width * height * 2), DeviceBuffer(nbytes=cw * ch * 2), DeviceBuffer(nbytes=cw * ch * 2)
    pitch = pitch or width * 4
    do = DeviceBuffer(nbytes=height * pitch)
    for d in (dy, du, dv, do):
        capi.check(L.ffhip_memset(d.ptr, 0, d.nbytes, None))
    tf = np.ascontiguousarray(tile_first if tile_first is not None else [0], dtype=np.int64)
    capi.check(L.ffhip_hevc_decode_tiles(tus.ctypes.data, dt.ptr, len(tus), tf.ctypes.data, len(tf), dr.ptr, dy.ptr, du.ptr, dv.ptr, width, height, width, cw, ch, cw, bd, bd,
                                         do.ptr, pitch, None), "ffhip_hevc_decode_tiles")
    capi.check(L.ffhip_stream_sync(None), "ffhip_stream_sync")
    return do.to_host((height, pitch), np.uint8), (dy.to_host((height, width), np.int16), du.to_host((ch, cw), np.int16), dv.to_host((ch, cw), np.int16))


def hevc_intra_recon(tus, residual, width, height, chroma=True, bd_y=8, bd_c=8, csub=2):
    """decode_intra_block steps 5-10 (coding/hevc.c:4730-4790) for a TU list in decode order
    (structured array of dtype synth.HEVC_TU_DTYPE == struct ffhip_hevc_tu); planes start at 0;
    csub = chroma subsampling divisor (2 for 4:2:0, 1 for 4:4:4)."""
    L = capi.require_device()
    tus = np.ascontiguousarray(tus)
    assert tus.dtype.itemsize == 32
    dt, dr = DeviceBuffer(tus.view(np.uint8)), DeviceBuffer(np.ascontiguousarray(residual))
    cw, ch = (width // csub, height // csub) if chroma else (0, 0)
    dy = DeviceBuffer(nbytes=width * height * 2)
    du = DeviceBuffer(nbytes=max(cw * ch * 2, 16))
    dv = DeviceBuffer(nbytes=max(cw * ch * 2, 16))
    for d in (dy, du, dv):
        capi.check(L.ffhip_memset(d.ptr, 0, d.nbytes, None))
    capi.check(L.ffhip_hevc_intra_recon(tus.ctypes.data, dt.ptr, len(tus), dr.ptr, dy.ptr, du.ptr if chroma else None,
                                        dv.ptr if chroma else None, width, height, width, cw, ch, cw, bd_y, bd_c, None),
               "ffhip_hevc_intra_recon")
    if chroma:
        return dy.to_host((height, width), np.int16), du.to_host((ch, cw), np.int16), dv.to_host((ch, cw), np.int16)
    return dy.to_host((height, width), np.int16), None, None


def file_args(files):
    """files (a list of bytes) as the batch calls take them: (the arrays that keep the bytes in place, const uint8_t *const *files,
    const size_t *lens)"""
    n = max(len(files), 1)
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    return bufs, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs])


def _files_to_pictures(files, probe, call, what, strict, own_failure=lambda rc: rc not in (0, capi.FFHIP_EINVAL)):
    """Pictures of any sizes into ONE device allocation, each at a 16-byte-aligned offset, and back to the host.
      probe(i, f) -> (pitch, rows, crop_w, crop_h) of file i's picture; capi.FfhipError for a file without one
      call(L, ptrs, lens, n, outs, pitches, status) -> the batch call's return
      strict: any failure raises; otherwise only one that own_failure(rc) says is the call's and no file's
    Returns ([host BGRA [crop_h][crop_w][4], None for a failing file], device buffer, per-file status codes)."""
    L = capi.require_device()
    n = len(files)
    places, offs, total = [], [], 0
    for i, f in enumerate(files):
        try:
            place = probe(i, f)
        except capi.FfhipError:
            place = (0, 0, 0, 0)
        places.append(place)
        offs.append(total)
        total += (place[0] * place[1] + 15) & ~15
    dout = DeviceBuffer(nbytes=max(total, 16))
    bufs, ptrs, lens = file_args(files)
    outs = (C.c_void_p * n)(*[dout.ptr + o for o in offs])
    status = (C.c_int * n)()
    rc = call(L, ptrs, lens, n, outs, (C.c_int64 * n)(*[p[0] for p in places]), status)
    if strict or own_failure(rc):
        capi.check(rc, what)
    flat = dout.to_host((max(total, 16),), np.uint8)
    images = []
    for (pitch, rows, w, h), off, code in zip(places, offs, status):
        if code or not pitch:
            images.append(None)
            continue
        images.append(flat[off:off + pitch * rows].reshape(rows, pitch // 4, 4)[:h, :w].copy())
    return images, dout, list(status)


def jpeg_probe(data):
    """Geometry of a baseline JPEG file (bytes) -> (JpegGeom, width, height)."""
    L = capi.lib()
    g, w, h = capi.JpegGeom(), C.c_int(), C.c_int()
    buf = np.frombuffer(data, dtype=np.uint8)
    capi.check(L.ffhip_jpeg_probe(buf.ctypes.data, buf.size, C.byref(g), C.byref(w), C.byref(h)), "ffhip_jpeg_probe")
    return g, w.value, h.value


def jpeg_probe_any(data):
    """ffhip_jpeg_probe_any: geometry of a baseline OR progressive JPEG file (bytes) -> (JpegGeom, width, height, progressive)."""
    L = capi.lib()
    g, w, h, pg = capi.JpegGeom(), C.c_int(), C.c_int(), C.c_int()
    buf = np.frombuffer(data, dtype=np.uint8)
    capi.check(L.ffhip_jpeg_probe_any(buf.ctypes.data if buf.size else None, buf.size, C.byref(g), C.byref(w), C.byref(h), C.byref(pg)),
               "ffhip_jpeg_probe_any")
    return g, w.value, h.value, bool(pg.value)


def jpeg_progressive_decode(data, k_max=63):
    """ffhip_jpeg_progressive_decode: the host decoder of progressive files (T.81 Annex G).  Returns (geom, cy, cu, cv, quant[4][64]) in the
    layout of jpeg_entropy_batch for one file; scans with Ss > k_max are skipped and their coefficients read as zero.  No device."""
    L = capi.lib()
    g, _, _, _ = jpeg_probe_any(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    cy = np.empty(g.y_blocks * 64, np.int16)
    cu = np.empty(g.c_blocks * 64, np.int16) if g.ncomp == 3 else None
    cv = np.empty(g.c_blocks * 64, np.int16) if g.ncomp == 3 else None
    quant = np.empty((4, 64), np.uint16)
    capi.check(L.ffhip_jpeg_progressive_decode(buf.ctypes.data, buf.size, C.byref(g), _vp(cy), _vp(cu), _vp(cv), _vp(quant), k_max),
               "ffhip_jpeg_progressive_decode")
    return g, cy, cu, cv, quant


def jpeg_progressive_batch_gpu(files, k_max=63, n_threads=4, strict=True):
    """ffhip_jpeg_progressive_batch_gpu on progressive files of one geometry; planes come back to the host for inspection.  Returns
    (geom, cy, cu, cv, quant[n][4][64]) like jpeg_entropy_batch_gpu; with strict=False a failing file does not raise and the per-file
    status codes follow."""
    L = capi.require_device()
    g, _, _, _ = jpeg_probe_any(files[0])
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    dy = DeviceBuffer(nbytes=n * g.y_blocks * 128)
    du = DeviceBuffer(nbytes=max(n * g.c_blocks * 128, 16)) if g.ncomp == 3 else None
    dv = DeviceBuffer(nbytes=max(n * g.c_blocks * 128, 16)) if g.ncomp == 3 else None
    dq = DeviceBuffer(nbytes=n * 512)
    status = (C.c_int * n)()
    rc = L.ffhip_jpeg_progressive_batch_gpu(ptrs, lens, n, n_threads, C.byref(g), dy.ptr, du.ptr if du else None, dv.ptr if dv else None, dq.ptr,
                                            k_max, status, None)
    if strict or rc not in (0, capi.FFHIP_EINVAL):
        capi.check(rc, "ffhip_jpeg_progressive_batch_gpu")
    cy = dy.to_host((n * g.y_blocks * 64,), np.int16)
    cu = du.to_host((n * g.c_blocks * 64,), np.int16) if du else None
    cv = dv.to_host((n * g.c_blocks * 64,), np.int16) if dv else None
    out = (g, cy, cu, cv, dq.to_host((n, 4, 64), np.uint16))
    return out if strict else out + (list(status),)


def progressive_last():
    """ffhip_debug_progressive_last: (progressive files, scans decoded, scans skipped, levels launched, front end: 0 host, 1 device) of the
    calling thread's last progressive call."""
    out = (C.c_int * 5)()
    capi.check(capi.lib().ffhip_debug_progressive_last(out), "ffhip_debug_progressive_last")
    return tuple(out)


def jpeg_entropy_batch(files, n_threads=4):
    """Host-side Huffman decode of same-geometry JPEG files (list of bytes) into the planes the
    reconstruction reads (format/jpg.c:255-415, 588-655).  Returns (geom, cy, cu, cv, quant[n][4][64])."""
    L = capi.lib()
    g, _, _ = jpeg_probe(files[0])
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    cy = np.empty(n * g.y_blocks * 64, np.int16)
    cu = np.empty(n * g.c_blocks * 64, np.int16) if g.ncomp == 3 else None
    cv = np.empty(n * g.c_blocks * 64, np.int16) if g.ncomp == 3 else None
    quant = np.empty((n, 4, 64), np.uint16)
    status = (C.c_int * n)()
    capi.check(L.ffhip_jpeg_entropy_batch(ptrs, lens, n, n_threads, C.byref(g), _vp(cy), _vp(cu), _vp(cv), _vp(quant), status),
               "ffhip_jpeg_entropy_batch")
    return g, cy, cu, cv, quant


def decode_jpeg_files(files, n_threads=4):
    """transbmp-equivalent core: files -> BGRA [n][H][W][4] (coded size), entropy on the host
    threads, reconstruction on the GPU."""
    g, cy, cu, cv, quant = jpeg_entropy_batch(files, n_threads)
    return g, jpeg_recon_batch_host(g, len(files), cy, cu, cv, quant)


def vp8_loopfilter(mbcols, mbrows, filter_type, modes, filters, y, u, v):
    """loopfilter over whole key frames (format/webp.c:1686-1752, 1856-1866); planes uint8
    [n][H][W] are filtered and returned."""
    L = capi.require_device()
    n = modes.shape[0]
    dm, df = DeviceBuffer(np.ascontiguousarray(modes)), DeviceBuffer(np.ascontiguousarray(filters))
    dy, du, dv = DeviceBuffer(np.ascontiguousarray(y)), DeviceBuffer(np.ascontiguousarray(u)), DeviceBuffer(np.ascontiguousarray(v))
    n_mb = mbcols * mbrows
    capi.check(L.ffhip_vp8_loopfilter(mbcols, mbrows, n, filter_type, dm.ptr, df.ptr, dy.ptr, du.ptr, dv.ptr,
                                      256 * n_mb, 64 * n_mb, None), "ffhip_vp8_loopfilter")
    return dy.to_host(y.shape, np.uint8), du.to_host(u.shape, np.uint8), dv.to_host(v.shape, np.uint8)


def heif_grid_parse(item):
    """ImageGrid item payload (bytes) -> capi.HeifGrid, as decode_grid_items reads it (format/heif.c:273-298)."""
    L = capi.lib()
    g = capi.HeifGrid()
    buf = (C.c_uint8 * len(item)).from_buffer_copy(bytes(item))
    capi.check(L.ffhip_heif_grid_parse(C.cast(buf, C.c_void_p), len(item), C.byref(g)), "ffhip_heif_grid_parse")
    return g


def heif_grid_compose(tiles, cols, out_w, out_h):
    """tiles uint8 [rows*cols][tile_h][tile_w][4] (row-major `dimg` order) -> canvas [out_h][out_w][4]."""
    L = capi.require_device()
    tiles = np.ascontiguousarray(tiles)
    n, th, tw, _ = tiles.shape
    dt = DeviceBuffer(tiles)
    dc = DeviceBuffer(nbytes=out_w * out_h * 4)
    capi.check(L.ffhip_heif_grid_compose(dc.ptr, out_w * 4, out_w, out_h, dt.ptr, tw * 4, tw * th * 4, tw, th, n // cols, cols,
                                         None), "ffhip_heif_grid_compose")
    return dc.to_host((out_h, out_w, 4), np.uint8)


class PinnedArray:
    """numpy view of pinned host memory (ffhip_host_malloc); keep the object alive while the view is used."""

    def __init__(self, shape, dtype=np.uint8):
        L = capi.require_device()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = L.ffhip_host_malloc(self.nbytes)
        if not self.ptr:
            raise capi.FfhipError("ffhip_host_malloc failed")
        self.array = np.frombuffer((C.c_uint8 * self.nbytes).from_address(self.ptr), dtype=dtype).reshape(shape)

    def __del__(self):
        try:
            capi.lib().ffhip_host_free(self.ptr)
        except Exception:
            pass


def jpeg_decode_files(files, n_threads=8, chunk=0, out=None):
    """ffhip_jpeg_decode_files: same-geometry baseline JPEG files (list of bytes) -> (geom, BGRA [n][H][W][4] at the
    coded size), entropy decode on host threads overlapped with copy + reconstruction on the GPU.  `out`: a
    preallocated uint8 array [n][H][W][4] (e.g. PinnedArray(...).array, which takes the device copy directly)."""
    L = capi.require_device()
    g, _, _ = jpeg_probe(files[0])
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    if out is None:
        out = np.empty((n, g.height, g.width, 4), np.uint8)
    assert out.shape == (n, g.height, g.width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
    status = (C.c_int * n)()
    g2 = capi.JpegGeom()
    capi.check(L.ffhip_jpeg_decode_files(ptrs, lens, n, n_threads, chunk, C.byref(g2), out.ctypes.data, g.width * 4,
                                         g.width * 4 * g.height, status), "ffhip_jpeg_decode_files")
    return g2, out


def jpeg_entropy_batch_gpu(files, n_threads=4):
    """ffhip_jpeg_entropy_batch_gpu on files with restart markers; planes come back to the host for inspection.
    Returns (geom, cy, cu, cv, quant[n][4][64]) like jpeg_entropy_batch."""
    L = capi.require_device()
    g, _, _ = jpeg_probe(files[0])
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    dy = DeviceBuffer(nbytes=n * g.y_blocks * 128)
    du = DeviceBuffer(nbytes=max(n * g.c_blocks * 128, 16)) if g.ncomp == 3 else None
    dv = DeviceBuffer(nbytes=max(n * g.c_blocks * 128, 16)) if g.ncomp == 3 else None
    dq = DeviceBuffer(nbytes=n * 512)
    status = (C.c_int * n)()
    capi.check(L.ffhip_jpeg_entropy_batch_gpu(ptrs, lens, n, n_threads, C.byref(g), dy.ptr, du.ptr if du else None, dv.ptr if dv else None, dq.ptr,
                                              status, None), "ffhip_jpeg_entropy_batch_gpu")
    cy = dy.to_host((n * g.y_blocks * 64,), np.int16)
    cu = du.to_host((n * g.c_blocks * 64,), np.int16) if du else None
    cv = dv.to_host((n * g.c_blocks * 64,), np.int16) if dv else None
    return g, cy, cu, cv, dq.to_host((n, 4, 64), np.uint16)


def jpeg_decode_files_device(files, n_threads=8):
    """ffhip_jpeg_decode_files_device: files -> BGRA left in device memory; returned here as a host copy for checks,
    together with the DeviceBuffer that holds it: (geom, host array [n][H][W][4], device buffer)."""
    L = capi.require_device()
    g, _, _ = jpeg_probe(files[0])
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    dout = DeviceBuffer(nbytes=n * g.width * g.height * 4)
    status = (C.c_int * n)()
    g2 = capi.JpegGeom()
    capi.check(L.ffhip_jpeg_decode_files_device(ptrs, lens, n, n_threads, C.byref(g2), dout.ptr, g.width * 4, g.width * 4 * g.height,
                                                status, None), "ffhip_jpeg_decode_files_device")
    return g2, dout.to_host((n, g.height, g.width, 4), np.uint8), dout


def jpeg_recon_items(items, stream=None):
    """ffhip_jpeg_recon_items: `items` a list of capi.JpegItem (device pointers); pictures of any fused layout and size in
    one call, one launch per layout class.  Only enqueues on `stream`."""
    L = capi.lib()
    n = len(items)
    arr = (capi.JpegItem * max(n, 1))(*items)
    capi.check(L.ffhip_jpeg_recon_items(arr, n, stream), "ffhip_jpeg_recon_items")


def jpeg_scaled_block(coef, quant, denom):
    """ffhip_jpeg_scaled_block: the N x N samples (N = 8 / denom, denom 2, 4 or 8) of one block from its 64 coefficients and 64 quantisers
    (natural order), by the reduced-size rule the kernel runs.  Needs no device."""
    coef = np.ascontiguousarray(coef, np.int16).reshape(64)
    quant = np.ascontiguousarray(quant, np.uint16).reshape(64)
    n = 8 // denom if denom in (1, 2, 4, 8) else 1
    out = np.zeros((n, n), np.int16)
    capi.check(capi.lib().ffhip_jpeg_scaled_block(_vp(coef), _vp(quant), denom, _vp(out)), "ffhip_jpeg_scaled_block")
    return out


def jpeg_scaled_size(width, height, denom):
    """ffhip_jpeg_scaled_size: (width, height) a width x height picture displays at 1 / denom."""
    w, h = C.c_int(), C.c_int()
    capi.check(capi.lib().ffhip_jpeg_scaled_size(width, height, denom, C.byref(w), C.byref(h)), "ffhip_jpeg_scaled_size")
    return w.value, h.value


def jpeg_scaled_rect(width, height, denom, roi):
    """ffhip_jpeg_scaled_rect: the rectangle (x0, y0, w, h) of the full-size width x height display picture mapped onto the picture at 1 / denom."""
    r, out = capi.Rect(*[int(v) for v in roi]), capi.Rect()
    capi.check(capi.lib().ffhip_jpeg_scaled_rect(width, height, denom, C.byref(r), C.byref(out)), "ffhip_jpeg_scaled_rect")
    return out.x0, out.y0, out.width, out.height


def jpeg_scale_choose(rect_w, rect_h, out_w, out_h):
    """ffhip_jpeg_scale_choose: the largest denominator in 8, 4, 2, 1 at which a rect_w x rect_h rectangle still covers out_w x out_h."""
    d = capi.lib().ffhip_jpeg_scale_choose(rect_w, rect_h, out_w, out_h)
    capi.check(min(d, 0), "ffhip_jpeg_scale_choose")
    return d


def jpeg_recon_items_scaled(items, denom, stream=None):
    """ffhip_jpeg_recon_items_scaled: `items` a list of capi.JpegItem whose d_bgra / pitch describe the picture at 1 / denom[i]; one launch
    per denominator present, denominator 1 through ffhip_jpeg_recon_items.  Only enqueues on `stream`."""
    L = capi.lib()
    n = len(items)
    arr = (capi.JpegItem * max(n, 1))(*items)
    den = (C.c_int * max(n, 1))(*[int(d) for d in denom])
    capi.check(L.ffhip_jpeg_recon_items_scaled(arr, den, n, stream), "ffhip_jpeg_recon_items_scaled")


def jpeg_libjpeg_block(coef, quant):
    """ffhip_jpeg_libjpeg_block: the 8 x 8 samples (uint8) libjpeg makes of one block's 64 coefficients and 64 quantisers (natural order):
    int32 dequantisation, the islow inverse DCT, + 128, clamped.  Needs no device."""
    coef = np.ascontiguousarray(coef, np.int16).reshape(64)
    quant = np.ascontiguousarray(quant, np.uint16).reshape(64)
    out = np.zeros((8, 8), np.uint8)
    capi.check(capi.lib().ffhip_jpeg_libjpeg_block(_vp(coef), _vp(quant), _vp(out)), "ffhip_jpeg_libjpeg_block")
    return out


def jpeg_libjpeg_picture(geom, width, height, coef_y, coef_u, coef_v, quant):
    """ffhip_jpeg_libjpeg_picture: the width x height display picture libjpeg makes of host planes (layout of jpeg_recon_batch_host, one
    picture; quant uint16 [4][64]) -> BGRA [height][width][4].  The CPU model of jpeg_recon_items_libjpeg.  Needs no device."""
    cy = np.ascontiguousarray(coef_y, np.int16)
    cu = None if coef_u is None else np.ascontiguousarray(coef_u, np.int16)
    cv = None if coef_v is None else np.ascontiguousarray(coef_v, np.int16)
    q = np.ascontiguousarray(quant, np.uint16)
    out = np.zeros((max(int(height), 1), max(int(width), 1), 4), np.uint8)
    capi.check(capi.lib().ffhip_jpeg_libjpeg_picture(C.byref(geom), width, height, _vp(cy), None if cu is None else _vp(cu),
                                                     None if cv is None else _vp(cv), _vp(q), _vp(out), out.shape[1] * 4),
               "ffhip_jpeg_libjpeg_picture")
    return out


def jpeg_recon_items_libjpeg(items, display, stream=None):
    """ffhip_jpeg_recon_items_libjpeg: `items` a list of capi.JpegItem (device pointers), display[i] = (width, height) of item i's display
    picture; libjpeg's pixels for pictures of any fused layout and size in one pair of launches.  Only enqueues on `stream`."""
    L = capi.lib()
    n = len(items)
    arr = (capi.JpegItem * max(n, 1))(*items)
    shown = (capi.Size * max(n, 1))(*[capi.Size(int(w), int(h)) for w, h in display])
    capi.check(L.ffhip_jpeg_recon_items_libjpeg(arr, shown, n, stream), "ffhip_jpeg_recon_items_libjpeg")


def jpeg_decode_files_mixed_device_scaled(files, denom, n_threads=8, stream=None, strict=True):
    """ffhip_jpeg_decode_files_mixed_device_scaled: as jpeg_decode_files_mixed_device with file i at 1 / denom[i] of its size.  Returns (geoms,
    [host BGRA [h][w][4] at the SCALED CODED size], device buffer); with strict=False a failing file's entry is None and the per-file status
    codes follow."""
    def probe(i, f):
        g, _, _ = jpeg_probe(f)
        return (g.width // denom[i] * 4 + 15) & ~15, g.height // denom[i], g.width // denom[i], g.height // denom[i]

    geoms = (capi.JpegGeom * len(files))()
    den = (C.c_int * len(files))(*[int(d) for d in denom])
    images, dout, status = _files_to_pictures(
        files, probe, lambda L, ptrs, lens, n, outs, pitches, status: L.ffhip_jpeg_decode_files_mixed_device_scaled(
            ptrs, lens, n, n_threads, outs, pitches, den, geoms, status, stream), "ffhip_jpeg_decode_files_mixed_device_scaled", strict)
    return (list(geoms), images, dout) if strict else (list(geoms), images, dout, status)


def tensor_last_parts():
    """ffhip_debug_tensor_last_parts: the parts the calling thread's last files-to-tensors call cut its batch into."""
    return capi.lib().ffhip_debug_tensor_last_parts()


def orient_last_items():
    """ffhip_debug_orient_last_items: the pictures the calling thread's last ffhip_*_decode_files_tensor* call turned upright"""
    return capi.lib().ffhip_debug_orient_last_items()


def _exif_orientation(call, data):
    buf = np.frombuffer(data, dtype=np.uint8)
    o = C.c_int(0)
    capi.check(call(buf.ctypes.data if buf.size else None, buf.size, C.byref(o)), "ffhip_*_exif_orientation")
    return o.value


def jpeg_exif_orientation(data):
    """ffhip_jpeg_exif_orientation: the EXIF orientation (1..8) of a JPEG file's bytes; 1 where the file has no usable tag.  No device."""
    return _exif_orientation(capi.lib().ffhip_jpeg_exif_orientation, data)


def webp_exif_orientation(data):
    """ffhip_webp_exif_orientation: the same from a WebP file's EXIF chunk"""
    return _exif_orientation(capi.lib().ffhip_webp_exif_orientation, data)


def orient_size(width, height, orientation):
    """ffhip_orient_size: (width, height) of the upright picture of a stored width x height one"""
    w, h = C.c_int(), C.c_int()
    capi.check(capi.lib().ffhip_orient_size(width, height, orientation, C.byref(w), C.byref(h)), "ffhip_orient_size")
    return w.value, h.value


def orient_rect(width, height, orientation, roi):
    """ffhip_orient_rect: the rectangle (x0, y0, w, h) of the upright picture as a rectangle of the stored width x height picture"""
    out = capi.Rect()
    capi.check(capi.lib().ffhip_orient_rect(width, height, orientation, C.byref(capi.Rect(*roi)), C.byref(out)), "ffhip_orient_rect")
    return out.x0, out.y0, out.width, out.height


def orient_inverse(orientation):
    """ffhip_orient_inverse: the orientation that undoes `orientation`"""
    o = capi.lib().ffhip_orient_inverse(orientation)
    capi.check(min(o, 0), "ffhip_orient_inverse")
    return o


def vp8_decode_items(items, stream=None):
    """ffhip_vp8_decode_items: `items` a list of capi.Vp8Item; key frames of any size, quantisers and loop filter in one call
    (one launch per filter type and residual-map form).  Only enqueues on `stream`."""
    L = capi.lib()
    n = len(items)
    arr = (capi.Vp8Item * max(n, 1))(*items)
    capi.check(L.ffhip_vp8_decode_items(arr, n, stream), "ffhip_vp8_decode_items")


def jpeg_decode_files_mixed_device(files, n_threads=8, stream=None, strict=True, crop=True, progressive=False, pixels="reference"):
    """ffhip_jpeg_decode_files_mixed_device: baseline JPEG files of any geometry (list of bytes) in one call.  Every picture
    gets its place in ONE device allocation, at a 16-byte-aligned offset with the pitch 4 x its coded width.  Returns
    (geoms, [host BGRA [h][w][4] cropped to each file's display size (crop=False: the coded size)], device buffer); with
    strict=False a failing file does not raise: its entry is None and a fourth element, the per-file status codes, follows.
    progressive=True: ffhip_jpeg_decode_files_mixed_device_ex with FFHIP_JPEG_ACCEPT_PROGRESSIVE -- progressive files are probed
    (jpeg_probe_any) and decoded too; False, the default, refuses them as ever.
    pixels='libjpeg': the same call with FFHIP_JPEG_PIXELS_LIBJPEG -- libjpeg's pixels (PIL's, torchvision's) instead of the reference's;
    any value but 'reference' and 'libjpeg' is a ValueError."""
    if pixels not in ("reference", "libjpeg"):
        raise ValueError(f"pixels {pixels!r}: 'reference' or 'libjpeg'")
    flags = (capi.FFHIP_JPEG_ACCEPT_PROGRESSIVE if progressive else 0) | (capi.FFHIP_JPEG_PIXELS_LIBJPEG if pixels == "libjpeg" else 0)
    def probe(i, f):
        g, w, h = jpeg_probe_any(f)[:3] if progressive else jpeg_probe(f)
        return (g.width * 4, g.height, w, h) if crop else (g.width * 4, g.height, g.width, g.height)

    geoms = (capi.JpegGeom * len(files))()

    def call(L, ptrs, lens, n, outs, pitches, status):
        if flags:
            return L.ffhip_jpeg_decode_files_mixed_device_ex(ptrs, lens, n, n_threads, outs, pitches, None, flags, geoms, status, stream)
        return L.ffhip_jpeg_decode_files_mixed_device(ptrs, lens, n, n_threads, outs, pitches, geoms, status, stream)

    images, dout, status = _files_to_pictures(files, probe, call, "ffhip_jpeg_decode_files_mixed_device", strict)
    return (list(geoms), images, dout) if strict else (list(geoms), images, dout, status)


def vp8_dequant_factors(y_ac_qi, deltas=(0, 0, 0, 0, 0), segmentation_enabled=0, update_mb_segmentation_map=1, updates=(0, 0, 0, 0)):
    """ffhip_vp8_dequant_factors (read_dequantization, format/webp.c:458-548): uint16 [4][8].  deltas = y_dc, y2_dc, y2_ac, uv_dc, uv_ac."""
    L = capi.lib()
    h = capi.Vp8QuantHeader()
    h.y_ac_qi = y_ac_qi
    h.y_dc_delta, h.y2_dc_delta, h.y2_ac_delta, h.uv_dc_delta, h.uv_ac_delta = [int(d) for d in deltas]
    h.segmentation_enabled, h.update_mb_segmentation_map = segmentation_enabled, update_mb_segmentation_map
    for i in range(4):
        h.quantizer_update_value[i] = int(updates[i])
    out = np.zeros((4, 8), np.uint16)
    capi.check(L.ffhip_vp8_dequant_factors(C.byref(h), out.ctypes.data), "ffhip_vp8_dequant_factors")
    return out


def webp_pixel_flags(pixels):
    """pixels 'reference' | 'libwebp' -> the flags of the ffhip_webp_*_ex calls; anything else is a ValueError"""
    if pixels not in ("reference", "libwebp"):
        raise ValueError(f"pixels {pixels!r}: 'reference' or 'libwebp'")
    return capi.FFHIP_WEBP_PIXELS_LIBWEBP if pixels == "libwebp" else 0


def webp_probe(data, pixels="reference"):
    """ffhip_webp_probe: (width, height, mbcols, mbrows) of a lossy WebP file (bytes); the picture ffhip_webp_decode_files_device
    writes is 16*mbcols x 16*mbrows, width x height of it is what the reference's loader reports.
    pixels='libwebp' (ffhip_webp_probe_ex with FFHIP_WEBP_PIXELS_LIBWEBP): the frame tag's width and height, and the macroblock grid of those."""
    flags = webp_pixel_flags(pixels)
    L = capi.lib()
    v = [C.c_int() for _ in range(4)]
    buf = np.frombuffer(data, dtype=np.uint8)
    if flags:
        capi.check(L.ffhip_webp_probe_ex(buf.ctypes.data, buf.size, flags, *[C.byref(x) for x in v]), "ffhip_webp_probe_ex")
    else:
        capi.check(L.ffhip_webp_probe(buf.ctypes.data, buf.size, *[C.byref(x) for x in v]), "ffhip_webp_probe")
    return tuple(x.value for x in v)


def _webp_parsed(n_mb):
    arrs = dict(modes=np.zeros((n_mb, 20), np.uint8), levels=np.zeros((n_mb, 25, 16), np.int16), mbinfo=np.zeros((n_mb, 32), np.uint8),
                resmap=np.zeros(n_mb, np.int32))
    p = capi.WebpParsed()
    p.modes, p.levels, p.mbinfo, p.resmap = [arrs[k].ctypes.data for k in ("modes", "levels", "mbinfo", "resmap")]
    p.n_mb_cap = n_mb
    return p, arrs


def _webp_result(p, arrs):
    i = p.info
    arrs.update(width=i.width, height=i.height, mbcols=i.mbcols, mbrows=i.mbrows, filter_type=i.filter_type, nbr_partitions=i.nbr_partitions,
                quant=np.ctypeslib.as_array(i.quant).reshape(4, 8).copy(), filters=np.ctypeslib.as_array(i.filters).reshape(4, 2, 3).copy(),
                info=i)
    return arrs


def webp_parse(data, pixels="reference"):
    """ffhip_webp_parse on the host: dict of modes [n_mb][20], levels [n_mb][25][16], mbinfo [n_mb][32], resmap [n_mb], quant [4][8],
    filters [4][2][3], filter_type, the sizes and the header (`info`, a capi.WebpInfo).  pixels='libwebp': ffhip_webp_parse_ex under that
    rule (RFC 6386 as libwebp parses it: tests/vp8_spec.py is the witness)."""
    flags = webp_pixel_flags(pixels)
    L = capi.lib()
    _, _, c, r = webp_probe(data, pixels)
    p, arrs = _webp_parsed(c * r)
    buf = np.frombuffer(data, dtype=np.uint8)
    if flags:
        capi.check(L.ffhip_webp_parse_ex(buf.ctypes.data, buf.size, flags, C.byref(p)), "ffhip_webp_parse_ex")
    else:
        capi.check(L.ffhip_webp_parse(buf.ctypes.data, buf.size, C.byref(p)), "ffhip_webp_parse")
    return _webp_result(p, arrs)


def _webp_parse_many(files, call, pixels="reference"):
    n = len(files)
    bufs, ptrs, lens = file_args(files)
    outs = (capi.WebpParsed * n)()
    keep = []
    for i, f in enumerate(files):
        try:
            _, _, c, r = webp_probe(f, pixels)
        except capi.FfhipError:
            c = r = 0
        p, arrs = _webp_parsed(max(c * r, 1))
        outs[i] = p
        keep.append(arrs)
    status = (C.c_int * n)()
    rc = call(ptrs, lens, n, outs, status)
    if rc not in (0, capi.FFHIP_EINVAL) and rc > -1000:
        capi.check(rc, "webp parse")
    return [None if status[i] else _webp_result(outs[i], keep[i]) for i in range(n)], list(status)


def webp_parse_batch(files, n_threads=4):
    """ffhip_webp_parse_batch: (list of webp_parse dicts, None for a failing file; status codes)."""
    L = capi.lib()
    return _webp_parse_many(files, lambda ptrs, lens, n, outs, status: L.ffhip_webp_parse_batch(ptrs, lens, n, n_threads, outs, status))


def webp_parse_device(files, stream=None, pixels="reference"):
    """ffhip_webp_parse_device: the same arrays from the two device kernels (no host fall-back), for comparing the halves.
    pixels='libwebp': ffhip_webp_parse_device_ex, the kernels' instances under that rule."""
    flags = webp_pixel_flags(pixels)
    L = capi.require_device()
    if flags:
        return _webp_parse_many(files, lambda ptrs, lens, n, outs, status: L.ffhip_webp_parse_device_ex(ptrs, lens, n, flags, outs, status, stream), pixels)
    return _webp_parse_many(files, lambda ptrs, lens, n, outs, status: L.ffhip_webp_parse_device(ptrs, lens, n, outs, status, stream))


def webp_decode_files_device(files, n_threads=8, stream=None, strict=True, crop=True, pixels="reference", planes=False, alpha=False):
    """ffhip_webp_decode_files_device: lossy WebP files of any sizes (list of bytes) in one call.  Every picture gets its place in ONE
    device allocation, at a 16-byte-aligned offset with the pitch 64 x its macroblock columns.  Returns (infos, [host BGRA [h][w][4]
    cropped to the probe's width x height (crop=False: the decoded 16*mbrows x 16*mbcols)], device buffer); with strict=False a
    failing file does not raise: its entry is None and a fourth element, the per-file status codes, follows.
    pixels='libwebp': ffhip_webp_decode_files_device_ex with FFHIP_WEBP_PIXELS_LIBWEBP -- libwebp's pixels (PIL's, a browser's) instead of
    the reference's; only the probe's width x height are written, so crop=False shows unwritten bytes beyond them.
    planes=True (needs pixels='libwebp'): a last element follows, per file (y, u, v) -- the loop-filtered planes of its macroblock grid --
    or None for a failing file.
    alpha=True (needs pixels='libwebp'): FFHIP_WEBP_ALPHA -- a file with an alpha plane gets it in byte 3 of its pixels."""
    flags = webp_pixel_flags(pixels)
    if planes and not flags:
        raise ValueError("planes=True needs pixels='libwebp'")
    if alpha and not flags:
        raise ValueError("alpha=True needs pixels='libwebp'")
    if alpha:
        flags |= capi.FFHIP_WEBP_ALPHA

    grids = []

    def probe(i, f):
        try:
            w, h, c, r = webp_probe(f, pixels)
        except capi.FfhipError:
            grids.append((0, 0))
            raise
        grids.append((c, r))
        return (64 * c, 16 * r, w, h) if crop else (64 * c, 16 * r, 16 * c, 16 * r)

    infos = (capi.WebpInfo * len(files))()
    pl = {}

    def call(L, ptrs, lens, n, outs, pitches, status):
        if not flags:
            return L.ffhip_webp_decode_files_device(ptrs, lens, n, n_threads, outs, pitches, infos, status, stream)
        triples = None
        if planes:
            offs, total = [], 0
            for c, r in grids:
                offs.append(total)
                total += 384 * c * r
            pl["buf"], pl["offs"] = DeviceBuffer(nbytes=max(total, 16)), offs
            triples = (C.c_void_p * (3 * max(n, 1)))()
            for i, (c, r) in enumerate(grids):
                base = pl["buf"].ptr + offs[i]
                triples[3 * i], triples[3 * i + 1], triples[3 * i + 2] = base, base + 256 * c * r, base + 320 * c * r
        return L.ffhip_webp_decode_files_device_ex(ptrs, lens, n, n_threads, outs, pitches, triples, flags, infos, status, stream)

    images, dout, status = _files_to_pictures(files, probe, call, "ffhip_webp_decode_files_device" + ("_ex" if flags else ""), strict,
                                              own_failure=lambda rc: rc not in (0, capi.FFHIP_EINVAL) and rc > -1000)
    out = (list(infos), images, dout) if strict else (list(infos), images, dout, status)
    if planes:
        flat = pl["buf"].to_host((pl["buf"].nbytes,), np.uint8) if "buf" in pl else None
        res = []
        for i, (c, r) in enumerate(grids):
            if status[i] or not c:
                res.append(None)
                continue
            o = pl["offs"][i]
            res.append((flat[o:o + 256 * c * r].reshape(16 * r, 16 * c).copy(), flat[o + 256 * c * r:o + 320 * c * r].reshape(8 * r, 8 * c).copy(),
                        flat[o + 320 * c * r:o + 384 * c * r].reshape(8 * r, 8 * c).copy()))
        out = out + (res,)
    return out


def vp8_libwebp_residual_mb(levels, has_y2, factors):
    """ffhip_vp8_libwebp_residual_mb (host, no device): one macroblock's levels [25][16], has_y2 and its six factors y1_dc, y1_ac, y2_dc,
    y2_ac, uv_dc, uv_ac -> (residual int16 [24][16], whether some block has a non-zero dequantised coefficient): the residual stage of
    pixels='libwebp' as the kernel compiles it."""
    lv = np.ascontiguousarray(levels, np.int16).reshape(25, 16)
    q = np.ascontiguousarray(np.asarray(factors).reshape(-1)[:6], np.uint16)
    res = np.zeros((24, 16), np.int16)
    nz = C.c_int()
    capi.check(capi.lib().ffhip_vp8_libwebp_residual_mb(lv.ctypes.data, int(bool(has_y2)), q.ctypes.data, res.ctypes.data, C.byref(nz)),
               "ffhip_vp8_libwebp_residual_mb")
    return res, bool(nz.value)


def webp_libwebp_color(y, u, v, pitch=None):
    """ffhip_webp_libwebp_color (host, no device): planes y [h][w], u / v [(h + 1) / 2][(w + 1) / 2] -> BGRA [h][w][4] by libwebp's fancy
    upsampler and colour step, as k_vp8_upsample_color compiles them."""
    y, u, v = (np.ascontiguousarray(p, np.uint8) for p in (y, u, v))
    h, w = y.shape
    if u.shape != ((h + 1) // 2, (w + 1) // 2) or v.shape != u.shape:
        raise ValueError(f"chroma planes {u.shape}, {v.shape} for a {w} x {h} picture")
    pitch = 4 * w if pitch is None else pitch
    out = np.zeros((h, pitch), np.uint8)
    capi.check(capi.lib().ffhip_webp_libwebp_color(y.ctypes.data, w, u.ctypes.data, v.ctypes.data, u.shape[1], w, h, out.ctypes.data, pitch),
               "ffhip_webp_libwebp_color")
    return out[:, :4 * w].reshape(h, w, 4)


def webp_alpha_probe(data):
    """ffhip_webp_alpha_probe (host, no device, cheap): a lossy WebP file (bytes) -> (has_alpha, compression, filter, pre_processing) of
    the ALPH chunk FFHIP_WEBP_ALPHA would decode; has_alpha 0 for a file the flag leaves opaque"""
    buf = np.frombuffer(data, dtype=np.uint8)
    v = [C.c_int() for _ in range(4)]
    capi.check(capi.lib().ffhip_webp_alpha_probe(buf.ctypes.data if buf.size else None, buf.size, *[C.byref(x) for x in v]), "ffhip_webp_alpha_probe")
    return tuple(x.value for x in v)


def webp_alpha_plane(data, pitch=None):
    """ffhip_webp_alpha_plane (host, no device): the whole alpha decode of a lossy WebP file (bytes), the filter undone by the function
    k_webp_alpha_unfilter compiles -> uint8 [h][w]"""
    w, h, _, _ = webp_probe(data, "libwebp")
    buf = np.frombuffer(data, dtype=np.uint8)
    pitch = w if pitch is None else pitch
    out = np.zeros((h, pitch), np.uint8)
    capi.check(capi.lib().ffhip_webp_alpha_plane(buf.ctypes.data, buf.size, out.ctypes.data, pitch), "ffhip_webp_alpha_plane")
    return out[:, :w]


def webp_alpha_last():
    """ffhip_debug_webp_alpha_last: (files with a plane, lossless ones among them, launches of k_webp_alpha_unfilter, parts) of this
    thread's last webp_decode_files_device(..., alpha=True)"""
    out = (C.c_int * 4)()
    capi.check(capi.lib().ffhip_debug_webp_alpha_last(out), "ffhip_debug_webp_alpha_last")
    return tuple(out)


def webp_alpha_times():
    """ffhip_debug_webp_alpha_times: milliseconds of that call's alpha stage -- (host walk, copies and stream decode; upload and the lossless
    planes' two kernels; k_webp_alpha_unfilter over its levels; k_webp_alpha_merge); the last three only while FFHIP_WEBP_ALPHA_TIMES is set"""
    out = (C.c_double * 4)()
    capi.check(capi.lib().ffhip_debug_webp_alpha_times(out), "ffhip_debug_webp_alpha_times")
    return tuple(out)


def webp_last_parts():
    """ffhip_debug_webp_last_parts: (parts the kernels took, parts the host threads took) in this thread's last WebP files call"""
    out = (C.c_int * 2)()
    capi.check(capi.lib().ffhip_debug_webp_last_parts(out), "ffhip_debug_webp_last_parts")
    return out[0], out[1]


def inflate(data, cap):
    """ffhip_inflate (host, no device): a zlib-wrapped deflate stream (bytes) into at most cap bytes -> bytes.  Everything the library
    refuses -- a bad header or check value, a stream that ends early, code lengths no tree has, output beyond cap -- is FfhipError (FFHIP_EINVAL)."""
    src = np.frombuffer(data, dtype=np.uint8)
    dst = np.zeros(max(int(cap), 1), np.uint8)
    got = C.c_size_t()
    capi.check(capi.lib().ffhip_inflate(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, int(cap), C.byref(got)), "ffhip_inflate")
    return dst[:got.value].tobytes()


def _inflate_host(entry, what, data, cap, *tail):
    src = np.frombuffer(data, dtype=np.uint8)
    dst = np.zeros(max(int(cap), 1), np.uint8)
    got = C.c_size_t()
    capi.check(entry(src.ctypes.data if src.size else dst.ctypes.data, src.size, dst.ctypes.data, int(cap), C.byref(got), *tail), what)
    return dst[:got.value].tobytes()


def inflate_upto(data, cap, partial=False):
    """ffhip_inflate_upto (host; csrc/ffhip_png_internal.h): ffhip_inflate, and with partial=True a stream that holds more than cap
    bytes is cut there and accepted, its check value not looked at"""
    return _inflate_host(capi.lib().ffhip_inflate_upto, "ffhip_inflate_upto", data, cap, int(bool(partial)))


def inflate_model(stream, cap, partial=False, mode=0):
    """ffhip_inflate_model (host): the model of k_inflate -- the body the kernel compiles, the wave's lanes emulated, every step as all 64
    loads, then all 64 stores.  Arguments, verdicts and bytes of inflate_upto.  mode: the emulation's variants for the test of the
    emulation itself (csrc/ffhip_inflate_model.c); 0 is the kernel's."""
    if mode:
        return _inflate_host(capi.lib().ffhip_inflate_model_mode, "ffhip_inflate_model_mode", stream, cap, int(bool(partial)), int(mode))
    return _inflate_host(capi.lib().ffhip_inflate_model, "ffhip_inflate_model", stream, cap, int(bool(partial)))


def inflate_streams_device(streams, caps=None, strict=True, stream=None, guard=0, fill=0):
    """ffhip_inflate_streams_device: zlib streams (list of bytes) inflated by k_inflate, a wave per stream, in one launch, each into its own
    piece of ONE device allocation.  caps: the pieces' sizes (None: found by the host decoder; a stream it refuses gets 0).  Returns
    (outputs, status): bytes per stream, None for a refused one, and the per-stream codes; strict: a refused stream raises.
    guard, fill: `guard` bytes of `fill` between the pieces (and the pieces filled with it), for tests; a third element follows then, the
    whole allocation as the call left it, with a fourth, the pieces' offsets."""
    L = capi.require_device()
    n = len(streams)
    if caps is None:
        caps = []
        for z in streams:
            try:
                caps.append(len(inflate_upto(z, 1 << 30 if len(z) > (1 << 20) else 1032 * max(len(z), 1))))
            except capi.FfhipError:
                caps.append(0)
    caps = [int(c) for c in caps]
    offs, total = [], guard
    for c in caps:
        offs.append(total)
        total += c + guard
    dout = DeviceBuffer(host=np.full(max(total, 16), fill, np.uint8))
    bufs = [np.frombuffer(z, dtype=np.uint8) for z in streams]
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
    outs = (C.c_void_p * max(n, 1))(*[dout.ptr + o if c else None for o, c in zip(offs, caps)])
    cap_arr = (C.c_size_t * max(n, 1))(*caps)
    got = (C.c_size_t * max(n, 1))()
    status = (C.c_int * max(n, 1))()
    rc = L.ffhip_inflate_streams_device(ptrs, lens, n, outs, cap_arr, got, status, stream)
    status = list(status)[:n]
    if strict or rc not in status:
        capi.check(rc, "ffhip_inflate_streams_device")
    flat = dout.to_host((max(total, 16),), np.uint8)
    outputs = [None if status[i] else flat[offs[i]:offs[i] + got[i]].tobytes() for i in range(n)]
    return (outputs, status, flat, offs) if guard else (outputs, status)


def png_inflate_flags(inflate):
    """inflate= of the PNG file calls -> their png_flags"""
    if inflate not in ("host", "device"):
        raise ValueError(f"inflate={inflate!r}: 'host' or 'device'")
    return capi.FFHIP_PNG_INFLATE_DEVICE if inflate == "device" else 0


def png_inflate_last():
    """ffhip_debug_png_inflate: (files inflated on the device, files inflated on the host, compressed bytes uploaded, milliseconds of
    k_inflate and its copy back -- only while FFHIP_PNG_TIMES is set) of this thread's last PNG file call, all its parts"""
    out = (C.c_double * 4)()
    capi.check(capi.lib().ffhip_debug_png_inflate(out), "ffhip_debug_png_inflate")
    return tuple(out)


def png_probe(data):
    """ffhip_png_probe (host, no device): a PNG file (bytes) -> capi.PngInfo: width, height, bit_depth, color_type, interlace, has_trns,
    palette_size, n_passes, filtered_bytes, pass_rows[7], pass_row_bytes[7]"""
    buf = np.frombuffer(data, dtype=np.uint8)
    info = capi.PngInfo()
    capi.check(capi.lib().ffhip_png_probe(buf.ctypes.data if buf.size else None, buf.size, C.byref(info)), "ffhip_png_probe")
    return info


def png_picture(data, pitch=None):
    """ffhip_png_picture (host, no device): the whole decode of a PNG file (bytes) by the functions the kernels compile -> BGRA [h][w][4]"""
    info = png_probe(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    pitch = 4 * info.width if pitch is None else pitch
    out = np.zeros((info.height, pitch), np.uint8)
    capi.check(capi.lib().ffhip_png_picture(buf.ctypes.data, buf.size, out.ctypes.data, pitch), "ffhip_png_picture")
    return out[:, :4 * info.width].reshape(info.height, info.width, 4)


def png_exif_orientation(data):
    """ffhip_png_exif_orientation: the same from a PNG file's eXIf chunk"""
    return _exif_orientation(capi.lib().ffhip_png_exif_orientation, data)


def png_decode_files_device(files, n_threads=8, stream=None, strict=True, inflate="host"):
    """ffhip_png_decode_files_device: PNG files of any sizes and kinds (list of bytes) in one call.  Every picture gets its place in ONE
    device allocation, at a 16-byte-aligned offset with the pitch 4 x its width rounded up to 16 bytes.  Returns (infos, [host BGRA
    [h][w][4], alpha included], device buffer); with strict=False a failing file does not raise: its entry is None and a fourth element,
    the per-file status codes, follows.  inflate: 'host', or 'device' -- ffhip_png_decode_files_device_ex with FFHIP_PNG_INFLATE_DEVICE:
    k_inflate inflates, a wave per file; the same pictures and codes."""
    png_flags = png_inflate_flags(inflate)

    def probe(i, f):
        info = png_probe(f)
        return ((4 * info.width + 15) & ~15, info.height, info.width, info.height)

    infos = (capi.PngInfo * max(len(files), 1))()

    def call(L, ptrs, lens, n, outs, pitches, status):
        if png_flags:
            return L.ffhip_png_decode_files_device_ex(ptrs, lens, n, n_threads, outs, pitches, infos, status, png_flags, stream)
        return L.ffhip_png_decode_files_device(ptrs, lens, n, n_threads, outs, pitches, infos, status, stream)

    images, dout, status = _files_to_pictures(files, probe, call, "ffhip_png_decode_files_device" + ("_ex" if png_flags else ""), strict)
    infos = list(infos)[:len(files)]
    return (infos, images, dout) if strict else (infos, images, dout, status)


def png_last():
    """ffhip_debug_png_last: (parts, launches of k_png_unfilter) of this thread's last ffhip_png_decode_files_device"""
    out = (C.c_int * 2)()
    capi.check(capi.lib().ffhip_debug_png_last(out), "ffhip_debug_png_last")
    return out[0], out[1]


def png_times():
    """ffhip_debug_png_times: milliseconds of this thread's last ffhip_png_decode_files_device -- (host chunk walk and inflate, upload,
    k_png_unfilter over its levels, k_png_expand); the last three only while FFHIP_PNG_TIMES is set"""
    out = (C.c_double * 4)()
    capi.check(capi.lib().ffhip_debug_png_times(out), "ffhip_debug_png_times")
    return tuple(out)


def vp8l_probe(data):
    """ffhip_vp8l_probe (host, no device, cheap): a lossless WebP file (bytes) -> (width, height, has_alpha) of its VP8L header"""
    buf = np.frombuffer(data, dtype=np.uint8)
    w, h, a = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().ffhip_vp8l_probe(buf.ctypes.data if buf.size else None, buf.size, C.byref(w), C.byref(h), C.byref(a)), "ffhip_vp8l_probe")
    return w.value, h.value, a.value


def vp8l_info(data):
    """ffhip_vp8l_read_info (host, no device): -> capi.Vp8lInfo: width, height, has_alpha, the transform types in the file's order, block
    bits, palette size and pixels per word, colour-cache bits, has_meta, residual_width"""
    buf = np.frombuffer(data, dtype=np.uint8)
    info = capi.Vp8lInfo()
    capi.check(capi.lib().ffhip_vp8l_read_info(buf.ctypes.data if buf.size else None, buf.size, C.byref(info)), "ffhip_vp8l_read_info")
    return info


def vp8l_picture(data, pitch=None):
    """ffhip_vp8l_picture (host, no device): the whole decode of a lossless WebP file (bytes), the transforms undone by the functions the
    kernels compile -> BGRA [h][w][4]"""
    w, h, _ = vp8l_probe(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    pitch = 4 * w if pitch is None else pitch
    out = np.zeros((h, pitch), np.uint8)
    capi.check(capi.lib().ffhip_vp8l_picture(buf.ctypes.data, buf.size, out.ctypes.data, pitch), "ffhip_vp8l_picture")
    return out[:, :4 * w].reshape(h, w, 4)


def vp8l_decode_files_device(files, n_threads=8, stream=None, strict=True):
    """ffhip_vp8l_decode_files_device: lossless WebP files of any sizes (list of bytes) in one call; shape and result of
    png_decode_files_device: (infos, [host BGRA [h][w][4], alpha included], device buffer), with strict=False the status codes fourth."""
    def probe(i, f):
        w, h, _ = vp8l_probe(f)
        return ((4 * w + 15) & ~15, h, w, h)

    infos = (capi.Vp8lInfo * max(len(files), 1))()

    def call(L, ptrs, lens, n, outs, pitches, status):
        return L.ffhip_vp8l_decode_files_device(ptrs, lens, n, n_threads, outs, pitches, infos, status, stream)

    images, dout, status = _files_to_pictures(files, probe, call, "ffhip_vp8l_decode_files_device", strict)
    infos = list(infos)[:len(files)]
    return (infos, images, dout) if strict else (infos, images, dout, status)


def vp8l_last():
    """ffhip_debug_vp8l_last: (parts, launches of k_vp8l_predict, files inverted on the host) of this thread's last
    ffhip_vp8l_decode_files_device"""
    out = (C.c_int * 3)()
    capi.check(capi.lib().ffhip_debug_vp8l_last(out), "ffhip_debug_vp8l_last")
    return out[0], out[1], out[2]


def vp8l_times():
    """ffhip_debug_vp8l_times: milliseconds of this thread's last ffhip_vp8l_decode_files_device -- (host stream decode, upload,
    k_vp8l_predict over its levels, k_vp8l_finish); the last three only while FFHIP_VP8L_TIMES is set"""
    out = (C.c_double * 4)()
    capi.check(capi.lib().ffhip_debug_vp8l_times(out), "ffhip_debug_vp8l_times")
    return tuple(out)


# ---- JPEG encoding (include/ffpic_hip.h "JPEG encoding") ----
JPEG_ENC_LAYOUTS = {"4:4:4": capi.FFHIP_JPEG_ENC_444, "4:2:2": capi.FFHIP_JPEG_ENC_422, "4:2:0": capi.FFHIP_JPEG_ENC_420, "grey": capi.FFHIP_JPEG_ENC_GREY}


def jpeg_encode_layout(layout):
    """a layout's FFHIP_JPEG_ENC_* value from its name ('4:4:4', '4:2:2', '4:2:0', 'grey') or the value itself"""
    if isinstance(layout, str):
        if layout not in JPEG_ENC_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(JPEG_ENC_LAYOUTS)}, got {layout!r}")
        return JPEG_ENC_LAYOUTS[layout]
    return int(layout)


def jpeg_encode_tables(quality):
    """ffhip_jpeg_encode_tables: libjpeg's quantiser tables of a quality -> uint16 [2][64] natural order (luma, chroma).  Needs no device."""
    out = np.zeros((2, 64), np.uint16)
    capi.check(capi.lib().ffhip_jpeg_encode_tables(int(quality), _vp(out)), "ffhip_jpeg_encode_tables")
    return out


def jpeg_encode_block(samples, quant):
    """ffhip_jpeg_encode_block: the quantised coefficients (int16 [64], natural order) of 64 samples: the islow forward DCT and libjpeg's
    quantiser.  Needs no device."""
    s = np.ascontiguousarray(samples, np.uint8).reshape(64)
    q = np.ascontiguousarray(quant, np.uint16).reshape(64)
    out = np.zeros(64, np.int16)
    capi.check(capi.lib().ffhip_jpeg_encode_block(_vp(s), _vp(q), _vp(out)), "ffhip_jpeg_encode_block")
    return out


def jpeg_encode_header(width, height, layout, quality, restart=0):
    """ffhip_jpeg_encode_header: the file's bytes in front of the scan data.  Needs no device."""
    out = np.zeros(capi.FFHIP_JPEG_ENC_HEADER_MAX, np.uint8)
    n = C.c_size_t()
    capi.check(capi.lib().ffhip_jpeg_encode_header(width, height, jpeg_encode_layout(layout), quality, restart, _vp(out), out.size, C.byref(n)),
               "ffhip_jpeg_encode_header")
    return out[:n.value].tobytes()


def jpeg_encode_bound(width, height, layout, restart=0):
    """ffhip_jpeg_encode_bound: a certain bound on the file's size (0: bad arguments).  Needs no device."""
    return int(capi.lib().ffhip_jpeg_encode_bound(width, height, jpeg_encode_layout(layout), restart))


def jpeg_host_source(pixels):
    """capi.JpegSource of a host array uint8 [H][W][3] (R, G, B) or [H][W] (grey), whatever its strides; keep the array alive"""
    if pixels.dtype != np.uint8 or pixels.ndim not in (2, 3) or (pixels.ndim == 3 and pixels.shape[2] != 3):
        raise ValueError("pixels must be uint8 [H][W][3] or [H][W]")
    st = pixels.strides
    chan = (0, st[2], 2 * st[2]) if pixels.ndim == 3 else (0,)
    return capi.jpeg_source(pixels.ctypes.data, pixels.shape[1], pixels.shape[0], st[0], st[1], chan, len(chan))


def jpeg_encode_picture(pixels, layout, quality=75, restart=0, cap=None):
    """ffhip_jpeg_encode_picture: host pixels (uint8 [H][W][3] RGB, or [H][W] for 'grey') to the file's bytes, the CPU model of
    jpeg_encode_items.  cap: the output's size (the bound when None); -> bytes, or with cap given (rc, length, the cap bytes)."""
    src = jpeg_host_source(pixels)
    size = jpeg_encode_bound(src.width, src.height, layout, restart) if cap is None else int(cap)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    rc = capi.lib().ffhip_jpeg_encode_picture(C.byref(src), jpeg_encode_layout(layout), quality, restart, _vp(out), size, C.byref(n))
    if cap is not None:
        return rc, n.value, out[:size].tobytes()
    capi.check(rc, "ffhip_jpeg_encode_picture")
    return out[:n.value].tobytes()


def jpeg_fdct_items(items, stream=None):
    """ffhip_jpeg_fdct_items: `items` a list of capi.JpegFdctItem (device pointers); pixels to quantised coefficient planes in MCU order, pictures
    of any sizes, layouts and qualities in one pair of launches.  Only enqueues on `stream`."""
    n = len(items)
    arr = (capi.JpegFdctItem * max(n, 1))(*items)
    capi.check(capi.lib().ffhip_jpeg_fdct_items(arr, n, stream), "ffhip_jpeg_fdct_items")


def _lengths_call(entry, kind, items, stream, strict):
    n = len(items)
    arr = (kind * max(n, 1))(*items)
    lens, status = (C.c_size_t * max(n, 1))(), (C.c_int * max(n, 1))()
    rc = getattr(capi.lib(), entry)(arr, n, lens, status, stream)
    status = list(status)[:n]
    if strict or (rc != 0 and rc not in status):
        capi.check(rc, entry)
    return list(lens)[:n], status


def jpeg_huff_encode_items(items, stream=None, strict=True):
    """ffhip_jpeg_huff_encode_items: `items` a list of capi.JpegHuffItem (device coefficient planes in MCU order) -> ([file length], [status]);
    the files are in the items' d_out.  Synchronises `stream` twice."""
    return _lengths_call("ffhip_jpeg_huff_encode_items", capi.JpegHuffItem, items, stream, strict)


def jpeg_encode_items(items, stream=None, strict=True):
    """ffhip_jpeg_encode_items: `items` a list of capi.JpegEncodeItem (device pictures) -> ([file length], [status]); the files are in the
    items' d_out.  With strict=False a file that does not fit its cap is its status (FFHIP_EJPEG_NOSPACE) and its length the size it needs."""
    return _lengths_call("ffhip_jpeg_encode_items", capi.JpegEncodeItem, items, stream, strict)


def deflate_bound(length):
    """ffhip_deflate_bound: a certain bound on the zlib stream of `length` bytes.  Needs no device."""
    return int(capi.lib().ffhip_deflate_bound(int(length)))


def deflate(data, cap=None):
    """ffhip_deflate (host, no device): bytes to a zlib stream under the rule of include/ffpic_hip.h "PNG encoding", the CPU model of
    deflate_streams_device.  cap: the output's size (the bound when None); -> bytes, or with cap given (rc, length, the cap bytes)."""
    src = np.frombuffer(data, dtype=np.uint8)
    size = deflate_bound(src.size) if cap is None else int(cap)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    rc = capi.lib().ffhip_deflate(src.ctypes.data if src.size else None, src.size, _vp(out), size, C.byref(n))
    if cap is not None:
        return rc, n.value, out[:size].tobytes()
    capi.check(rc, "ffhip_deflate")
    return out[:n.value].tobytes()


def deflate_code_lengths(freq, limit):
    """ffhip_deflate_code_lengths: the length rule alone -- frequencies (up to 288) -> uint8 code lengths of at most `limit` bits"""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(max(f.size, 1), np.uint8)
    capi.check(capi.lib().ffhip_deflate_code_lengths(_vp(f), f.size, int(limit), _vp(out)), "ffhip_deflate_code_lengths")
    return out[:f.size]


def deflate_streams_device(buffers, caps=None, strict=True, stream=None, guard=0, fill=0):
    """ffhip_deflate_streams_device: byte strings, uploaded into ONE device allocation, to zlib streams by k_deflate_chunks, each into its own
    piece of another.  caps: the pieces' sizes (None: the bound).  Returns (streams, lengths, status): bytes per buffer (what lies below its
    cap), the sizes the call names and the per-stream codes; strict: a stream that does not fit raises.  guard, fill: `guard` bytes of
    `fill` between the pieces (and the pieces filled with it), for tests; a fourth element follows then, the whole allocation as the call
    left it, with a fifth, the pieces' offsets."""
    L = capi.require_device()
    n = len(buffers)
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in buffers]
    caps = [deflate_bound(b.size) if caps is None or caps[k] is None else int(caps[k]) for k, b in enumerate(bufs)]
    in_offs, in_total = [], 0
    for b in bufs:
        in_offs.append(in_total)
        in_total += (b.size + 255) & ~255
    flat_in = np.zeros(max(in_total, 16), np.uint8)
    for o, b in zip(in_offs, bufs):
        flat_in[o:o + b.size] = b
    din = DeviceBuffer(host=flat_in)
    offs, total = [], guard
    for c in caps:
        offs.append(total)
        total += c + guard
    dout = DeviceBuffer(host=np.full(max(total, 16), fill, np.uint8))
    srcs = (C.c_void_p * max(n, 1))(*[din.ptr + o if b.size else None for o, b in zip(in_offs, bufs)])
    lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
    outs = (C.c_void_p * max(n, 1))(*[dout.ptr + o if c else None for o, c in zip(offs, caps)])
    cap_arr = (C.c_size_t * max(n, 1))(*caps)
    got = (C.c_size_t * max(n, 1))()
    status = (C.c_int * max(n, 1))()
    rc = L.ffhip_deflate_streams_device(srcs, lens, n, outs, cap_arr, got, status, stream)
    status = list(status)[:n]
    if strict or (rc != 0 and rc not in status):
        capi.check(rc, "ffhip_deflate_streams_device")
    flat = dout.to_host((max(total, 16),), np.uint8)
    streams = [flat[offs[i]:offs[i] + min(got[i], caps[i])].tobytes() for i in range(n)]
    return (streams, list(got)[:n], status, flat, offs) if guard else (streams, list(got)[:n], status)


def png_filter_id(filter):
    """'adaptive', 'none', 'sub', 'up', 'average', 'paeth' or 0..5 -> the filter argument of the PNG encoder"""
    names = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": capi.FFHIP_PNG_FILTER_ADAPTIVE}
    if isinstance(filter, str):
        if filter not in names:
            raise ValueError(f"filter={filter!r}: one of {sorted(names)}")
        return names[filter]
    if isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or not 0 <= int(filter) <= capi.FFHIP_PNG_FILTER_ADAPTIVE:
        raise ValueError(f"filter={filter!r}: 0..5 or a filter's name")
    return int(filter)


def png_host_source(pixels):
    """capi.PngSource of a host array uint8 [H][W][C] (C in 1..4, file order) or [H][W] (grey), whatever its strides; keep the array alive"""
    if pixels.dtype != np.uint8 or pixels.ndim not in (2, 3) or (pixels.ndim == 3 and not 1 <= pixels.shape[2] <= 4):
        raise ValueError("pixels must be uint8 [H][W][C] with C in 1..4, or [H][W]")
    st = pixels.strides
    chan = tuple(k * st[2] for k in range(pixels.shape[2])) if pixels.ndim == 3 else (0,)
    return capi.png_source(pixels.ctypes.data, pixels.shape[1], pixels.shape[0], st[0], st[1], chan)


def _png_src(pixels):
    return pixels if isinstance(pixels, capi.PngSource) else png_host_source(pixels)


def png_filtered_size(width, height, channels):
    return int(capi.lib().ffhip_png_filtered_size(width, height, channels))


def png_encode_bound(width, height, channels):
    """ffhip_png_encode_bound: a certain bound on the file's size (0: bad arguments).  Needs no device."""
    return int(capi.lib().ffhip_png_encode_bound(width, height, channels))


def png_filter_picture(pixels, filter="adaptive"):
    """ffhip_png_filter_picture: host pixels (an array as png_host_source takes it, or a capi.PngSource of host memory) -> the filtered
    picture's bytes: per row the filter type and width x channels bytes.  Needs no device."""
    src = _png_src(pixels)
    size = png_filtered_size(src.width, src.height, src.channels)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    capi.check(capi.lib().ffhip_png_filter_picture(C.byref(src), png_filter_id(filter), _vp(out), size, C.byref(n)), "ffhip_png_filter_picture")
    return out[:n.value].tobytes()


def png_encode_picture(pixels, filter="adaptive", cap=None):
    """ffhip_png_encode_picture: host pixels (as png_filter_picture) to the PNG file's bytes, the CPU model of png_encode_items.  cap: the
    output's size (the bound when None); -> bytes, or with cap given (rc, length, the cap bytes)."""
    src = _png_src(pixels)
    size = png_encode_bound(src.width, src.height, src.channels) if cap is None else int(cap)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    rc = capi.lib().ffhip_png_encode_picture(C.byref(src), png_filter_id(filter), _vp(out), size, C.byref(n))
    if cap is not None:
        return rc, n.value, out[:size].tobytes()
    capi.check(rc, "ffhip_png_encode_picture")
    return out[:n.value].tobytes()


def png_encode_items(items, stream=None, strict=True):
    """ffhip_png_encode_items: `items` a list of capi.PngEncodeItem (device pictures) -> ([file length], [status]); the files are in the
    items' d_out.  With strict=False a file that does not fit its cap is its status (FFHIP_EPNG_NOSPACE) and its length the size it needs."""
    return _lengths_call("ffhip_png_encode_items", capi.PngEncodeItem, items, stream, strict)


# ---- Lossless WebP encoding (include/ffpic_hip.h "Lossless WebP encoding") ----
def vp8l_encode_flags(predict=True, subtract_green=True):
    return (capi.FFHIP_VP8L_ENC_PREDICT if predict else 0) | (capi.FFHIP_VP8L_ENC_SUBTRACT_GREEN if subtract_green else 0)


def vp8l_encode_bound(width, height):
    """ffhip_vp8l_encode_bound: a certain bound on the file's size (0: bad arguments).  Needs no device."""
    return int(capi.lib().ffhip_vp8l_encode_bound(width, height))


def vp8l_encode_residual(pixels, flags=3):
    """ffhip_vp8l_encode_residual: host pixels (an array as png_host_source takes it, or a capi.PngSource of host memory) -> (the residual
    ARGB words uint32 [H][W] as the file codes them, the tiles' modes uint8 [tile rows][tile columns] or None without
    FFHIP_VP8L_ENC_PREDICT).  Needs no device."""
    src = _png_src(pixels)
    tile = 1 << capi.FFHIP_VP8L_ENC_TILE_BITS
    res = np.zeros((src.height, src.width), np.uint32)
    modes = np.zeros(((src.height + tile - 1) // tile, (src.width + tile - 1) // tile), np.uint8)
    capi.check(capi.lib().ffhip_vp8l_encode_residual(C.byref(src), int(flags), _vp(res), _vp(modes)), "ffhip_vp8l_encode_residual")
    return res, (modes if int(flags) & capi.FFHIP_VP8L_ENC_PREDICT else None)


def vp8l_encode_picture(pixels, flags=3, cap=None):
    """ffhip_vp8l_encode_picture: host pixels (as vp8l_encode_residual) to the lossless WebP file's bytes, the CPU model of
    vp8l_encode_items.  cap: the output's size (the bound when None); -> bytes, or with cap given (rc, length, the cap bytes)."""
    src = _png_src(pixels)
    size = vp8l_encode_bound(src.width, src.height) if cap is None else int(cap)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    rc = capi.lib().ffhip_vp8l_encode_picture(C.byref(src), int(flags), _vp(out), size, C.byref(n))
    if cap is not None:
        return rc, n.value, out[:size].tobytes()
    capi.check(rc, "ffhip_vp8l_encode_picture")
    return out[:n.value].tobytes()


def vp8l_encode_items(items, stream=None, strict=True):
    """ffhip_vp8l_encode_items: `items` a list of capi.Vp8lEncodeItem (device pictures) -> ([file length], [status]); the files are in the
    items' d_out.  With strict=False a file that does not fit its cap is its status (FFHIP_EVP8L_NOSPACE) and its length the size it needs."""
    return _lengths_call("ffhip_vp8l_encode_items", capi.Vp8lEncodeItem, items, stream, strict)


# ---- lossy WebP encoding (include/ffpic_hip.h "Lossy WebP encoding")
def _vp8_src(pixels):
    return pixels if isinstance(pixels, capi.JpegSource) else jpeg_host_source(pixels)


def vp8_encode_quality_index(quality):
    """ffhip_vp8_encode_quality_index: y_ac_qi of a quality 0..100.  Needs no device."""
    qi = int(capi.lib().ffhip_vp8_encode_quality_index(int(quality)))
    capi.check(min(qi, 0), "ffhip_vp8_encode_quality_index")
    return qi


def vp8_encode_bound(width, height):
    """ffhip_vp8_encode_bound: a certain bound on the file's size (0: bad arguments).  Needs no device."""
    return int(capi.lib().ffhip_vp8_encode_bound(width, height))


def vp8_encode_planes(pixels):
    """ffhip_vp8_encode_planes: host pixels (uint8 [H][W][3] RGB or [H][W] grey, or a capi.JpegSource of host memory) -> (y, u, v), the padded
    planes of the macroblock grid.  Needs no device."""
    src = _vp8_src(pixels)
    cols, rows = (src.width + 15) >> 4, (src.height + 15) >> 4
    y, u, v = np.zeros((16 * rows, 16 * cols), np.uint8), np.zeros((8 * rows, 8 * cols), np.uint8), np.zeros((8 * rows, 8 * cols), np.uint8)
    capi.check(capi.lib().ffhip_vp8_encode_planes(C.byref(src), _vp(y), _vp(u), _vp(v)), "ffhip_vp8_encode_planes")
    return y, u, v


def vp8_encode_mbs(pixels, quality=75):
    """ffhip_vp8_encode_mbs: host pixels (as vp8_encode_planes) -> dict(ymode [n], uvmode [n], levels [n][25][16], y, u, v): modes, levels
    in tests/vp8_writer.keyframe_from's layout and the unfiltered reconstruction.  Needs no device."""
    src = _vp8_src(pixels)
    cols, rows = (src.width + 15) >> 4, (src.height + 15) >> 4
    n = cols * rows
    out = dict(ymode=np.zeros(n, np.uint8), uvmode=np.zeros(n, np.uint8), levels=np.zeros((n, 25, 16), np.int16),
               y=np.zeros((16 * rows, 16 * cols), np.uint8), u=np.zeros((8 * rows, 8 * cols), np.uint8), v=np.zeros((8 * rows, 8 * cols), np.uint8))
    capi.check(capi.lib().ffhip_vp8_encode_mbs(C.byref(src), int(quality), *[_vp(out[k]) for k in ("ymode", "uvmode", "levels", "y", "u", "v")]),
               "ffhip_vp8_encode_mbs")
    return out


def vp8_encode_picture(pixels, quality=75, filter=-1, cap=None):
    """ffhip_vp8_encode_picture: host pixels (as vp8_encode_planes) to the lossy WebP file's bytes, the CPU model of vp8_encode_items.
    filter: the loop filter level 0..63, -1 for the rule's own.  cap: the output's size (the bound when None); -> bytes, or with cap
    given (rc, length, the cap bytes)."""
    src = _vp8_src(pixels)
    size = vp8_encode_bound(src.width, src.height) if cap is None else int(cap)
    out = np.zeros(max(size, 1), np.uint8)
    n = C.c_size_t()
    rc = capi.lib().ffhip_vp8_encode_picture(C.byref(src), int(quality), int(filter), _vp(out), size, C.byref(n))
    if cap is not None:
        return rc, n.value, out[:size].tobytes()
    capi.check(rc, "ffhip_vp8_encode_picture")
    return out[:n.value].tobytes()


def vp8_encode_items(items, stream=None, strict=True):
    """ffhip_vp8_encode_items: `items` a list of capi.Vp8EncodeItem (device pictures) -> ([file length], [status]); the files are in the
    items' d_out.  With strict=False a file that does not fit its cap is its status (FFHIP_EVP8_NOSPACE) and its length the size it needs."""
    return _lengths_call("ffhip_vp8_encode_items", capi.Vp8EncodeItem, items, stream, strict)
