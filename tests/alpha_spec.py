"""The witness of the alpha rule (include/ffpic_hip.h, "alpha into the tensors"), written in numpy from the rule's text and
from nothing in the C: div255, premultiply, un-premultiply, over a background; the sink's four- and three-channel outputs; the
premultiplying resize (the taps of the axis rule come from ffhip_resize_axis_taps, as the rule of 4.11 says); the chain of the file calls
(resize in the stored axes, turn, sink).  Pictures are uint8 [h][w][4], B,G,R,A."""
import numpy as np

MODES = ("straight", "premultiplied", "over")


def div255(t):
    """floor(t / 255 + 1/2) for t in 0..65025, by shifts"""
    t = np.asarray(t, dtype=np.int64) + 128
    return (t + (t >> 8)) >> 8


def premultiply(bgra):
    v = np.asarray(bgra).astype(np.int64)
    out = v.copy()
    out[..., :3] = div255(v[..., :3] * v[..., 3:4])
    return out.astype(np.uint8)


def unpremultiply(bgra):
    """a == 0 ? 0 : floor(255 p / a); a pixel with p > a is no premultiplied pixel and saturates at 255"""
    v = np.asarray(bgra).astype(np.int64)
    a = v[..., 3:4]
    out = v.copy()
    out[..., :3] = np.where(a == 0, 0, np.minimum((255 * v[..., :3]) // np.maximum(a, 1), 255))
    return out.astype(np.uint8)


def over(bgra, background_bgr, source_premultiplied=False):
    """the three colour bytes [h][w][3] (B,G,R) of the picture composited over the background"""
    v = np.asarray(bgra).astype(np.int64)
    a, g = v[..., 3:4], np.asarray(background_bgr, dtype=np.int64)
    if source_premultiplied:
        return np.minimum(v[..., :3] + div255(g * (255 - a)), 255).astype(np.uint8)
    return div255(v[..., :3] * a + g * (255 - a)).astype(np.uint8)


def channels(bgra, mode, source_premultiplied=False, background_rgb=(0, 0, 0), bgr=False):
    """the bytes of the output's channels, [h][w][C] in output order: C = 4 (colour, then alpha) or 3 for 'over'"""
    bgra = np.asarray(bgra, dtype=np.uint8)
    if mode == "over":
        colour = over(bgra, tuple(background_rgb)[::-1], source_premultiplied)
    elif mode == "straight":
        colour = (unpremultiply(bgra) if source_premultiplied else bgra)[..., :3]
    elif mode == "premultiplied":
        colour = (bgra if source_premultiplied else premultiply(bgra))[..., :3]
    else:
        raise ValueError(mode)
    colour = colour if bgr else colour[..., ::-1]
    return colour if mode == "over" else np.concatenate([colour, bgra[..., 3:4]], -1)


def sink(bgra, mode, np_dtype=np.uint8, planar=True, bgr=False, scale=(1, 1, 1), bias=(0, 0, 0), alpha_scale=1.0, alpha_bias=0.0,
         source_premultiplied=False, background_rgb=(0, 0, 0)):
    """the tensor: [C][h][w] (planar) or [h][w][C]; floats are float32(byte) * float32(scale) + float32(bias), each operation rounded to
    float32, float16 that float32 rounded to nearest even"""
    ch = channels(bgra, mode, source_premultiplied, background_rgb, bgr)
    if np.dtype(np_dtype) != np.uint8:
        sc = np.array(list(scale) + [alpha_scale], np.float32)[:ch.shape[-1]]
        bi = np.array(list(bias) + [alpha_bias], np.float32)[:ch.shape[-1]]
        prod = ch.astype(np.float32) * sc
        ch = (prod + bi).astype(np.float32).astype(np_dtype)
    return np.ascontiguousarray(ch.transpose(2, 0, 1)) if planar else ch


def filter_rule(v, oh, ow, antialias, axis_taps):
    """the rule of 4.11 over the four bytes alike: (sum_y sum_x qy qx v + 2^23) >> 24; axis_taps(n_in, n_out, antialias) ->
    (first[n_out], [weights])"""
    v = np.asarray(v).astype(np.int64)
    h, w = v.shape[:2]

    def matrix(n_in, n_out):
        first, taps = axis_taps(n_in, n_out, antialias)
        m = np.zeros((n_out, n_in), np.int64)
        for o in range(n_out):
            m[o, first[o]:first[o] + len(taps[o])] = taps[o].astype(np.int64)
        assert (m.sum(1) == 4096).all() and m.min() >= 0
        return m

    acc = np.einsum("oy,yxc->oxc", matrix(h, oh), v)
    acc = np.einsum("px,oxc->opc", matrix(w, ow), acc)
    return ((acc + (1 << 23)) >> 24).astype(np.uint8)


def resize_premultiplied(bgra, oh, ow, antialias, axis_taps):
    """straight BGRA in, premultiplied BGRA out: premultiply, then the rule of 4.11"""
    return filter_rule(premultiply(bgra), oh, ow, antialias, axis_taps)


def chain(bgra, mode, axis_taps, orient, size=None, orientation=1, antialias=True, **fmt):
    """what a files-to-tensors call with alpha= delivers for a decoded picture: the resize in the STORED axes (the upright size swapped for
    orientations 5..8), the turn (orient(picture, o): the EXIF table), the sink, told that its source is premultiplied behind a resize"""
    v, pre = np.asarray(bgra, dtype=np.uint8), False
    if size is not None:
        oh, ow = size if orientation < 5 else size[::-1]
        v, pre = resize_premultiplied(v, oh, ow, antialias, axis_taps), True
    if orientation != 1:
        v = orient(v, orientation)
    return sink(v, mode, source_premultiplied=pre, **fmt)
