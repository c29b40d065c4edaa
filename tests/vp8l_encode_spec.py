"""The lossless WebP encoder's witness: the TRANSFORMS rule of include/ffpic_hip.h ("Lossless WebP encoding") written once more with numpy,
from the rule's and the format's text, and nothing of the library's.  The 14 predictors are restated here on whole pictures; the residual
the witness arrives at is also run through tests/vp8l_writer.py's forward(), the decoders' answer key, by check_against_writer().

Pixels are ARGB words, or their channels as int32 [H][W][4] in the order blue, green, red, alpha (the words' bytes, lowest first)."""
import numpy as np

import vp8l_writer as W

SUBTRACT_GREEN, PREDICT = 1, 2
TILE_BITS = 4                 # FFHIP_VP8L_ENC_TILE_BITS
CHUNK = 4096                  # FFHIP_VP8L_ENC_CHUNK


def rgba_of(samples):
    """samples uint8 [H][W][C], C in 1..4 in file order -> what a decoder has to give back: uint8 [H][W][4] R, G, B, A"""
    h, w, c = samples.shape
    out = np.full((h, w, 4), 255, np.uint8)
    if c <= 2:
        out[..., :3] = samples[..., :1]
    else:
        out[..., :3] = samples[..., :3]
    if c in (2, 4):
        out[..., 3] = samples[..., c - 1]
    return out


def channels_of(samples, flags):
    """int32 [H][W][4] blue, green, red, alpha; green subtracted from red and blue with SUBTRACT_GREEN"""
    rgba = rgba_of(samples).astype(np.int32)
    ch = rgba[..., [2, 1, 0, 3]]
    if flags & SUBTRACT_GREEN:
        ch[..., 0] = (ch[..., 0] - ch[..., 1]) & 255
        ch[..., 2] = (ch[..., 2] - ch[..., 1]) & 255
    return ch


def words_of(ch):
    ch = ch.astype(np.uint32) & 255
    return ch[..., 0] | ch[..., 1] << 8 | ch[..., 2] << 16 | ch[..., 3] << 24


def half(a, b):
    return (a + b) >> 1


def predictions(ch):
    """the 14 predictions of every pixel with a row above and a pixel to its left: [14][H-1][W-1][4]"""
    L, T, TL = ch[1:, :-1], ch[:-1, 1:], ch[:-1, :-1]
    TR = np.concatenate([ch[:-1, 2:], ch[1:, :1]], axis=1)       # the rightmost pixel's: its row's first pixel
    black = np.zeros_like(L)
    black[..., 3] = 255
    est = L + T - TL
    dl, dt = np.abs(est - L).sum(-1, keepdims=True), np.abs(est - T).sum(-1, keepdims=True)
    avg = half(L, T)
    d = avg - TL
    return np.stack([black, L, T, TR, TL, half(half(L, TR), T), half(L, TL), half(L, T), half(TL, T), half(T, TR), half(half(L, TL), half(T, TR)),
                     np.where(dl < dt, L, T), np.clip(est, 0, 255), np.clip(avg + np.sign(d) * (np.abs(d) // 2), 0, 255)])


def cost(res):
    """residual bytes read as signed, the absolute values summed over the channels"""
    r = res & 255
    return np.where(r < 128, r, 256 - r).sum(-1)


def residual(samples, flags, tile_bits=TILE_BITS):
    """-> (residual words uint32 [H][W], modes uint8 [tile rows][tile columns] or None, sums int64 [tile rows][tile columns][14] or None)"""
    ch = channels_of(samples, flags)
    h, w = ch.shape[:2]
    if not flags & PREDICT:
        return words_of(ch), None, None
    tile = 1 << tile_bits
    ty, tx = -(-h // tile), -(-w // tile)
    sums = np.zeros((ty, tx, 14), np.int64)
    res = np.zeros_like(ch)
    res[0, 0] = ch[0, 0] - np.array([0, 0, 0, 255])
    res[0, 1:] = ch[0, 1:] - ch[0, :-1]
    res[1:, 0] = ch[1:, 0] - ch[:-1, 0]
    modes = np.zeros((ty, tx), np.uint8)
    if h > 1 and w > 1:
        pred = predictions(ch)
        costs = np.zeros((14, h, w), np.int64)                    # what the format fixes adds nothing to any mode
        costs[:, 1:, 1:] = cost(ch[None, 1:, 1:] - pred)
        for j in range(ty):
            for i in range(tx):
                sums[j, i] = costs[:, j * tile:(j + 1) * tile, i * tile:(i + 1) * tile].sum((1, 2))
        modes = sums.argmin(-1).astype(np.uint8)                  # the first of equal ones
        per_pixel = np.repeat(np.repeat(modes, tile, 0), tile, 1)[1:h, 1:w].astype(np.int64)
        chosen = np.take_along_axis(pred, per_pixel[None, ..., None], 0)[0]
        res[1:, 1:] = ch[1:, 1:] - chosen
    return words_of(res), modes, sums


def check_against_writer(samples, flags, res, modes, tile_bits=TILE_BITS):
    """tests/vp8l_writer.py's forward() of the same transforms with the witness's modes gives the witness's residual"""
    h, w = samples.shape[:2]
    words = [int(v) for v in words_of(channels_of(samples, 0)).reshape(-1)]
    if flags & SUBTRACT_GREEN:
        words = W.forward(words, w, h, {"type": W.ADD_GREEN})
    if flags & PREDICT:
        words = W.forward(words, w, h, {"type": W.PREDICTOR, "bits": tile_bits, "image": modes.astype(np.uint32) << 8})
    assert np.array_equal(np.array(words, np.uint32).reshape(h, w), res)


def to_bgra(samples):
    return rgba_of(samples)[..., [2, 1, 0, 3]]
