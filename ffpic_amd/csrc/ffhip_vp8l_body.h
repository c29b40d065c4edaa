/* ffhip_vp8l_body.h -- the inverse transforms of lossless WebP (include/ffpic_hip.h, "lossless WebP") as the host decoder
 * (ffhip_vp8l.c) and the two kernels (ffhip_vp8l_gpu.hip) compile them: one function per transform step, on ARGB words
 * (alpha << 24 | red << 16 | green << 8 | blue: BGRA bytes in memory).  Plain C, so that a C program can hold it against the rule written
 * another way; the one builtin, Select's sum of absolute differences on the device, has its plain form beside it.
 *
 * The predictor works on CHUNKS of four pixels that start at a multiple of four: the block size is at least four, so a chunk has one mode,
 * and the switch over the 14 modes is taken once per chunk, not once per pixel.  A chunk's neighbours come as up[6]: up[0] the pixel above
 * left of the chunk's first, up[1..4] the four above, up[5] the one above right of its last. */
#ifndef FFHIP_VP8L_BODY_H
#define FFHIP_VP8L_BODY_H

#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define FFHIP_VP8L_FN __host__ __device__ static inline
#ifdef __clang__
#define FFHIP_VP8L_UNROLL _Pragma("unroll")
#else
#define FFHIP_VP8L_UNROLL
#endif

enum { FFHIP_VP8L_PREDICTOR = 0, FFHIP_VP8L_CROSS_COLOR = 1, FFHIP_VP8L_ADD_GREEN = 2, FFHIP_VP8L_COLOR_INDEXING = 3 };

/* per byte, modulo 256 */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_add(uint32_t a, uint32_t b)
{
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}

/* per byte, (a + b) >> 1 */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_avg2(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1); }

FFHIP_VP8L_FN int ffhip_vp8l_sad(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__builtin_amdgcn_sad_u8(a, b, 0u); /* the one instruction that is this sum */
#endif
    int s = 0;
    FFHIP_VP8L_UNROLL
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 255u) - (int)((b >> k) & 255u);
        s += d < 0 ? -d : d;
    }
    return s;
}

/* L when T is nearer to TL than L is, over the four channels' absolute differences; otherwise T */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_select(uint32_t L, uint32_t T, uint32_t TL) { return ffhip_vp8l_sad(T, TL) < ffhip_vp8l_sad(L, TL) ? L : T; }

FFHIP_VP8L_FN uint32_t ffhip_vp8l_clamp_full(uint32_t L, uint32_t T, uint32_t TL)
{
    uint32_t out = 0;
    FFHIP_VP8L_UNROLL
    for (int k = 0; k < 32; k += 8) {
        const int v = (int)((L >> k) & 255u) + (int)((T >> k) & 255u) - (int)((TL >> k) & 255u);
        out |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << k;
    }
    return out;
}

/* a + (a - b) / 2 per byte, the division truncating toward zero */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_clamp_half(uint32_t a, uint32_t b)
{
    uint32_t out = 0;
    FFHIP_VP8L_UNROLL
    for (int k = 0; k < 32; k += 8) {
        const int x = (int)((a >> k) & 255u), v = x + (x - (int)((b >> k) & 255u)) / 2;
        out |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << k;
    }
    return out;
}

#define FFHIP_VP8L_MODES(M) \
    M(1, L) M(2, T) M(3, TR) M(4, TL) M(5, ffhip_vp8l_avg2(ffhip_vp8l_avg2(L, TR), T)) M(6, ffhip_vp8l_avg2(L, TL)) M(7, ffhip_vp8l_avg2(L, T)) \
    M(8, ffhip_vp8l_avg2(TL, T)) M(9, ffhip_vp8l_avg2(T, TR)) M(10, ffhip_vp8l_avg2(ffhip_vp8l_avg2(L, TL), ffhip_vp8l_avg2(T, TR))) \
    M(11, ffhip_vp8l_select(L, T, TL)) M(12, ffhip_vp8l_clamp_full(L, T, TL)) M(13, ffhip_vp8l_clamp_half(ffhip_vp8l_avg2(L, T), TL))

/* one pixel's prediction; mode 0..15, 14 and 15 as 0 */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_predict(int mode, uint32_t L, uint32_t T, uint32_t TR, uint32_t TL)
{
    switch (mode) {
#define FFHIP_VP8L_ONE(k, expr) case k: return expr;
        FFHIP_VP8L_MODES(FFHIP_VP8L_ONE)
#undef FFHIP_VP8L_ONE
    default: return 0xff000000u;
    }
}

/* A chunk's n <= 4 pixels: res + prediction -> out.  mode_first is the first pixel's mode (what the picture's top row and left column
 * impose on it, or the block's), mode the others'; left is the pixel in front of the chunk.  tr_own: the pixel 1..3 whose TR is the chunk's
 * own first pixel -- the last pixel of a row that is one chunk long -- or 0 */
FFHIP_VP8L_FN void ffhip_vp8l_predict_chunk(int mode_first, int mode, int n, int tr_own, const uint32_t res[4], uint32_t left, const uint32_t up[6],
                                            uint32_t out[4])
{
    uint32_t L = out[0] = ffhip_vp8l_add(res[0], ffhip_vp8l_predict(mode_first, left, up[1], up[2], up[0]));
    switch (mode) {
#define FFHIP_VP8L_ONE(k, expr)                                      \
    case k:                                                          \
        FFHIP_VP8L_UNROLL                                            \
        for (int j = 1; j < 4; j++) {                                \
            if (j >= n) continue;                                    \
            const uint32_t T = up[j + 1], TR = j == tr_own ? out[0] : up[j + 2], TL = up[j]; \
            (void)T; (void)TR; (void)TL;                             \
            L = out[j] = ffhip_vp8l_add(res[j], expr);               \
        }                                                            \
        break;
        FFHIP_VP8L_MODES(FFHIP_VP8L_ONE)
#undef FFHIP_VP8L_ONE
    default:
        FFHIP_VP8L_UNROLL
        for (int j = 1; j < 4; j++) {
            if (j >= n) continue;
            out[j] = ffhip_vp8l_add(res[j], 0xff000000u);
        }
        break;
    }
}

/* the mode of a block: the low four bits of its pixel's green byte */
FFHIP_VP8L_FN int ffhip_vp8l_mode_of(uint32_t block_pixel) { return (int)((block_pixel >> 8) & 15u); }

/* The predictor undone over a whole image in place: h rows of w words, modes at block resolution (bx blocks a row).  A row's last pixel
 * takes the word behind the row above -- the current row's first pixel -- as its TR: the rows lie one behind the other */
FFHIP_VP8L_FN void ffhip_vp8l_predict_rows(uint32_t *px, uint32_t w, uint32_t h, int bits, const uint32_t *modes, uint32_t bx)
{
    for (uint32_t y = 0; y < h; y++) {
        uint32_t *cur = px + (uint64_t)y * w;
        const uint32_t *above = y ? cur - w : cur;
        for (uint32_t x0 = 0; x0 < w; x0 += 4) {
            const int n = w - x0 < 4 ? (int)(w - x0) : 4;
            const int block = y ? ffhip_vp8l_mode_of(modes[(uint64_t)(y >> bits) * bx + (x0 >> bits)]) : 1;
            uint32_t up[6] = {0, 0, 0, 0, 0, 0}, res[4] = {0, 0, 0, 0}, out[4];
            for (int k = 0; y && k <= n + 1; k++)
                if (x0 + (uint32_t)k >= 1) up[k] = above[x0 + (uint32_t)k - 1];
            for (int j = 0; j < n; j++) res[j] = cur[x0 + (uint32_t)j];
            ffhip_vp8l_predict_chunk(x0 ? block : y ? 2 : 0, block, n, w <= 4 ? n - 1 : 0, res, x0 ? cur[x0 - 1] : 0, up, out);
            for (int j = 0; j < n; j++) cur[x0 + (uint32_t)j] = out[j];
        }
    }
}

FFHIP_VP8L_FN int ffhip_vp8l_delta(uint32_t mult, uint32_t colour) { return ((int)(int8_t)(uint8_t)mult * (int)(int8_t)(uint8_t)colour) >> 5; }

/* cross-colour undone on one pixel; m is its block's pixel: green_to_red in bits 0..7, green_to_blue in 8..15, red_to_blue in 16..23.
 * Blue takes the NEW red */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_cross(uint32_t v, uint32_t m)
{
    const uint32_t g = (v >> 8) & 255u;
    const uint32_t r = ((v >> 16) + (uint32_t)ffhip_vp8l_delta(m, g)) & 255u;
    const uint32_t b = (v + (uint32_t)ffhip_vp8l_delta(m >> 8, g) + (uint32_t)ffhip_vp8l_delta(m >> 16, r)) & 255u;
    return (v & 0xff00ff00u) | r << 16 | b;
}

FFHIP_VP8L_FN uint32_t ffhip_vp8l_add_green(uint32_t v)
{
    const uint32_t g = (v >> 8) & 255u;
    return (v & 0xff00ff00u) | (((v & 0x00ff00ffu) + (g << 16 | g)) & 0x00ff00ffu);
}

/* pixel x of a row whose words hold 1 << bits indices each in their green byte, the first pixel lowest; pal has 256 entries, 0 beyond the
 * file's */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_index(uint32_t word, uint32_t x, int bits, const uint32_t *pal)
{
    const int depth = 8 >> bits;
    return pal[(((word >> 8) & 255u) >> (depth * (int)(x & ((1u << bits) - 1)))) & ((1u << depth) - 1)];
}

/* What the pointwise steps need of a file, and the steps of the device form in the order they are undone.  A step is a transform type:
 * cross-colour or add-green; colour indexing, when the file has it, is undone last of all and has its own flag */
typedef struct ffhip_vp8l_steps {
    uint8_t n_pre, pre[2];   /* undone before the predictor: k_vp8l_predict applies them to the residual as it loads it */
    uint8_t has_predictor;
    uint8_t n_post, post[2]; /* undone behind it (or alone): k_vp8l_finish */
    uint8_t has_index, index_bits, has_alpha;
    uint8_t predictor_bits, cross_bits;
    uint32_t predictor_bx, cross_bx; /* blocks in a row of the two block images */
} ffhip_vp8l_steps;

/* one pointwise step on the word at (x, y) of the image it is undone on */
FFHIP_VP8L_FN uint32_t ffhip_vp8l_pointwise(int type, uint32_t v, uint32_t x, uint32_t y, const ffhip_vp8l_steps *s, const uint32_t *cross)
{
    if (type == FFHIP_VP8L_ADD_GREEN) return ffhip_vp8l_add_green(v);
    return ffhip_vp8l_cross(v, cross[(uint64_t)(y >> s->cross_bits) * s->cross_bx + (x >> s->cross_bits)]);
}

#endif
