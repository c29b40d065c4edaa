/* ffhip_webp_alpha_body.h -- the alpha plane's filter rule (include/ffpic_hip.h, "lossy WebP, the alpha plane") as
 * ffhip_webp_alpha_plane (ffhip_webp_alpha.c) and k_webp_alpha_unfilter (ffhip_webp_alpha_gpu.hip) compile it.  Plain C without builtins.
 *
 * A sample is its stored byte plus a prediction from the FINISHED plane, modulo 256.  With a = left, b = above, c = above left:
 *   filter 1 (horizontal) a;  filter 2 (vertical) b;  filter 3 (gradient) clip255(a + b - c).
 * Row 0 is horizontal under every filter, with 0 to the left of (0, 0); column 0 of every later row predicts from above.  A caller gets
 * both edges from the one function by what it passes for the first sample of a row: a = c = 0 in row 0, a = c = b in the rows below
 * (horizontal then gives b, the gradient b + b - b). */
#ifndef FFHIP_WEBP_ALPHA_BODY_H
#define FFHIP_WEBP_ALPHA_BODY_H

#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define FFHIP_WEBP_ALPHA_FN __host__ __device__ static inline

#define FFHIP_WEBP_ALPHA_HORIZONTAL 1
#define FFHIP_WEBP_ALPHA_VERTICAL 2
#define FFHIP_WEBP_ALPHA_GRADIENT 3

/* mode: the filter 1..3, or 1 for a sample of row 0 */
FFHIP_WEBP_ALPHA_FN int ffhip_webp_alpha_sample(int mode, int stored, int a, int b, int c)
{
    int pred = a;
    if (mode == FFHIP_WEBP_ALPHA_VERTICAL) pred = b;
    if (mode == FFHIP_WEBP_ALPHA_GRADIENT) {
        pred = a + b - c;
        pred = pred < 0 ? 0 : pred > 255 ? 255 : pred;
    }
    return (stored + pred) & 255;
}

/* a whole plane on the host: sample (x, y) of the stored plane is src[y * src_pitch + x * src_step]; filter 1..3 */
FFHIP_WEBP_ALPHA_FN void ffhip_webp_alpha_unfilter_rows(const uint8_t *src, int64_t src_pitch, int src_step, int filter, uint32_t width, uint32_t height,
                                                        uint8_t *out, int64_t pitch)
{
    for (uint32_t y = 0; y < height; y++) {
        const uint8_t *in = src + (int64_t)y * src_pitch;
        uint8_t *cur = out + (int64_t)y * pitch;
        const uint8_t *up = y ? cur - pitch : 0;
        const int mode = y ? filter : FFHIP_WEBP_ALPHA_HORIZONTAL;
        for (uint32_t x = 0; x < width; x++) {
            const int b = up ? up[x] : 0;
            const int a = x ? cur[x - 1] : b, c = x ? (up ? up[x - 1] : 0) : b;
            cur[x] = (uint8_t)ffhip_webp_alpha_sample(mode, in[(int64_t)x * src_step], a, b, c);
        }
    }
}

#endif
