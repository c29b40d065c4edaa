/* ffhip_alpha_body.h -- the integer alpha rule (include/ffpic_hip.h, "alpha into the tensors"), one function per step.  Plain
 * C++ without builtins, __host__ too: the tensor sink (ffhip_tensor_body.h), the premultiplying resize (ffhip_resize.hip) and a CPU program
 * run the same text.  c, p, g and a are bytes. */
#ifndef FFHIP_ALPHA_BODY_H
#define FFHIP_ALPHA_BODY_H

#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

/* floor(t / 255 + 1/2) for t in 0..65025 */
__host__ __device__ inline uint32_t alpha_div255(uint32_t t)
{
    t += 128u;
    return (t + (t >> 8)) >> 8;
}

__host__ __device__ inline uint32_t alpha_premultiply(uint32_t c, uint32_t a) { return alpha_div255(c * a); }

/* a == 0 ? 0 : floor(255 p / a), exact for p <= a; a pixel that is not premultiplied (p > a) saturates at 255.  No integer division: one
 * float reciprocal per alpha (the compiler shares it among a pixel's three colours), then per byte a product, a sum and a truncation.
 * n = 255 p <= 65025 and a are exact floats; for p <= a the product n * (1 / a) is within 255 * 2^-22 < 0.0001 of n / a, and n / a is an
 * integer or lies between 1 / 255 above one and 1 / 255 below the next.  Adding 0.002 -- more than the error, less than 1 / 255 less the
 * error -- therefore lifts an integer quotient over its integer and no other over the next: the truncated sum is the quotient.  Every
 * (p, a) is checked against the integer division on the CPU and on the device. */
__host__ __device__ inline uint32_t alpha_unpremultiply(uint32_t p, uint32_t a)
{
    const float r = 1.0f / (float)(a ? a : 1u);
    const float prod = (float)(255u * p) * r; /* built with -ffp-contract=off: product and sum round separately */
    const uint32_t q = (uint32_t)(prod + 0.002f);
    return a == 0u ? 0u : (q < 255u ? q : 255u);
}

/* over the background byte g: a straight source, a premultiplied source (p <= a: at most 255; saturates otherwise) */
__host__ __device__ inline uint32_t alpha_over_straight(uint32_t c, uint32_t a, uint32_t g) { return alpha_div255(c * a + g * (255u - a)); }
__host__ __device__ inline uint32_t alpha_over_premultiplied(uint32_t p, uint32_t a, uint32_t g)
{
    const uint32_t v = p + alpha_div255(g * (255u - a));
    return v < 255u ? v : 255u;
}

/* a straight BGRA pixel (B in the low byte) premultiplied: what the resize stages into its LDS row */
__host__ __device__ inline uint32_t alpha_premultiply_pixel(uint32_t px)
{
    const uint32_t a = px >> 24;
    return alpha_premultiply(px & 0xffu, a) | alpha_premultiply((px >> 8) & 0xffu, a) << 8 | alpha_premultiply((px >> 16) & 0xffu, a) << 16 | a << 24;
}

#endif
