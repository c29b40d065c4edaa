/* ffhip_png_body.h -- the PNG pixel rule (include/ffpic_hip.h, "PNG") as the host decoder (ffhip_png.c) and the two kernels
 * (ffhip_png_gpu.hip) compile it: the five row filters on one byte of a filter unit, the Paeth predictor, one pixel of each of the 15 valid
 * (colour type, bit depth) pairs to a BGRA dword, and the Adam7 map.  Plain C without builtins, so that a C program can hold it against the
 * rule written another way.
 *
 * A filter unit is bpp = max(1, bits x channels / 8) bytes; byte k of unit x is predicted from byte k of the unit to the left (a), the one
 * above (b) and the one above left (c), each 0 outside the sub-image.  All sums are taken modulo 256. */
#ifndef FFHIP_PNG_BODY_H
#define FFHIP_PNG_BODY_H

#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define FFHIP_PNG_FN __host__ __device__ static inline

/* 0 for a (colour type, bit depth) pair PNG does not have */
FFHIP_PNG_FN int ffhip_png_channels(int ctype, int depth)
{
    const int d8 = depth == 8 || depth == 16, dlow = depth == 1 || depth == 2 || depth == 4;
    switch (ctype) {
    case 0: return d8 || dlow ? 1 : 0;
    case 2: return d8 ? 3 : 0;
    case 3: return dlow || depth == 8 ? 1 : 0;
    case 4: return d8 ? 2 : 0;
    case 6: return d8 ? 4 : 0;
    default: return 0;
    }
}

FFHIP_PNG_FN int ffhip_png_bpp(int ctype, int depth)
{
    const int bits = ffhip_png_channels(ctype, depth) * depth;
    return bits < 8 ? 1 : bits / 8;
}

/* the spec's order on ties: a, then b, then c */
FFHIP_PNG_FN int ffhip_png_paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

/* one byte: filter type 0..4 (the caller has refused anything else), the filtered byte and its three neighbours -> the byte */
FFHIP_PNG_FN int ffhip_png_unfilter_byte(int ft, int raw, int a, int b, int c)
{
    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ffhip_png_paeth(a, b, c);
    return (raw + pred) & 255;
}

/* a sub-image's rows in place: `rows` rows of 1 + row_bytes bytes, the filter byte left alone */
FFHIP_PNG_FN void ffhip_png_unfilter_rows(uint8_t *sub, uint32_t rows, uint32_t row_bytes, int bpp)
{
    const uint64_t pitch = (uint64_t)row_bytes + 1;
    for (uint32_t y = 0; y < rows; y++) {
        uint8_t *cur = sub + y * pitch + 1;
        const uint8_t *up = y ? cur - pitch : 0;
        const int ft = cur[-1];
        for (uint32_t i = 0; i < row_bytes; i++) {
            const int a = i >= (uint32_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = up && i >= (uint32_t)bpp ? up[i - bpp] : 0;
            cur[i] = (uint8_t)ffhip_png_unfilter_byte(ft, cur[i], a, b, c);
        }
    }
}

/* What expansion needs of a file besides its rows.  key: the tRNS sample (grey) or triple (RGB), masked to the file's bit depth */
typedef struct ffhip_png_expand_rule {
    uint8_t ctype, depth, has_trns, interlace;
    uint16_t key[3];
} ffhip_png_expand_rule;

FFHIP_PNG_FN uint32_t ffhip_png_bgra(uint32_t b, uint32_t g, uint32_t r, uint32_t a) { return b | g << 8 | r << 16 | a << 24; }

/* sample i of a row of `depth`-bit samples (behind the filter byte), at the file's own depth: 16-bit samples big-endian */
FFHIP_PNG_FN uint32_t ffhip_png_sample(const uint8_t *row, uint64_t i, int depth)
{
    if (depth == 8) return row[i];
    if (depth == 16) return (uint32_t)row[2 * i] << 8 | row[2 * i + 1];
    const uint64_t bit = i * (uint64_t)depth;
    return (uint32_t)(row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1);
}

/* pixel px of an unfiltered row -> BGRA.  pal: 256 BGRA dwords with the tRNS alpha in them (colour type 3 only; entries beyond PLTE are
 * never read: the host refuses a file with such an index) */
FFHIP_PNG_FN uint32_t ffhip_png_pixel(const ffhip_png_expand_rule *r, const uint8_t *row, uint32_t px, const uint32_t *pal)
{
    const int d = r->depth, down = d == 16 ? 8 : 0;
    switch (r->ctype) {
    case 0: {
        const uint32_t v = ffhip_png_sample(row, px, d);
        const uint32_t g = d == 1 ? v * 255 : d == 2 ? v * 85 : d == 4 ? v * 17 : v >> down;
        return ffhip_png_bgra(g, g, g, r->has_trns && v == r->key[0] ? 0 : 255);
    }
    case 2: {
        const uint32_t R = ffhip_png_sample(row, 3ull * px, d), G = ffhip_png_sample(row, 3ull * px + 1, d), B = ffhip_png_sample(row, 3ull * px + 2, d);
        const int hit = r->has_trns && R == r->key[0] && G == r->key[1] && B == r->key[2];
        return ffhip_png_bgra(B >> down, G >> down, R >> down, hit ? 0 : 255);
    }
    case 3: return pal[ffhip_png_sample(row, px, d)];
    case 4: {
        const uint32_t g = ffhip_png_sample(row, 2ull * px, d) >> down;
        return ffhip_png_bgra(g, g, g, ffhip_png_sample(row, 2ull * px + 1, d) >> down);
    }
    default:
        return ffhip_png_bgra(ffhip_png_sample(row, 4ull * px + 2, d) >> down, ffhip_png_sample(row, 4ull * px + 1, d) >> down,
                              ffhip_png_sample(row, 4ull * px, d) >> down, ffhip_png_sample(row, 4ull * px + 3, d) >> down);
    }
}

/* Adam7: output pixel (x, y) -> its pass 0..6, and its column and row in that pass's sub-image */
FFHIP_PNG_FN int ffhip_png_adam7_of(uint32_t x, uint32_t y, uint32_t *px, uint32_t *py)
{
    if (y & 1) { *px = x; *py = y >> 1; return 6; }
    if (x & 1) { *px = x >> 1; *py = y >> 1; return 5; }
    if (y & 2) { *px = x >> 1; *py = y >> 2; return 4; }
    if (x & 2) { *px = x >> 2; *py = y >> 2; return 3; }
    if (y & 4) { *px = x >> 2; *py = y >> 3; return 2; }
    if (x & 4) { *px = x >> 3; *py = y >> 3; return 1; }
    *px = x >> 3; *py = y >> 3;
    return 0;
}

/* pass p of a width x height picture: its columns and rows, either may be 0 */
FFHIP_PNG_FN void ffhip_png_adam7_size(int p, uint32_t width, uint32_t height, uint32_t *pw, uint32_t *ph)
{
    const uint32_t xs = p == 1 ? 4 : p == 3 ? 2 : p == 5 ? 1 : 0, ys = p == 2 ? 4 : p == 4 ? 2 : p == 6 ? 1 : 0;
    const uint32_t dx = p < 2 ? 8 : p < 4 ? 4 : p < 6 ? 2 : 1, dy = p < 3 ? 8 : p < 5 ? 4 : 2;
    *pw = width > xs ? (width - xs + dx - 1) / dx : 0;
    *ph = height > ys ? (height - ys + dy - 1) / dy : 0;
}

#endif
