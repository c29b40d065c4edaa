/* ffhip_vp8_libwebp_body.h -- the arithmetic of WEBP_RULE_LIBWEBP behind the bool decoder, written once for the kernels
 * (k_vp8_residual_items_libwebp in ffhip_vp8_libwebp.hip, k_vp8_upsample_color there too) and for the two host entries that let a machine
 * without a device hold it to the witness (ffhip_vp8_libwebp_residual_mb, ffhip_webp_libwebp_color): RFC 6386 sections 14.1 - 14.4 as
 * `_residual`, `_iwht` and `_idct` of tests/vp8_spec.py have them, and libwebp's fancy upsampler and colour step as `_upsample_row` and `to_rgb`
 * have them.  Plain integer C, no tables. */
#ifndef FFHIP_VP8_LIBWEBP_BODY_H
#define FFHIP_VP8_LIBWEBP_BODY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LW_FN __host__ __device__ static inline
#else
#define LW_FN static inline
#endif

LW_FN int lw_i16(int v) { return (int)(int16_t)(uint16_t)(unsigned)v; } /* the int16 store of a dequantised coefficient and of a Y2-derived DC */

/* the two constants of section 14.3; the second pass sees sums beyond 16 bits (the first pass is plain int under this rule), so the products
 * are 64-bit */
LW_FN int lw_mul1(int x) { return x + (int)(((long long)x * 20091) >> 16); }
LW_FN int lw_mul2(int x) { return (int)(((long long)x * 35468) >> 16); }

/* section 14.3, vertical pass first: c[16] -> o[16] */
LW_FN void lw_idct(const int *c, int *o)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
        const int cc = lw_mul2(c[4 + i]) - lw_mul1(c[12 + i]), dd = lw_mul1(c[4 + i]) + lw_mul2(c[12 + i]);
        t[i] = a + dd; t[4 + i] = b + cc; t[8 + i] = b - cc; t[12 + i] = a - dd;
    }
    for (int r = 0; r < 4; r++) {
        const int x0 = t[4 * r], x1 = t[4 * r + 1], x2 = t[4 * r + 2], x3 = t[4 * r + 3];
        const int a = x0 + x2, b = x0 - x2;
        const int cc = lw_mul2(x1) - lw_mul1(x3), dd = lw_mul1(x1) + lw_mul2(x3);
        o[4 * r] = (a + dd + 4) >> 3; o[4 * r + 1] = (b + cc + 4) >> 3; o[4 * r + 2] = (b - cc + 4) >> 3; o[4 * r + 3] = (a - dd + 4) >> 3;
    }
}

/* the Y2 block -> the DC of luma block `blk` (section 14.3's inverse WHT, then the int16 store): y2[16] levels, q_dc / q_ac its factors */
LW_FN int lw_y2_dc(const int16_t *y2, int q_dc, int q_ac, int blk)
{
    int c[16], t[16];
    for (int i = 0; i < 16; i++) c[i] = lw_i16((int)y2[i] * (i ? q_ac : q_dc));
    for (int i = 0; i < 4; i++) {
        const int a0 = c[i] + c[12 + i], a1 = c[4 + i] + c[8 + i], a2 = c[4 + i] - c[8 + i], a3 = c[i] - c[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
    int out = 0;
    for (int r = 0; r < 4; r++) {
        const int x0 = t[4 * r], x1 = t[4 * r + 1], x2 = t[4 * r + 2], x3 = t[4 * r + 3];
        const int a0 = x0 + x3, a1 = x1 + x2, a2 = x1 - x2, a3 = x0 - x3;
        const int o[4] = {(a0 + a1 + 3) >> 3, (a3 + a2 + 3) >> 3, (a0 - a1 + 3) >> 3, (a3 - a2 + 3) >> 3};
        for (int k = 0; k < 4; k++)
            if (4 * r + k == blk) out = o[k];
    }
    return lw_i16(out);
}

/* One 4x4 block: lv[16] levels at their raster positions, its factors, and -- for a luma block of a macroblock with a Y2 block -- the DC
 * that replaces its own.  res[16] gets the residual (zeros when there is nothing to transform: no lone-AC shortcut, every block with a non-zero
 * coefficient goes through the IDCT).  Returns whether the block has a non-zero dequantised coefficient. */
LW_FN int lw_block(const int16_t *lv, int q_dc, int q_ac, int has_dc, int dc, int16_t *res)
{
    int c[16], o[16], any = 0;
    for (int i = 0; i < 16; i++) c[i] = lw_i16((int)lv[i] * (i ? q_ac : q_dc));
    if (has_dc) c[0] = dc;
    for (int i = 0; i < 16; i++) any |= c[i];
    if (!any) {
        for (int i = 0; i < 16; i++) res[i] = 0;
        return 0;
    }
    lw_idct(c, o);
    /* crafted coefficients reach +-60 000 here; the residual is int16 and SATURATES, which the prediction's add-and-clip to 8 bits cannot tell
     * from the int (a sample plus anything beyond +-255 is 0 or 255 either way) */
    for (int i = 0; i < 16; i++) res[i] = (int16_t)(o[i] < -32768 ? -32768 : (o[i] > 32767 ? 32767 : o[i]));
    return 1;
}

/* the factors of block b (0-15 Y, 16-23 U / V) out of q[6] = y1_dc, y1_ac, y2_dc, y2_ac, uv_dc, uv_ac */
LW_FN int lw_block_qdc(const uint16_t *q, int b) { return b < 16 ? q[0] : q[4]; }
LW_FN int lw_block_qac(const uint16_t *q, int b) { return b < 16 ? q[1] : q[5]; }

/* ---- colour ---- */
/* clip8(v >> 6), written clamp first, shift second (16383 >> 6 = 255).  Shift-then-clamp of two neighbouring bytes is what hipcc makes
 * v_ashr_pk_u8_i32 of on gfx950, and the OR that put the third byte above that pair found bits 16-31 set whenever the pair's first value was
 * negative: on the device R came out 255 wherever B clipped to 0.  This form has no such pattern and the same value. */
LW_FN int lw_clip8_q6(int v) { return (v < 0 ? 0 : (v > 16383 ? 16383 : v)) >> 6; }

/* libwebp's 14-bit fixed point: y, u, v -> the BGRA dword (alpha 255, as the default rule writes it) */
LW_FN uint32_t lw_pixel(int y, int u, int v)
{
    const int yy = (19077 * y) >> 8;
    const int r = lw_clip8_q6(yy + ((26149 * v) >> 8) - 14234);
    const int g = lw_clip8_q6(yy - ((6419 * u) >> 8) - ((13320 * v) >> 8) + 8708);
    const int b = lw_clip8_q6(yy + ((33050 * u) >> 8) - 17685);
    return (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16 | 0xff000000u;
}

/* the chroma row further away from picture row r, of ch chroma rows: the one above an even row, the one below an odd row, the row itself at the
 * top, clamped at the bottom (the last row of a picture of even height has no chroma row below it) */
LW_FN int lw_far_row(int r, int ch)
{
    const int near = r >> 1;
    const int far = r == 0 ? near : ((r & 1) ? near + 1 : near - 1);
    return far < ch - 1 ? far : ch - 1;
}

/* the upsampled chroma of pixel x of a row of w pixels: n / f = the chroma row nearer to the picture row / further away (9-3-3-1 over the four
 * samples around the pixel, in libwebp's two-step rounding; the first pixel, and the last one of an even width, have two samples: 3-1) */
LW_FN int lw_upsample(const uint8_t *n, const uint8_t *f, int x, int w)
{
    if (x == 0) return (3 * n[0] + f[0] + 2) >> 2;
    const int k = (x + 1) >> 1;
    if (k > ((w - 1) >> 1)) return (3 * n[k - 1] + f[k - 1] + 2) >> 2; /* x = w - 1, w even */
    const int s = n[k - 1] + n[k] + f[k - 1] + f[k] + 8;
    if (x & 1) return (((s + 2 * (n[k] + f[k - 1])) >> 3) + n[k - 1]) >> 1;
    return (((s + 2 * (n[k - 1] + f[k])) >> 3) + n[k]) >> 1;
}

/* The same for the four pixels x0 .. x0 + 3 (x0 a multiple of 4, x0 + 4 <= w) at once, from the two rows' samples x0 / 2 - 1 .. x0 / 2 + 2 packed a
 * byte each into n4 and f4, lowest byte first: what the kernel has after two aligned dword loads per row.  Bytes that stand for samples outside
 * the row (the first of x0 = 0, the last where x0 + 3 = w - 1) are never looked at: those pixels take the two-sample form. */
LW_FN void lw_upsample4(uint32_t n4, uint32_t f4, int x0, int w, int *out)
{
    const uint8_t n[4] = {(uint8_t)n4, (uint8_t)(n4 >> 8), (uint8_t)(n4 >> 16), (uint8_t)(n4 >> 24)};
    const uint8_t f[4] = {(uint8_t)f4, (uint8_t)(f4 >> 8), (uint8_t)(f4 >> 16), (uint8_t)(f4 >> 24)};
    for (int k = 0; k < 4; k++) {
        const int a = (k + 1) >> 1;                                  /* pixel x0 + k lies between the samples n[a] and n[a + 1] */
        const int s = n[a] + n[a + 1] + f[a] + f[a + 1] + 8;
        out[k] = (k & 1) ? (((s + 2 * (n[a + 1] + f[a])) >> 3) + n[a]) >> 1 : (((s + 2 * (n[a] + f[a + 1])) >> 3) + n[a + 1]) >> 1;
    }
    if (x0 == 0) out[0] = (3 * n[1] + f[1] + 2) >> 2;
    if (x0 + 3 == w - 1) out[3] = (3 * n[2] + f[2] + 2) >> 2;         /* the last pixel of an even width */
}

/* four pixels from x0 (a multiple of 4, x0 + 4 <= w): y4 their luma, un4 .. vf4 the chroma windows of lw_upsample4 */
LW_FN void lw_color_run4(uint32_t y4, uint32_t un4, uint32_t uf4, uint32_t vn4, uint32_t vf4, int x0, int w, uint32_t *out)
{
    int u[4], v[4];
    lw_upsample4(un4, uf4, x0, w, u);
    lw_upsample4(vn4, vf4, x0, w, v);
    for (int k = 0; k < 4; k++) out[k] = lw_pixel((int)((y4 >> (8 * k)) & 255u), u[k], v[k]);
}
/* a row's chroma window for lw_upsample4 read sample by sample (the host's way; an index outside 0 .. cw - 1 stands for a byte that is never
 * looked at and is clamped) */
LW_FN uint32_t lw_window(const uint8_t *row, int x0, int cw)
{
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) {
        int i = (x0 >> 1) - 1 + k;
        i = i < 0 ? 0 : (i > cw - 1 ? cw - 1 : i);
        v |= (uint32_t)row[i] << (8 * k);
    }
    return v;
}

/* the pixels x0 .. x0 + count - 1 (count <= 4) of a picture row; yrun: their luma samples */
LW_FN void lw_color_run(const uint8_t *yrun, const uint8_t *un, const uint8_t *uf, const uint8_t *vn, const uint8_t *vf, int x0, int count, int w,
                        uint32_t *out)
{
    for (int k = 0; k < count; k++) out[k] = lw_pixel(yrun[k], lw_upsample(un, uf, x0 + k, w), lw_upsample(vn, vf, x0 + k, w));
}

#endif
