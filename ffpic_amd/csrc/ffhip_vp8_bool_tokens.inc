/* ffhip_vp8_bool_tokens.inc -- vp8_get_coefficients (webp.c:992-1064) without its dequantising multiply: the LEVELS at their raster position in
 * out[16].  probs: the 8 bands x 3 contexts x 11 probabilities of the block's type.  Included as text by ffhip_vp8_bool.h once per WebpPixelRule
 * with FFB_COEF_NAME, FFB_TOKENS_NAME (the two functions) and FFB_COEF_RULE (the rule, a literal) defined: the reference's instances keep the names and the parameter
 * lists they had before the second rule existed, because the category table is a static of it and that table's symbol name, which holds both, stands
 * in the listings of kernels that are held to their code. */
FFB_FN int FFB_COEF_NAME(ffb_dec *d, const uint8_t *probs, int first, int ctx, int16_t *out)
{
    FFB_TBL uint8_t pcat[4][12] = {{173, 148, 140, 0}, {176, 155, 140, 135, 0}, {180, 157, 141, 134, 130, 0},
                                   {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0}};
    const uint64_t bands = 0x7666666665463210ull;  /* coeff_bands[16], a nibble each (webp.c:1129) */
    const uint64_t zigzag = 0xfeb7adc963258410ull; /* kZigzag[16] (webp.c:1013) */
    int prev_zero = 0;
    for (int n = first; n < 16; ++n) {
        const uint8_t *p = probs + (int)((bands >> (4 * n)) & 15) * 33 + ctx * 11;
        int v;
        if (!prev_zero && !ffb_bit(d, p[0])) return n - first; /* dct_eob; not coded behind a zero */
        if (!ffb_bit(d, p[1])) {
            prev_zero = 1;
            ctx = 0;
            continue; /* out[] was cleared by the caller */
        }
        prev_zero = 0;
        if (!ffb_bit(d, p[2])) {
            v = 1;
        } else if (!ffb_bit(d, p[3])) {
            if (!ffb_bit(d, p[4])) v = 2;
            else v = 3 + ffb_bit(d, p[5]);
        } else if (!ffb_bit(d, p[6])) {
            if (!ffb_bit(d, p[7])) {
                v = 5 + ffb_bit(d, 159); /* cat1 */
            } else {
                v = 7 + 2 * ffb_bit(d, 165); /* cat2 */
                v += ffb_bit(d, 145);
            }
        } else {
            const int b1 = ffb_bit(d, p[8]);
            const int cat = 2 * b1 + ffb_bit(d, p[9 + b1]); /* 0..3 = cat3..cat6 */
            uint32_t extra = 0;
            if (FFB_COEF_RULE == WEBP_RULE_LIBWEBP)
                for (const uint8_t *q = pcat[cat]; *q; ++q) extra = 2 * extra + (uint32_t)ffb_bit(d, *q); /* cat6's eleven bits as they are */
            else
                for (const uint8_t *q = pcat[cat]; *q; ++q) extra = (2 * extra + (uint32_t)ffb_bit(d, *q)) & 255u; /* a uint8_t in the reference */
            v = (int)extra + (cat == 0 ? 11 : cat == 1 ? 19 : cat == 2 ? 35 : 67);
        }
        ctx = v == 1 ? 1 : 2;
        if (ffb_bit(d, 128)) v = -v;
        out[(zigzag >> (4 * n)) & 15] = (int16_t)v;
    }
    return 16;
}


/* The token parse of one coded macroblock (webp.c:1147-1196).  probs [4][8][3][11]; *top9 / *left9: the nine "had tokens" flags
 * of the column above / of the row so far, bit 0 the Y2 block, 1-4 luma, 5-6 U, 7-8 V; levels [25][16] must be ZERO on entry
 * (only non-zero levels are stored), counts [25] receives every block's token count. */
FFB_FN void FFB_TOKENS_NAME(ffb_dec *d, const uint8_t *probs, int has_y2, uint32_t *top9, uint32_t *left9, int16_t *levels, uint8_t *counts)
{
    uint32_t top = *top9, left = *left9;
    int first = 0;
    const uint8_t *yp = probs + 3 * 264;
    if (has_y2) {
        const int nz = FFB_COEF_NAME(d, probs + 264, 0, (int)(top & 1) + (int)(left & 1), levels + 24 * 16);
        counts[24] = (uint8_t)nz;
        top = (top & ~1u) | (nz > 0);
        left = (left & ~1u) | (nz > 0);
        first = 1;
        yp = probs;
    } else {
        counts[24] = 0;
    }
    for (int y = 0; y < 4; ++y) {
        uint32_t l = (left >> (y + 1)) & 1;
        for (int x = 0; x < 4; ++x) {
            const int nz = FFB_COEF_NAME(d, yp, first, (int)((top >> (x + 1)) & 1) + (int)l, levels + (y * 4 + x) * 16);
            counts[y * 4 + x] = (uint8_t)nz;
            l = nz > 0;
            top = (top & ~(2u << x)) | (l << (x + 1));
        }
        left = (left & ~(2u << y)) | (l << (y + 1));
    }
    int blk = 16;
    for (int ch = 5; ch <= 7; ch += 2)
        for (int y = 0; y < 2; ++y) {
            uint32_t l = (left >> (y + ch)) & 1;
            for (int x = 0; x < 2; ++x, ++blk) {
                const int nz = FFB_COEF_NAME(d, probs + 2 * 264, 0, (int)l + (int)((top >> (x + ch)) & 1), levels + blk * 16);
                counts[blk] = (uint8_t)nz;
                l = nz > 0;
                top = (top & ~(1u << (x + ch))) | (l << (x + ch));
            }
            left = (left & ~(1u << (y + ch))) | (l << (y + ch));
        }
    *top9 = top;
    *left9 = left;
}
