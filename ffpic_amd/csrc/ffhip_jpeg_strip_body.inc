/* ffhip_jpeg_strip_body.inc -- the body of the fused strip kernels (4:4:4, 4:2:2, 4:4:0, 4:1:1 and its transpose, grey;
 * ffhip_jpeg.hip), included inside k_jpeg_fused_strip and, with FFHIP_JPEG_ITEMS defined, inside k_jpeg_fused_strip_items.
 * Shared as text for the reason ffhip_jpeg420_body.inc gives. */
    constexpr int BPM = H * V;                            /* luma blocks per MCU          */
    constexpr int MPS = ((NC == 1 || BPM == 1) ? 8 : 4) * ((TWO && BPM < 4) ? 2 : 1); /* MCUs per strip (of a wave) */
    constexpr int LR = MPS * BPM / 8;                    /* luma rounds: 4:1:1 and its transpose take TWO strips' worth of luma per wave (1 024 pixels), so that
                                                            their one chroma round (4 U + 4 V blocks) has no idle block -- 1.5 rounds per 512 pixels where the
                                                            single strip took 2 -- and the transpose's rows are runs of 128 bytes, not 64 */
    constexpr int PASSES = 2 * LR;                       /* colour passes of 256 pixels */
    constexpr int SW = MPS * 8 * H, SH = 8 * V;          /* strip size in pixels (512; h * v = 4 or TWO: 1024) */
    constexpr int CW = MPS * 8;                          /* chroma samples per strip row */
    constexpr int GPR = SW / 4;                          /* 4-pixel groups per pixel row */
    constexpr int RPP = 64 / GPR;                        /* lane rows per pass */
    static_assert((LR == 1 || LR == 2) && SW * SH == 512 * LR && BPM <= 4 && BPM != 3 && (H == 1 || V == 1), "strip geometry");
    /* the sample planes in the wave's LDS behind the 1 KB work tile: luma SW x SH, then U and V (8 rows of CW) */
    constexpr int CPB = CW * 8 * 2;                      /* bytes of a chroma plane */
    constexpr int YP = SM_YP, UP = YP + SW * SH * 2, VP = UP + ((LR == 1 && CPB < 1024) ? 1024 : CPB);
    constexpr int WAVE_LDS = NC == 3 ? VP + CPB : UP;
    constexpr int WAVE_BYTES = WAVE_LDS <= SM_WAVE_BYTES ? SM_WAVE_BYTES : (WAVE_LDS + 1023) / 1024 * 1024; /* 4 KB as ever; TWO: 4:4:4 7 KB, 4:2:2 / 4:4:0 5 KB */
    static_assert(UP == SM_UP || LR == 2, "plane offsets");
    __shared__ __attribute__((aligned(16))) char lds_all[WAVES_PER_WG * WAVE_BYTES];
    const u32 lane = threadIdx.x & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef FFHIP_JPEG_ITEMS
    JpegBatch p;
    const int img = 0, wgi = jpeg_item_batch(items, p); /* the workgroup's item: its picture as a batch of one, pointers offset */
#else
    u32 wg;
    {
        wg = xcd_remap_wg(p.xcd_remap);
    }
    int img = (int)__umulhi(wg, p.wpi_magic), wgi = (int)wg - img * p.wgs_per_image; /* scalar */
    if (wgi < 0) { img--; wgi += p.wgs_per_image; }
    if (wgi >= p.wgs_per_image) { img++; wgi -= p.wgs_per_image; }
#endif
    const int sidx = (int)((u32)wgi * WAVES_PER_WG + wave);
    if (sidx >= p.quads_per_image) return; /* wave-uniform; no barriers in this kernel */
    int mrow = (int)__umulhi((u32)sidx, p.qpr_magic), scol = sidx - mrow * p.quads_per_row;
    if (scol < 0) { mrow--; scol += p.quads_per_row; }
    if (scol >= p.quads_per_row) { mrow++; scol -= p.quads_per_row; }
    const int mcu0 = scol * MPS, last = p.mcu_cols - 1;
    const int rem = last - mcu0 < MPS - 1 ? last - mcu0 : MPS - 1; /* MCUs of this strip that exist, minus one */

    WaveCtx c;
    wave_ctx_init(c, lds_all + wave * WAVE_BYTES, lane);
    const u32 row = lane & 7, lblk = lane >> 3;
    const long long mcu_base = ((long long)img * p.mcu_rows + mrow) * p.mcu_cols + mcu0; /* scalar */
    const uint16_t *qt = p.quant + (long long)img * p.quant_stride;

    /* ---- all loads up front: ragged strips re-read their last MCU, its pixels are never stored ---- */
    u32x4 ly[LR], lc0, lc1, lc2, lc3; /* (lc2, lc3: the second halves of U and V where a wave has sixteen MCUs of 4:4:4) */
#pragma unroll
    for (int lr = 0; lr < LR; lr++) {
        int m = ((int)lblk + 8 * lr) / BPM;
        m = m > rem ? rem : m;
        ly[lr] = load16<NT & 1>((const char *)(p.coef_y + (mcu_base + m) * (64 * BPM) + (((int)lblk + 8 * lr) % BPM) * 64 + row * 8));
    }
    const u32x4 q_y = *(const u32x4 *)(qt + p.qt_y * 64 + row * 8);
    u32x4 q_c0 = q_y, q_c1 = q_y;
    if (NC == 3) {
        if (MPS >= 8) { /* rounds of 8 blocks: U, then V (sixteen MCUs: two of each) */
            const int m = (int)lblk > rem ? rem : (int)lblk;
            lc0 = load16<NT & 1>((const char *)(p.coef_u + (mcu_base + m) * 64 + row * 8));
            lc1 = load16<NT & 1>((const char *)(p.coef_v + (mcu_base + m) * 64 + row * 8));
            if (MPS == 16) {
                const int m2 = (int)lblk + 8 > rem ? rem : (int)lblk + 8;
                lc2 = load16<NT & 1>((const char *)(p.coef_u + (mcu_base + m2) * 64 + row * 8));
                lc3 = load16<NT & 1>((const char *)(p.coef_v + (mcu_base + m2) * 64 + row * 8));
            }
            q_c0 = *(const u32x4 *)(qt + p.qt_u * 64 + row * 8);
            q_c1 = *(const u32x4 *)(qt + p.qt_v * 64 + row * 8);
        } else {        /* one round: blocks 0-3 = U of MCU 0-3, blocks 4-7 = V */
            int m = (int)(lblk & 3);
            m = m > rem ? rem : m;
            lc0 = load16<NT & 1>((const char *)((lane < 32 ? p.coef_u : p.coef_v) + (mcu_base + m) * 64 + row * 8));
            q_c0 = *(const u32x4 *)(qt + (lane < 32 ? p.qt_u : p.qt_v) * 64 + row * 8);
        }
    }

    /* ---- IDCT rounds -> sample planes in LDS: luma SH rows x SW, chroma 8 rows x CW (int16).  The 16-byte chunks of a
     * plane row are XOR-swizzled by the row (sw_off) so that the block-row writes here (lanes of one block are 8 rows
     * apart at the same chunk) and the row-segment reads of the colour passes both touch every bank once: laid out
     * plainly, the writes were 4-way bank conflicts (175 M conflict cycles per launch at 4:4:4, profiles/r1_jpeg_geoms_pmc.txt) ---- */
    /* v = 2: the colour passes take rows 2j (pass 0) and 2j + 1 (pass 1) on the same lane, so that the chroma terms the
     * two rows share are computed once; the luma plane keeps the even rows first, then the odd ones, which keeps the
     * four rows a pass reads at once in four different bank quarters */
    auto yrow_pos = [](u32 r) -> u32 { return (r >> 1) + 8 * (r & 1u); };
    auto sw_off = [](u32 row, u32 col, u32 row_samples) -> u32 { /* byte offset of sample (row, col) in a swizzled plane */
        const u32 key = row_samples >= 64 ? (row & 7u) : ((row >> 2) & 3u);
        return row * row_samples * 2 + ((((col >> 3) ^ key) & (row_samples / 8 - 1)) << 4) + (col & 7u) * 2;
    };
    u32x4 pat = {0u, 0u, 0u, 0u}; /* PATTERN: what gets stored -- an XOR of everything the wave loaded */
    if (PATTERN) {
#pragma unroll
        for (int lr = 0; lr < LR; lr++) pat = pat ^ ly[lr];
        if (NC == 3) pat = pat ^ lc0;
        if (NC == 3 && MPS >= 8) pat = pat ^ lc1;
        if (NC == 3 && MPS == 16) pat = pat ^ lc2 ^ lc3;
    }
#pragma unroll
    for (int lr = 0; lr < LR && !PATTERN; lr++) {
        const u32x4 pk = idct8x8_round(c, ly[lr], q_y);
        const u32 gb = c.blk + 8 * lr, m = gb / BPM, sub = gb % BPM;
        const u32 pcol = (m * H + (H > 1 ? sub : 0)) * 8, prow = (V > 1 ? sub : 0) * 8 + c.idx;
        *(u32x4 *)(c.lds + YP + sw_off(V == 2 ? yrow_pos(prow) : prow, pcol, SW)) = pk;
    }
    if (NC == 3 && !PATTERN) {
        if (MPS >= 8) {
            const u32x4 pu = idct8x8_round(c, lc0, q_c0);
            *(u32x4 *)(c.lds + UP + sw_off(c.idx, c.blk * 8, CW)) = pu;
            const u32x4 pv = idct8x8_round(c, lc1, q_c1);
            *(u32x4 *)(c.lds + VP + sw_off(c.idx, c.blk * 8, CW)) = pv;
            if (MPS == 16) {
                const u32x4 pu2 = idct8x8_round(c, lc2, q_c0);
                *(u32x4 *)(c.lds + UP + sw_off(c.idx, (c.blk + 8) * 8, CW)) = pu2;
                const u32x4 pv2 = idct8x8_round(c, lc3, q_c1);
                *(u32x4 *)(c.lds + VP + sw_off(c.idx, (c.blk + 8) * 8, CW)) = pv2;
            }
        } else {
            const u32x4 pc = idct8x8_round(c, lc0, q_c0);
            if (MPS == 4 || (c.blk & 3) < MPS) /* h*v = 4: blocks 2, 3, 6, 7 of the round are repeats of the strip's last MCU */
                *(u32x4 *)(c.lds + (c.blk < 4 ? UP : VP) + sw_off(c.idx, (c.blk & 3) * 8, CW)) = pc;
        }
    }

    /* ---- colour: 2 passes x 4 pixels per lane; 4/H chroma samples serve them.  Same packed form as the 4:2:0 kernel:
     * per pixel PAIR three 16-bit adds, three saturating packs and three byte permutes ---- */
    uint8_t *const obase = p.bgra + (long long)img * p.image_stride + (long long)mrow * SH * p.pitch + (long long)mcu0 * (32 * H);
    TermBits grey_t = {};
    if (NC == 1) grey_t = chroma_term_bits(0u, 0u); /* U = V = 0 planes (jpg.c:501,552-554): uu = vv = -128, never "sensitive" */
    u32 tr2[2], tg2[2], tb2[2], us[2] = {0, 0}, vs[2] = {0, 0}, sens = 0;
    /* per-lane LDS offsets of the two passes, computed once: pass 1 reads 64 / GPR rows (v = 2: 8 row positions) further
     * on, which flips one bit of the swizzle key -- an XOR and an add instead of a second address computation */
    const u32 row0 = V >= 2 ? 2 * (lane / GPR) : lane / GPR, pc0 = (lane % GPR) * 4;
    const u32 y_off0 = sw_off(V == 2 ? yrow_pos(row0) : row0, pc0, SW);
    /* v = 4: rows 2j and 2j + 1 share (row >> 2), i.e. the swizzle key: the next plane row, 32 bytes on */
    const u32 y_off1 = SW == 64 ? (y_off0 ^ 0x40u) + 4 * 128 : (SW == 32 ? (y_off0 ^ 0x20u) + 8 * 64 : y_off0 + 32);
    static_assert((SW == 64 && 64 / GPR == 4 && V == 1) || (SW == 32 && V == 2) || LR == 2, "pass-1 offset identities");
    /* the pixel row of pass `it`.  v = 1: RPP lane rows a pass, one below the other (128 x 8 pixels: two rows a pass, four passes).  v >= 2: a lane takes rows
     * 2j and 2j + 1 in two passes running (they share their chroma row), RPP such pairs a pass pair -- the transpose of 4:1:1 (32 x 32): the upper half, then the
     * lower half; two strips of 4:4:0 (64 x 16): rows 0-7, then 8-15 */
    auto pass_row = [&](int it) -> u32 {
        return V >= 2 ? row0 + (u32)(it & 1) + (u32)(2 * RPP * (it >> 1)) : row0 + (u32)(it * RPP);
    };
    u32 y_offs[PASSES], c_offs[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; it++) {
        y_offs[it] = LR == 2 ? sw_off(V == 2 ? yrow_pos(pass_row(it)) : pass_row(it), pc0, SW) : (it ? y_off1 : y_off0); /* (four passes: worked out pass by pass) */
        c_offs[it] = 0;
    }
    const u32 c_off0 = NC == 3 ? sw_off(row0 / V, pc0 / H, CW) : 0;
    /* v = 1: pass 1 is four rows down -- one bit of the key flips and four chroma rows (CW samples each) are skipped */
    const u32 c_off1 = V >= 2 ? c_off0 : (CW == 64 ? (c_off0 ^ 0x40u) + 4 * 128 : (c_off0 ^ 0x10u) + 4 * CW * 2);
#pragma unroll
    for (int it = 0; it < PASSES; it++) c_offs[it] = (LR == 2 && NC == 3) ? sw_off(pass_row(it) / V, pc0 / H, CW) : (it ? c_off1 : c_off0);
#pragma unroll
    for (int it = 0; it < PASSES; it++) {
        const u32 prow = pass_row(it);
        if (PATTERN) { /* the pass's store, at its address and under its mask */
            if (mcu0 + (int)(pc0 / (8 * H)) <= last) {
                u32x4 *dst = (u32x4 *)(obase + (long long)prow * p.pitch + pc0 * 4);
                if (NT & 2) __builtin_nontemporal_store(pat + (u32)it, dst);
                else *dst = pat + (u32)it;
            }
            continue;
        }
        const u32x2 yy = *(const u32x2 *)(c.lds + YP + y_offs[it]);
        if (V >= 2 && (it & 1)) {
            /* the terms of pass 0 serve this row too */
        } else if (NC == 1) {
            tr2[0] = tr2[1] = __builtin_amdgcn_perm(grey_t.r, grey_t.r, 0x01000100u);
            tg2[0] = tg2[1] = __builtin_amdgcn_perm(grey_t.g, grey_t.g, 0x01000100u);
            tb2[0] = tb2[1] = __builtin_amdgcn_perm(grey_t.b, grey_t.b, 0x01000100u);
        } else {
            const u32 c_off = c_offs[it];
            if (H == 1) {
                const u32x2 a = *(const u32x2 *)(c.lds + UP + c_off), b = *(const u32x2 *)(c.lds + VP + c_off);
                us[0] = a[0]; us[1] = a[1]; vs[0] = b[0]; vs[1] = b[1];
            } else if (H == 2) {
                us[0] = *(const u32 *)(c.lds + UP + c_off);
                vs[0] = *(const u32 *)(c.lds + VP + c_off);
                us[1] = vs[1] = 0;
            } else { /* h = 4: the lane's four pixels share one chroma sample */
                us[0] = *(const uint16_t *)(c.lds + UP + c_off);
                vs[0] = *(const uint16_t *)(c.lds + VP + c_off);
                us[1] = vs[1] = 0;
            }
            sens = 0;
            if (H == 4) {
                const TermBits t = chroma_term_bits(us[0], vs[0]);
                sens = t.sens ? 1u : 0u;
                tr2[0] = tr2[1] = __builtin_amdgcn_perm(t.r, t.r, 0x01000100u);
                tg2[0] = tg2[1] = __builtin_amdgcn_perm(t.g, t.g, 0x01000100u);
                tb2[0] = tb2[1] = __builtin_amdgcn_perm(t.b, t.b, 0x01000100u);
            } else {
                constexpr int NP = H == 1 ? 2 : 1; /* sample pairs: two at h = 1, one at h = 2 */
                TermBits2 t[NP];
#pragma unroll
                for (int k = 0; k < NP; k++) t[k] = chroma_term_bits2(us[k], vs[k]);
                float any;
                if (H == 1) {
                    const f32x2 m = t[0].rem * t[NP - 1].rem;
                    any = m.x * m.y;
#pragma unroll
                    for (int h2 = 0; h2 < 2; h2++) { /* one chroma sample per pixel */
                        tr2[h2] = t[h2 % NP].r;
                        tg2[h2] = t[h2 % NP].g;
                        tb2[h2] = t[h2 % NP].b;
                    }
                } else {
                    any = t[0].rem.x * t[0].rem.y;
                    tr2[0] = __builtin_amdgcn_perm(t[0].r, t[0].r, 0x01000100u); /* a pixel pair shares its chroma sample */
                    tr2[1] = __builtin_amdgcn_perm(t[0].r, t[0].r, 0x03020302u);
                    tg2[0] = __builtin_amdgcn_perm(t[0].g, t[0].g, 0x01000100u);
                    tg2[1] = __builtin_amdgcn_perm(t[0].g, t[0].g, 0x03020302u);
                    tb2[0] = __builtin_amdgcn_perm(t[0].b, t[0].b, 0x01000100u);
                    tb2[1] = __builtin_amdgcn_perm(t[0].b, t[0].b, 0x03020302u);
                }
                if (any == 0.0f) { /* rare: some sample's G sum is a multiple of 1000 (zero included) */
#pragma unroll
                    for (int k = 0; k < 2 * NP; k++) {
                        const float rem = (k & 1) ? t[k >> 1].rem.y : t[k >> 1].rem.x, sf = (k & 1) ? t[k >> 1].sf.y : t[k >> 1].sf.x;
                        sens |= (rem == 0.0f && sf != 76288.0f) ? 1u << k : 0u;
                    }
                }
            }
        }
        u32x4 px;
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
            const u32 y2 = yy[h2];
            const u32 r2 = sat_pk_u8_i16(pk_add16(y2, tr2[h2]));
            const u32 g2 = sat_pk_u8_i16(pk_add16(y2, tg2[h2]));
            const u32 b2 = sat_pk_u8_i16(pk_add16(y2, tb2[h2]));
            const u32 bg = __builtin_amdgcn_perm(g2, b2, 0x05010400u); /* b0 g0 b1 g1 */
            px[2 * h2] = __builtin_amdgcn_perm(r2, bg, 0x0d040100u);     /* b0 g0 r0 ff */
            px[2 * h2 + 1] = __builtin_amdgcn_perm(r2, bg, 0x0d050302u); /* b1 g1 r1 ff */
        }
        if (NC == 3 && sens) { /* rare: exact-integer G decided by the fp64 roundings */
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const int k = d / H;
                if (sens & (1u << k)) {
                    const int y1 = (int)((d & 1) ? (yy[d >> 1] >> 16) : (yy[d >> 1] & 0xffffu));
                    const u32 ua = (k & 1) ? (us[k >> 1] >> 16) : (us[k >> 1] & 0xffffu); /* raw samples: uu = u - 128 (colorspace.c:149) */
                    const u32 va = (k & 1) ? (vs[k >> 1] >> 16) : (vs[k >> 1] & 0xffffu);
                    px[d] = (px[d] & 0xffff00ffu) | (green_fp64(y1, (int)ua - 128, (int)va - 128) << 8);
                }
            }
        }
        if (mcu0 + (int)(pc0 / (8 * H)) <= last) {
            u32x4 *dst = (u32x4 *)(obase + (long long)prow * p.pitch + pc0 * 4);
            if (NT & 2) __builtin_nontemporal_store(px, dst);
            else *dst = px;
        }
    }
