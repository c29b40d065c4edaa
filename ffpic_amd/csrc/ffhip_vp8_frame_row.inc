/* ffhip_vp8_frame_row.inc -- one macroblock row (row y of the frame, row g of the workgroup's share) of k_vp8_frames /
 * k_vp8_frames_items: fetch, prediction, loop filter, colour, the lines handed down and the progress counter.  Included as
 * text by both kernels (ffhip_vp8_frame.hip); the frame's geometry and pointers come from `a`, its image from `img`. */
        /* ONE buffer resource for the workgroup's line slots (round 6: one per slot in use were four scalar registers more in a kernel that spills
         * seventy); a slot is picked by the scalar offset, which the range check counts in (out of range: offset >= num_records - soffset): the first
         * row of a frame, which has no row above, reads "its" row above at soffset = num_records -- everything out of range, zeros, no traffic */
        const int me_off = (int)((unsigned)(g % a.nslot) * a.slot_bytes);
        const int up_off = y > 0 ? (int)((unsigned)((g + a.nslot - 1) % a.nslot) * a.slot_bytes) : (int)((unsigned)a.nslot * a.slot_bytes);
        const int yr = real_row ? y : a.mbrows - 1;
        const uint8_t *mrow = a.modes + ((long long)img * n_mb + (long long)yr * a.mbcols) * 20;
        const int32_t *maprow = MAP ? a.resmap + (long long)img * n_mb + (long long)yr * a.mbcols : nullptr;
        const __amdgpu_buffer_rsrc_t rRes = ffhip_rsrc(a.residual + (long long)img * a.res_stride,
                                                       (unsigned)(a.res_stride * 2 > 0xffffffffLL ? 0xffffffffLL : a.res_stride * 2));
        const __amdgpu_buffer_rsrc_t rMo = ffhip_rsrc(mrow, real_row ? 20u * (unsigned)a.mbcols : 0u);
        const __amdgpu_buffer_rsrc_t rOut = ffhip_rsrc(a.bgra + img * a.image_stride, (unsigned)(16 * a.mbrows) * (unsigned)a.pitch);
        const __amdgpu_buffer_rsrc_t rY = ffhip_rsrc(PLANES ? a.y + img * a.plane_y : nullptr, PLANES ? 256u * (unsigned)n_mb : 0u),
                                     rU = ffhip_rsrc(PLANES ? a.u + img * a.plane_uv : nullptr, PLANES ? 64u * (unsigned)n_mb : 0u),
                                     rV = ffhip_rsrc(PLANES ? a.v + img * a.plane_uv : nullptr, PLANES ? 64u * (unsigned)n_mb : 0u);
        const unsigned long long em_rows = y == 0 ? rows_first : (real_row ? ~0ull : ~rows_first);
        const unsigned long long pc_rows = y == 0 ? prow_first : (real_row ? pc_all : pc_all & ~prow_first);
        u32 seen = y == 0 ? 0x7fffffffu : 0u; /* macroblocks of the row above whose lines are known to be complete */

        struct Fetch { u32 res[3]; u32 mo; int pb; u32 lt; } f;
        f.res[0] = f.res[1] = f.res[2] = 0; f.mo = 0; f.pb = 0; f.lt = 0;
        /* everything macroblock x1 needs, issued a macroblock ahead; blocks only while the row above is not far enough */
        auto fetch = [&](int x1, long long rrow, u32 need) {
            int spins = 0;
            const u32 want = up_base + need;
            while (seen < want) {
                seen = (u32)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&PROG[wp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (seen >= want) break;
                /* (the row kernels of ffhip_vp8_pred.hip / ffhip_vp8_lf.hip wait the same way on device-coherent counters: another scope, sleep and limit) */
                /* A wait that runs out cannot happen (the row above belongs to a wave of this workgroup); a hang guard all the same.  It does NOT
                 * leave the kernel: the wave stops waiting -- here and, through the abort word, everywhere in the workgroup -- and goes on to the end
                 * with whatever it finds (the call reports FFHIP_EIO).  An exit from inside the macroblock loop would be one more way round it for
                 * the compiler's wait counts to allow for: with it, the wait for the fetched registers was a wait for the stores behind the fetch. */
                if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
                if (++spins > FR_SPIN_LIMIT) {
                    if (lane == 0) {
                        __hip_atomic_store(ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(a.async_err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    break;
                }
                if (spins < 16) __builtin_amdgcn_s_sleep(1);
                else __builtin_amdgcn_s_sleep(8);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            /* FOUR loads, whatever the row: the emission-only row below the picture reads them from outside their buffers (zeros, no traffic).
             * With a branch round them the compiler's wait for the fetched registers -- the minimum over the ways into the loop head -- became a
             * wait for everything in flight, the stores issued behind the fetch included */
            {
                const u32x3 r3 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(rRes, real_row ? lane * 12 : FR_OUT, (int)(rrow * 768), 0));
                f.res[0] = r3[0]; f.res[1] = r3[1]; f.res[2] = r3[2];
                f.mo = (u32)__builtin_amdgcn_raw_buffer_load_b32(rMo, (lane < 5 ? lane : 4) * 4, x1 * 20, 0);
                /* the row above's last pixel for the raw H_PRED read at x = 0; the rest of that column is not reconstructed yet and reads 0 */
                const int pbo = pb_off + x1 * pb_step;
#if FR_SPEC /* WEBP_RULE_LIBWEBP: no raw read; instead the right-most macroblock's four above-right lanes take the last sample above it */
                f.pb = (int)(unsigned char)__builtin_amdgcn_raw_buffer_load_b8(rL, lane >= 17 && lane <= 20 && x1 == a.mbcols - 1 ? off_ul + ys - 1 : pbo, up_off, FR_AUX_SC0);
#else
                f.pb = (int)(unsigned char)__builtin_amdgcn_raw_buffer_load_b8(rL, lane == 48 && x1 == 0 ? off_ul + ys - 1 : pbo, up_off, FR_AUX_SC0);
#endif
            }
            f.lt = (u32)__builtin_amdgcn_raw_buffer_load_b32(rL, lt_off + x1 * lt_step, up_off, FR_AUX_SC0);
        };
        auto map_load = [&](int x1) {
            int v;
            asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(maprow + x1) : "memory");
            return v;
        };
        int map_next = 0;
        if (MAP && real_row) map_next = map_load(0);
        auto res_row = [&](int x1) {
            long long r = (long long)yr * a.mbcols + x1;
            if (MAP) {
                r = (long long)map_next;
                if (x1 + 1 < a.mbcols) map_next = map_load(x1 + 1);
            }
            return r;
        };
        /* luma reads above-right, and the filter's top rows must have had the next macroblock's left-edge filter: x + 1 of the row above */
        auto need_of = [&](int x1) { return y == 0 ? 0u : (u32)(x1 + 2 < a.mbcols ? x1 + 2 : a.mbcols); };

        u32 mo[5] = {0, 0, 0, 0, 0};
        /* the fetched macroblock into the tiles: the prediction's borders in their final form (129 left of the picture, 127
         * above it and right of it, predict.c:433-437, 492-517; raw memory for V_PRED / H_PRED), the residual, the filter tiles'
         * new columns */
        auto consume = [&](const int x) {
            if (real_row) {
#pragma unroll
                for (int i = 0; i < 5; i++) mo[i] = (u32)__builtin_amdgcn_readlane((int)f.mo, i);
                const int ymode = (int)(mo[0] & 0xff);
#if FR_SPEC
                const bool raw = false; /* V_PRED and H_PRED take the 127 / 129 borders like the other modes */
                (void)ymode;
#else
                const bool raw = ymode == 2 || ymode == 3;
#endif
                const int carry = (int)BT[carry_src]; /* the previous macroblock's right column (unfiltered: the filter works on its own tile) */
                const unsigned long long none = 0ull;
                *(u32x3 *)((char *)R + lane * 12) = u32x3{f.res[0], f.res[1], f.res[2]};
                const unsigned long long m127 = (y == 0 ? (M_UTOP | M_VTOP | (raw ? none : M_LUMATOP)) : none) | ((!FR_SPEC && !raw && x == a.mbcols - 1) ? M_TOPRIGHT : none); /* (FR_SPEC: below row 0 the fetch brought the last sample above) */
                const unsigned long long m129 = (x == 0 ? (M_FIRST_CHROMA | (raw ? none : (M_FIRST_LUMA | M_LEFT))) : none) & ~m127;
                int v = f.pb;
                v = lane_select_smask(x != 0 ? M_LEFT : none, v, carry);
                v = lane_select_smask(m127, v, 127);
                v = lane_select_smask(m129, v, 129);
                BT[dst1] = (uint8_t)v;
                BT[dst2] = (uint8_t)(x == 0 ? 129 : carry);
            }
            FLDS32(lt_dst) = f.lt;
            wave_sync();
#if FR_SPEC /* above-right of sub-blocks 7, 11 and 15: the four samples above-right of the MACROBLOCK, where sub-block 3 gets them */
            if (lane < 12) T[(4 + 4 * (lane >> 2)) * PRS + 20 + (lane & 3)] = T[20 + (lane & 3)];
            wave_sync();
#endif
        };
        const int ymode0 = real_row ? __builtin_amdgcn_readfirstlane((int)mrow[0]) : 0;
        fetch(0, real_row ? res_row(0) : 0, (!FR_SPEC && real_row && y > 0 && ymode0 == 3) ? (u32)a.mbcols : need_of(0));
        consume(0);
        {   /* the loop's state at its head, from here as from its own end: one fetch in flight, the stores of a macroblock behind it (these go nowhere) */
            const int x1 = 1 < a.mbcols ? 1 : a.mbcols - 1;
            fetch(x1, real_row ? res_row(x1) : 0, need_of(x1));
            __builtin_amdgcn_raw_buffer_store_b32(0u, rL, FR_OUT, me_off, 0);
#if !FR_SPEC
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, rOut, FR_OUT, 0, 0);
#endif
            if (PLANES) {
                __builtin_amdgcn_raw_buffer_store_b32(0u, rY, FR_OUT, 0, 0);
                if (lane < 16) __builtin_amdgcn_raw_buffer_store_b32(0u, rU, FR_OUT, 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b32(0u, rV, FR_OUT, 0, 0);
            }
        }

        for (int x = 0; x <= a.mbcols; x++) {
            const bool real_mb = real_row && x < a.mbcols;
            int sub = 0, inter = 0, hevt = 0;
            bool inner = false;
            if (real_mb) {
                const int ymode = (int)(mo[0] & 0xff), uvmode = (int)((mo[0] >> 8) & 0xff);
                u32 lumaout = 0;
                int outc[2] = {0, 0};
                /* ---- luma ---- */
                const int r16 = lane >> 2, c16 = (lane & 3) * 4;
                if (ymode == 4) { /* B_PRED: the 16 sub-blocks in 10 dependent, branch-free steps (ffhip_vp8_pred.hip has the reasoning) */
                    static constexpr int SA[10] = {0, 1, 2, 3, 6, 7, 10, 11, 14, 15}, SB[10] = {0, 1, 4, 5, 8, 9, 12, 13, 14, 15};
                    const int l16 = lane & 15, r = l16 >> 2, c = l16 & 3;
                    const bool second = (lane & 16) != 0;
                    /* what a step needs that is not a sample -- the tap word of its sub-block's mode and the lane's residual -- is read ONE step ahead
                     * (two registers; held for all ten steps in six arrays, as until round 6, it was sixty, the kernel's register peak) */
                    auto sub_mode = [&](const int nb) { return FR_SUBMODE((int)((mo[(2 + nb) >> 2] >> (8 * ((2 + nb) & 3))) & 0xff)); };
                    auto step_mode = [&](const int t) { const int mA = sub_mode(SA[t]), mB = sub_mode(SB[t]); return second ? mB : mA; };
                    /* (the clamp of the mode depends on the instance, FR_SUBMODE: k_vp8_frames has none -- a record with a sub-block mode above 9 never gets
                     * there, the host's check or k_vp8_check_modes in front of the launch refuses the call, and the abort word is read at the kernel's start; a
                     * vector clamp was three instructions a step -- while k_vp8_frames_items clamps the scalar mode to 9, since an item's host copy is checked,
                     * not its device copy) */
                    const u32 *const TTl = TT + l16;
                    auto step_taps = [&](const int t) { return TTl[step_mode(t) * 16]; };
                    auto step_res = [&](const int t) { return (int)R[16 * (second ? SB[t] : SA[t]) + l16]; };
                    u32 to_n = step_taps(0);
                    int rv_n = step_res(0);
#pragma unroll
                    for (int t = 0; t < 10; t++) {
                        const u32 to = to_n;
                        const int rv = rv_n;
                        if (t + 1 < 10) { to_n = step_taps(t + 1); rv_n = step_res(t + 1); }
                        const int nA = SA[t], nB = SB[t];
                        const int oA = ((nA >> 2) * 4 + 1) * PRS + 4 + (nA & 3) * 4, oB = ((nB >> 2) * 4 + 1) * PRS + 4 + (nB & 3) * 4;
                        const int sb = second ? oB : oA;
                        const int mode = step_mode(t);
                        uint8_t *S = T + sb;
                        const int va = T[sb - 64 + (int)(to & 0xff)], vb = T[sb - 64 + (int)((to >> 8) & 0xff)], vc = T[sb - 64 + (int)(to >> 16)];
                        const int dir = (va + 2 * vb + vc + 2) >> 2;
                        const int tm = clamp255(va + vb - vc);
                        int p = mode == 1 ? tm : dir;
                        /* B_DC_PRED's five LDS reads and the sum only where one of the step's two sub-blocks asks for it (the modes are the
                         * wave's: a scalar test) */
                        if (sub_mode(nA) == 0 || sub_mode(nB) == 0) {
                            const u32 top4 = *(const u32 *)(S - PRS);
                            const int l0 = S[-1], l1 = S[PRS - 1], l2 = S[2 * PRS - 1], l3 = S[3 * PRS - 1];
                            const int dc = (4 + sum4(top4) + l0 + l1 + l2 + l3) >> 3;
                            p = mode == 0 ? dc : p;
                        }
                        S[r * PRS + c] = (uint8_t)clamp255(p + rv);
                        wave_sync();
                    }
                    lumaout = *(const u32 *)(T + (r16 + 1) * PRS + 4 + c16);
                } else {
                    const u32 top4 = *(const u32 *)(T + 4 + c16);
                    const int lf = T[(r16 + 1) * PRS + 3], cor = T[3];
                    int dcv = 0;
                    if (ymode == 0) { /* DC over the edges that exist (predict.c:34-76) */
                        int dc = 0;
                        if (x > 0) {
#pragma unroll
                            for (int k2 = 0; k2 < 16; k2++) dc += T[(k2 + 1) * PRS + 3];
                        }
                        if (y > 0) dc += sum4(*(const u32 *)(T + 4)) + sum4(*(const u32 *)(T + 8)) + sum4(*(const u32 *)(T + 12)) + sum4(*(const u32 *)(T + 16));
                        if (x == 0 && y == 0) dc = 0x80;
                        else if (x == 0 || y == 0) dc = (dc + 8) >> 4;
                        else dc = (dc + 16) >> 5;
                        dcv = dc & 0xff;
                    }
                    const s16x4 rs = *(const s16x4 *)(R + 16 * (4 * (r16 >> 2) + (c16 >> 2)) + 4 * (r16 & 3));
                    u32 o = 0;
                    const unsigned long long is_dc = __builtin_amdgcn_ballot_w64(ymode == 0), is_v = __builtin_amdgcn_ballot_w64(ymode == 2),
                                             is_h = __builtin_amdgcn_ballot_w64(ymode == 3);
                    const int lc = lf - cor;
#pragma unroll
                    for (int k2 = 0; k2 < 4; k2++) {
                        const int tpx = (int)((top4 >> (8 * k2)) & 0xff);
                        int p = clamp255(tpx + lc);          /* TM_PRED */
                        p = lane_select_smask(is_h, p, lf);             /* raw dst[-1]   (predict.c:346-353) */
                        p = lane_select_smask(is_v, p, tpx);            /* raw row above (predict.c:338-344) */
                        p = lane_select_smask(is_dc, p, dcv);
                        o |= (u32)clamp255(p + rs[k2]) << (8 * k2);
                    }
                    wave_sync();
                    *(u32 *)(T + (r16 + 1) * PRS + 4 + c16) = o;
                    lumaout = o;
                }
                /* ---- chroma: one pixel of U and one of V per lane ---- */
                {
                    const int r = lane >> 3, c = lane & 7;
#pragma unroll
                    for (int pl = 0; pl < 2; pl++) {
                        const uint8_t *Cp = pl ? C1 : C0;
                        const int lf = Cp[(r + 1) * PCS + 3], tpx = Cp[4 + c], cor = Cp[3];
                        int p;
                        if (uvmode == 0) {
                            int dc = 0;
                            if (x > 0) {
#pragma unroll
                                for (int k2 = 0; k2 < 8; k2++) dc += Cp[(k2 + 1) * PCS + 3];
                            }
                            if (y > 0) dc += sum4(*(const u32 *)(Cp + 4)) + sum4(*(const u32 *)(Cp + 8));
                            if (x == 0 && y == 0) dc = 0x80;
                            else if (x == 0 || y == 0) dc = (dc + 4) >> 3;
                            else dc = (dc + 8) >> 4;
                            p = dc & 0xff;
                        } else {
                            p = lane_select_smask(__builtin_amdgcn_ballot_w64(uvmode == 1), lf, clamp255(lf + tpx - cor));
                            p = lane_select_smask(__builtin_amdgcn_ballot_w64(uvmode == 2), p, tpx);
                        }
                        const int ri = 256 + 64 * pl + 16 * (2 * (r >> 2) + (c >> 2)) + 4 * (r & 3) + (c & 3);
                        outc[pl] = clamp255(p + R[ri]);
                    }
                    wave_sync();
                    C0[(r + 1) * PCS + 4 + c] = (uint8_t)outc[0];
                    C1[(r + 1) * PCS + 4 + c] = (uint8_t)outc[1];
                    /* ---- the reconstructed macroblock into the filter tiles (the prediction tiles keep the unfiltered copy) ---- */
                    *(u32 *)(TL + (r16 + 6) * FLS + 8 + c16) = lumaout;
                    (AR + AR_TC0)[(r + 4) * FLS + 4 + c] = (uint8_t)outc[0];
                    (AR + AR_TC1)[(r + 4) * FLS + 4 + c] = (uint8_t)outc[1];
                }
                wave_sync();
                /* ---- the loop filter of this macroblock (webp.c:1686-1752): left edge + inner vertical edges, then top edge +
                 * inner horizontal edges; inner edges for B_PRED macroblocks in the simple filter, for the others in the normal one ---- */
                if (TYPE != 0) {
                    const bool bpred = ymode == 4;
                    const uint8_t *fp = FT + ((((mo[4] >> 16) & 3) * 2) + (bpred ? 1 : 0)) * 3;
                    sub = __builtin_amdgcn_readfirstlane((int)fp[0]); inter = __builtin_amdgcn_readfirstlane((int)fp[1]);
                    hevt = __builtin_amdgcn_readfirstlane((int)fp[2]);
                    /* FR_SPEC, both filter types: B_PRED, or some block has a non-zero dequantised coefficient (byte [19] of the record, left there
                     * by the residual stage; mo[4] is fetched for the segment id anyway) */
#if FR_SPEC
                    inner = bpred || ((mo[4] >> 24) & 1u) != 0u;
#else
                    inner = TYPE == 1 ? bpred : !bpred;
#endif
                    if (sub) {
                        filter_phase<1, TYPE == 1 ? 1 : 2>(f_vbase, f_active, f_lum, x > 0, inner, sub, inter, hevt);
                        wave_sync();
                        filter_phase<FLS, TYPE == 1 ? 1 : 2>(f_hbase, f_active, f_lum, y > 0, inner, sub, inter, hevt);
                        wave_sync();
                    }
                }
            }
            /* ---- out of the tiles: the lines this macroblock hands down, the block it emits ---- */
            const u32 lsv = FLDS32(ls_src);
            const u32 el = FLDS32(em_l);
            const u32 eu = (u32)FLDS16(em_u), ev = (u32)FLDS16(em_v);
            const u32 pcv = PLANES ? FLDS32(pc_src) : 0u;
            /* colour (utils/colorspace.c:291-329) in the packed form of the fused JPEG kernels: the three chroma terms of the lane's two
             * chroma samples at once (one fma + one add each, exact on 8-bit samples: tests/tools/check_color_fma.c), per pixel PAIR three
             * 16-bit adds, three saturating packs, three byte permutes; fp64 only where 215 uu + 381 vv is a non-zero multiple of 1000 */
#if FR_SPEC /* planes only: the colour step is a kernel of its own */
            (void)eu; (void)ev; (void)rOut; (void)em_dst;
#else
            const u32x4 px = ff_packed420_row(ff_packed420_terms(eu, ev), el);
#endif
            /* ---- the lines of macroblock x - 1 are complete, and the fetch of x + 1 has arrived, once all but this wave's NEWEST memory operations
             * have completed (they complete in issue order): the end of the previous iteration issued the fetch of x + 1 FIRST, then the lines of
             * x - 1, then -- last -- the block of x - 1 (and its planes).  Those last stores are a kilobyte on its way to HBM; nothing waits for them
             * here (as s_waitcnt vmcnt(0), with the fetch issued at the top of the iteration behind them, this wait was for their completion:
             * 41 % of the waves' cycles were waiting, profiles/r4_vp8_frames256_pmc.txt) ---- */
#if FR_SPEC /* no block: behind the fetch and the lines come luma, U | V (two instructions), so all but the newest THREE */
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
#else
            if (PLANES) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); /* block, luma, U | V (two instructions) */
            else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");        /* block */
#endif
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0 && real_row) __hip_atomic_store(&PROG[w], my_base + (u32)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            /* ---- the tiles move on: their right ends become the left border, the fetched macroblock goes in ---- */
            if (x < a.mbcols) {
                const u32x2 kl = keeps_l ? *(__attribute__((address_space(3))) u32x2 *)(unsigned long long)(keep_l + 16) : u32x2{0, 0};
                const u32 kc = FLDS32(keep_c + (keep_c == dump ? 0 : 8));
                wave_sync();
                if (keeps_l) *(__attribute__((address_space(3))) u32x2 *)(unsigned long long)keep_l = kl;
                FLDS32(keep_c) = kc;
                if (x + 1 < a.mbcols) consume(x + 1);
                else wave_sync();
            }
            /* ---- the fetch of the macroblock after next, IN FRONT of this one's stores (see the wait above) ---- */
            {   /* (past the row's end: its last macroblock again, for nobody -- a fetch on every way round the loop, see above) */
                const int x2 = x + 2 < a.mbcols ? x + 2 : a.mbcols - 1;
                fetch(x2, real_row ? res_row(x2) : 0, need_of(x2));
                }
            /* ---- stores: the lines (real macroblocks only), the BGRA block, the planes for who wants them ---- */
            {
                const int dst = lane_select_smask(real_mb ? (x > 0 ? ls_any : ls_at0) : 0ull, FR_OUT, ls_dst + x * ls_step); /* (no lines from the emission-only row and column: dropped) */
                __builtin_amdgcn_raw_buffer_store_b32(lsv, rL, dst, me_off, 0);
            }
            {
                const unsigned long long em_ok = em_rows & (x == 0 ? cols_first : (x < a.mbcols ? ~0ull : ~cols_first));
#if !FR_SPEC
                const int dst = lane_select_smask(em_ok, FR_OUT, em_dst + y * 16 * a.pitch + x * 64);
                __builtin_amdgcn_raw_buffer_store_b128(px, rOut, dst, 0, 0);
#endif
                if (PLANES) {
                    const int dsty = lane_select_smask(em_ok, FR_OUT, em_dsty + y * 16 * ys + x * 16);
                    __builtin_amdgcn_raw_buffer_store_b32(el, rY, dsty, 0, 0);
                    const unsigned long long pc_ok = pc_rows & (x == 0 ? pcol_first : (x < a.mbcols ? pc_all : pc_all & ~pcol_first));
                    const int dstc = lane_select_smask(pc_ok, FR_OUT, pc_dst + y * 8 * us + x * 8);
                    if (lane < 16) __builtin_amdgcn_raw_buffer_store_b32(pcv, rU, dstc, 0, 0);
                    else __builtin_amdgcn_raw_buffer_store_b32(pcv, rV, dstc, 0, 0);
                }
            }
        }
        /* ---- the row is complete once its last stores are ---- */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0 && real_row) __hip_atomic_store(&PROG[w], my_base + (u32)a.mbcols, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
