/* ffhip_vp8_residual_body.inc -- the residual stage of one macroblock `mb` of `a` by one 32-lane slot (t, slot, y2in, y2t in
 * scope).  Included as text by k_vp8_residual and k_vp8_residual_items (ffhip_vp8.hip). */
    const bool even = (t & 1) == 0;
    const int blk = even ? t >> 1 : 16 + (t >> 1); /* the block this lane computes; >= 25: none (odd lanes 19..31) */
    const bool works = blk < 25;
    const int kb = works ? blk : 0;
    /* the macroblock's 32 info bytes as two aligned dwords per lane (the one holding nz[blk], and bytes 24-27: nz of the
     * Y2 block, has_y2, segment) and the quantiser pair as one dword */
    const u32 *info = (const u32 *)(a.info + mb * 32);
    const u32 iw = info[kb >> 2], ic = info[6];
    const int nz = (int)((iw >> (8 * (kb & 3))) & 0xffu), nz24 = (int)(ic & 0xffu), has_y2 = ((ic >> 8) & 0xffu) != 0, seg = (int)((ic >> 16) & 3u);
    const int qsel = kb < 16 ? 0 : (kb < 24 ? 4 : 2);
    const u32 qpair = *(const u32 *)(a.quant + seg * 8 + qsel); /* (dc, ac) of this lane's block kind */
    const u32 qdc = qpair & 0xffffu, qac = qpair >> 16;
    const u32x4 *src = (const u32x4 *)(a.levels + mb * 400);
    const u32x4 c1 = __builtin_nontemporal_load(src + t);
    u32x4 c2 = {0u, 0u, 0u, 0u};
    if (t < 18) c2 = __builtin_nontemporal_load(src + 32 + t);
    if (PATTERN) { /* (info and quantiser words are loaded as ever: iw, ic, qpair feed the stored words so that nothing is dropped) */
        u32x4 *dstp = (u32x4 *)(a.out + mb * 384);
        const u32 k = iw ^ ic ^ qpair;
        __builtin_nontemporal_store(c1 + k, dstp + t);
        if (t < 16) __builtin_nontemporal_store(c2 + k, dstp + 32 + t);
        return;
    }
    /* block assembly inside the lane pair */
    const unsigned long long even_lanes = 0x5555555555555555ull;
    const u32x4 l0 = pair_pick<false>(c2, c1, even_lanes);  /* even: my first chunk; odd: my even neighbour's second load */
    const u32x4 l1 = pair_pick<true>(c1, c2, ~even_lanes);  /* even: my odd neighbour's first chunk; odd: my second load */
    const u32 lv[8] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    u32 pk[8]; /* pk[2r + h] = (c[4r + 2h], c[4r + 2h + 1]) */
#pragma unroll
    for (int i = 0; i < 8; i++) {
        /* low 16 bits of level*q == the int16 store of webp.c:1061 */
        const u32 f = i == 0 ? (qdc | (qac << 16)) : (qac | (qac << 16));
        using u16x2 = unsigned short __attribute__((ext_vector_type(2)));
        const u32 lvi = lv[i];
        pk[i] = __builtin_bit_cast(u32, (u16x2)(__builtin_bit_cast(u16x2, lvi) * __builtin_bit_cast(u16x2, f)));
    }
    /* Y2 -> luma DCs, ACROSS the sixteen luma lanes of the macroblock (webp.c:1067-1106).  Done by the Y2 lane
     * alone the inverse WHT is ~100 instructions that the whole wave pays for one or two working lanes (a third
     * of this VALU-bound kernel).  Instead the Y2 lane parks its 16 dequantised coefficients in LDS and the lane of luma
     * block 4r + i computes t[4r + i] of the column pass from column i, parks that, and computes w[4r + i] of the
     * row pass from row r: each is one of four +- combinations picked by r (then i), and w[blk] is exactly the DC
     * that block needs.  Writers and readers never sit on two sides of one branch (divergent sides have no defined
     * order): stores are predicated blocks followed by a wave-level fence; LDS serves a wave in program order. */
    if (blk == 24 && has_y2) {
        *(u32x4 *)&y2in[slot][0] = u32x4{pk[0], pk[1], pk[2], pk[3]};
        *(u32x4 *)&y2in[slot][8] = u32x4{pk[4], pk[5], pk[6], pk[7]};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool luma = even; /* blk < 16 */
    const int r4 = (blk >> 2) & 3, i4 = blk & 3;
    int tv = 0;
    if (luma && has_y2) {
        const int v0 = y2in[slot][i4], v1 = y2in[slot][4 + i4], v2 = y2in[slot][8 + i4], v3 = y2in[slot][12 + i4];
        const int a4 = v0 + v3, b4 = v1 + v2, e4 = v1 - v2, f4 = v0 - v3;
        const int p4 = (r4 & 1) ? f4 : a4, q4 = (r4 & 1) ? e4 : b4;
        tv = (r4 & 2) ? p4 - q4 : p4 + q4; /* rows: a+b, f+e, a-b, f-e */
        y2t[slot][blk] = tv;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (luma && has_y2) {
        const u32x4 row = *(const u32x4 *)&y2t[slot][4 * r4];
        const int t0 = (int)row[0], t1 = (int)row[1], t2 = (int)row[2], t3 = (int)row[3];
        const int a4 = t0 + t3, b4 = t1 + t2, e4 = t1 - t2, f4 = t0 - t3;
        const int p4 = (i4 & 1) ? f4 : a4, q4 = (i4 & 1) ? e4 : b4;
        const int full = (short)((((i4 & 2) ? p4 - q4 : p4 + q4) + 3) >> 3);
        const int fast = (short)((y2in[slot][0] + 3) >> 3); /* IWHT_fast, webp.c:1098-1106 */
        pk[0] = __builtin_amdgcn_perm(pk[0], (u32)(nz24 > 1 ? full : fast), 0x07060100u);
    }
    if (works && blk != 24 && (nz > 1 || (pk[0] & 0xffffu) != 0)) vp8_idct4x4(pk);
    /* back to chunks: chunk t = even ? my lower half : my even neighbour's upper half; chunk 32 + t (t < 16) = even ? my odd
     * neighbour's lower half : my upper half */
    const u32x4 o0 = {pk[0], pk[1], pk[2], pk[3]}, o1 = {pk[4], pk[5], pk[6], pk[7]};
    const u32x4 s1 = pair_pick<false>(o1, o0, even_lanes), s2 = pair_pick<true>(o0, o1, ~even_lanes);
    u32x4 *dst = (u32x4 *)(a.out + mb * 384);
    __builtin_nontemporal_store(s1, dst + t);
    if (t < 16) __builtin_nontemporal_store(s2, dst + 32 + t);
