/* ffhip_vp8_frame_lanes.inc -- what each lane of a k_vp8_frames / k_vp8_frames_items wave does, by its number, for a frame of
 * a.mbcols macroblocks (ys, us, off_* in scope).  Included as text by both kernels (ffhip_vp8_frame.hip). */
    /* ---- what a lane does, by its number ---- */
    /* prediction borders, one byte per lane out of the row above's unfiltered lines: luma columns -1..19 (lanes 0..20), U and V
     * columns -1..7 (21..29, 32..40); lane 48: the sample left of the row's first pixel at x = 0 (the last pixel of the row above) */
    const int pb_off = lane <= 20 ? off_ul + lane - 1 : (lane >= 21 && lane <= 29 ? off_uu + lane - 22 : (lane >= 32 && lane <= 40 ? off_uv + lane - 33 : FR_OUT));
    const int pb_step = lane <= 20 ? 16 : 8;
    const int dst1 = lane <= 20 ? 3 + lane : (lane <= 29 && lane >= 21 ? BT_C0 + 3 + (lane - 21) : (lane >= 32 && lane <= 40 ? BT_C1 + 3 + (lane - 32) :
                     (lane >= 48 ? (lane - 47) * PRS + 3 : BT_DUMP)));
    const int dst2 = lane < 16 ? (lane < 8 ? BT_C0 : BT_C1) + ((lane & 7) + 1) * PCS + 3 : BT_DUMP;
    const int carry_src = lane >= 48 ? (lane - 47) * PRS + 4 + 15 : (lane < 16 ? (lane < 8 ? BT_C0 : BT_C1) + ((lane & 7) + 1) * PCS + 4 + 7 : BT_DUMP);
    /* the filter tiles' top rows out of the row above's filtered lines, a dword per lane: luma rows -6..-1 (lanes 0..23: row
     * lane >> 2, dword lane & 3), chroma rows -4..-1 of U (32..39) and V (40..47) */
    const int lt_off = lane < 24 ? (lane >> 2) * ys + 4 * (lane & 3) : (lane >= 32 && lane < 48 ? (lane < 40 ? off_fu : off_fv) + ((lane >> 1) & 3) * us + 4 * (lane & 1) : FR_OUT);
    const int lt_step = lane < 24 ? 16 : 8;
    const unsigned lt_dst = lane < 24 ? tl + (unsigned)((lane >> 2) * FLS + 8 + 4 * (lane & 3))
                                      : (lane >= 32 && lane < 48 ? (lane < 40 ? tc0 : tc1) + (unsigned)(((lane >> 1) & 3) * FLS + 4 + 4 * (lane & 1)) : dump);
    /* the tiles' right ends become the next macroblock's left border: luma 8 columns of 22 rows (lanes 0..21: two dwords),
     * chroma 4 columns of 12 rows (lanes 32..43 U, 44..55 V) */
    const unsigned keep_l = lane < 22 ? tl + (unsigned)(lane * FLS) : dump;
    const unsigned keep_c = lane >= 32 && lane < 56 ? (lane < 44 ? tc0 : tc1) + (unsigned)(((lane - 32) % 12) * FLS) : dump;
    const bool keeps_l = lane < 22;
    /* the lines this row hands down, a dword per lane, out of the tiles AFTER the filter (lanes 0..29: luma rows 10..15, columns
     * -4..15 as five dwords; 32..55: chroma rows 4..7 of U then V, columns -4..7 as three dwords) and out of the prediction
     * tiles, which the filter never touches (56..63: the unfiltered bottom row, 4 + 2 + 2 dwords).  Columns 13..15 (5..7) are
     * rewritten by the next macroblock, whose left-edge filter changes them; the dword left of the first macroblock does not exist */
    int ls_dst, ls_step;
    unsigned ls_src;
    bool ls_first;
    if (lane < 30) {
        const int r = lane / 5, d = lane % 5;
        ls_src = tl + (unsigned)((16 + r) * FLS + 4 + 4 * d); ls_dst = r * ys - 4 + 4 * d; ls_step = 16; ls_first = d > 0;
    } else if (lane >= 32 && lane < 56) {
        const int p = (lane - 32) / 12, j = (lane - 32) % 12, r = j / 3, d = j % 3;
        ls_src = (p ? tc1 : tc0) + (unsigned)((8 + r) * FLS + 4 * d); ls_dst = (p ? off_fv : off_fu) + r * us - 4 + 4 * d; ls_step = 8; ls_first = d > 0;
    } else if (lane >= 56) {
        const int k = lane - 56;
        if (k < 4) { ls_src = bt + (unsigned)(16 * PRS + 4 + 4 * k); ls_dst = off_ul + 4 * k; ls_step = 16; }
        else if (k < 6) { ls_src = bt + (unsigned)(BT_C0 + 8 * PCS + 4 + 4 * (k - 4)); ls_dst = off_uu + 4 * (k - 4); ls_step = 8; }
        else { ls_src = bt + (unsigned)(BT_C1 + 8 * PCS + 4 + 4 * (k - 6)); ls_dst = off_uv + 4 * (k - 6); ls_step = 8; }
        ls_first = true;
    } else { ls_src = dump; ls_dst = FR_OUT; ls_step = 0; ls_first = false; }
    const unsigned long long ls_any = __builtin_amdgcn_ballot_w64(ls_dst != FR_OUT), ls_at0 = __builtin_amdgcn_ballot_w64(ls_first);
    /* the pixels a macroblock emits: rows -6..9, columns -8..7 from its origin; lane = (row, group of four pixels) */
    const int er = lane >> 2, eg = lane & 3;
    const unsigned em_l = tl + (unsigned)(er * FLS + 4 * eg), em_u = tc0 + (unsigned)((1 + (er >> 1)) * FLS + 2 * eg), em_v = tc1 + (unsigned)((1 + (er >> 1)) * FLS + 2 * eg);
    const int em_dst = (er - 6) * a.pitch + (4 * eg - 8) * 4, em_dsty = (er - 6) * ys + 4 * eg - 8;
    const unsigned long long rows_first = __builtin_amdgcn_ballot_w64(er >= 6), cols_first = __builtin_amdgcn_ballot_w64(eg >= 2);
    /* ... and, for callers that want the planes too, the chroma of that block: rows -3..4, columns -4..3 (lanes 0..15 U, 16..31 V) */
    const int pr = (lane >> 1) & 7, pd = lane & 1;
    const unsigned pc_src = lane < 32 ? (lane < 16 ? tc0 : tc1) + (unsigned)((1 + pr) * FLS + 4 * pd) : dump;
    const int pc_dst = lane < 32 ? (pr - 3) * us + 4 * pd - 4 : FR_OUT;
    const unsigned long long prow_first = __builtin_amdgcn_ballot_w64(lane < 32 && pr >= 3), pcol_first = __builtin_amdgcn_ballot_w64(lane < 32 && pd >= 1),
                             pc_all = __builtin_amdgcn_ballot_w64(lane < 32);
    /* the filter's lines: lanes 0..15 a luma line, 16..23 U, 24..31 V */
    const bool f_lum = lane < 16, f_active = lane < 16 || (lane < 32 && TYPE == 2);
    uint8_t *const f_mine = f_lum ? TL : (AR + ((lane >> 3) & 1 ? AR_TC1 : AR_TC0));
    const int f_li = f_lum ? lane : (lane & 7);
    uint8_t *const f_vbase = f_lum ? f_mine + (f_li + 6) * FLS + 4 : f_mine + (f_li + 4) * FLS;
    uint8_t *const f_hbase = f_lum ? f_mine + 2 * FLS + f_li + 8 : f_mine + f_li + 4;
