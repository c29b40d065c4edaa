/* ffhip_jpeg420_body.inc -- the body of the fused 4:2:0 kernels (ffhip_jpeg.hip), included inside k_jpeg420_fused and, with
 * FFHIP_JPEG_ITEMS defined, inside k_jpeg420_fused_items.  Shared as text rather than as a __forceinline__ function: inlining
 * a function reorders the kernel's IR and with it the register allocation, and the uniform kernels' ISA is to stay what it was
 * (DESIGN.md 4.2 "Mixed batches").  Not a header: no include guard, and nothing but ffhip_jpeg.hip includes it. */
    __shared__ __attribute__((aligned(16))) char lds_all[WAVES_PER_WG * LDS_WAVE_BYTES];
    const u32 lane = threadIdx.x & 63;
    /* wave-uniform values are forced into SGPRs: hipcc cannot prove that anything
     * derived from threadIdx is uniform and would run all the index math per lane */
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    /* 1-D grid over (image, slot group); a slot is QPW consecutive quads of the image's row-major
     * quad sequence.  Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one), so
     * the linear id is remapped to give every XCD one contiguous chunk of the sequence: the
     * pieces of an output row then come from one XCD back to back instead of from eight at
     * different times (+6 % on the memory-only pattern, tests/tools/membench_jpeg.hip).
     * Speed only: any placement computes the same bytes. */
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
    const int qidx0 = (int)((u32)wgi * WAVES_PER_WG + wave) * QPW;
    if (qidx0 >= p.quads_per_image) return; /* wave-uniform; no barriers anywhere in this kernel */

    WaveCtx c;
    wave_ctx_init(c, lds_all + wave * LDS_WAVE_BYTES, lane);
    LaneRoles r;
    lane_roles_init(r, c, lane, (u32)p.pitch);

    int mrow[QPW], qcol[QPW];
    QuadLoads ld[QPW];
#pragma unroll
    for (int i = 0; i < QPW; i++) {
        int qi = qidx0 + i;
        qi = qi < p.quads_per_image ? qi : p.quads_per_image - 1; /* duplicate load, never stored */
        int mr = (int)__umulhi((u32)qi, p.qpr_magic), qc = qi - mr * p.quads_per_row; /* scalar */
        if (qc < 0) { mr--; qc += p.quads_per_row; }
        if (qc >= p.quads_per_row) { mr++; qc -= p.quads_per_row; } /* quads_per_row == 1: magic saturates */
        mrow[i] = mr;
        qcol[i] = qc;
        ld[i] = quad_load<NT & 1>(p, r, lane, img, mr, qc * 4);
    }
    const uint16_t *qt = p.quant + (long long)img * p.quant_stride;
    const u32x4 q_y = *(const u32x4 *)(qt + p.qt_y * 64 + r.row * 8);
    const u32x4 q_c = *(const u32x4 *)(qt + (lane < 32 ? p.qt_u : p.qt_v) * 64 + r.row * 8);
#pragma unroll
    for (int i = 0; i < QPW; i++)
        if (qidx0 + i < p.quads_per_image) {
            if (PATTERN) quad_pattern<NT>(p, r, ld[i], img, mrow[i], qcol[i] * 4);
            else quad_recon<NT>(p, c, r, lane, ld[i], q_y, q_c, img, mrow[i], qcol[i] * 4);
        }
