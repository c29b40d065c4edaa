/* ffhip_vp8_frame_items.inc -- the body of k_vp8_frames_items and of k_vp8_frames_items_libwebp (ffhip_vp8_frame.hip), from the LDS layout to the
 * walk over the workgroup's schedule: ONE text, included by both kernels with FR_SPEC 0 / 1 and PLANES, MAP (and TYPE) in scope, so that arena,
 * tap table and schedule cannot drift apart.  It includes the lane roles and the row text in its turn. */
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32 *const TT = (u32 *)(smem + SH_TT);
    u32 *const PROG = (u32 *)(smem + SH_PROG);
    u32 *const ABORT = (u32 *)(smem + SH_ABORT);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), NW = (int)(blockDim.x >> 6);
    uint8_t *const AR = smem + SH_BYTES + w * AR_BYTES;
    uint8_t *const FT = smem + SH_BYTES + NW * AR_BYTES + 32 * w; /* the wave's frame's filter parameters */
    uint8_t *const BT = AR + AR_BT, *const T = BT, *const C0 = BT + BT_C0, *const C1 = BT + BT_C1;
    short *const R = (short *)(AR + AR_R);
    uint8_t *const TL = AR + AR_TL;
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    const unsigned bt = (unsigned)(unsigned long long)(lds_u8 *)BT, tl = (unsigned)(unsigned long long)(lds_u8 *)TL,
                   tc0 = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_TC0), tc1 = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_TC1),
                   dump = (unsigned)(unsigned long long)(lds_u8 *)(AR + AR_DUMP) + 4u * (unsigned)lane;

    if (w == 0) {
        if (lane < 16) {
            auto off = [](int k) { return k < 4 ? (3 - k) * PRS - 1 : (k == 4 ? -PRS - 1 : -PRS + (k - 5)); };
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const unsigned t = kVp8Taps[m][lane];
                TT[(m + 2) * 16 + lane] = (u32)(off((int)(t & 15)) + 64) | ((u32)(off((int)((t >> 4) & 15)) + 64) << 8) | ((u32)(off((int)(t >> 8)) + 64) << 16);
            }
            const int r = lane >> 2, c = lane & 3;
            TT[16 + lane] = (u32)(r * PRS - 1 + 64) | ((u32)(-PRS + c + 64) << 8) | ((u32)(-PRS - 1 + 64) << 16);
            TT[lane] = 64u | (64u << 8) | (64u << 16);
            PROG[lane] = 0u;
        }
        if (lane == 0) *ABORT = ia.ctrl[1];
    }
    if (lane < 12) T[(4 + 4 * (lane >> 2)) * PRS + 20 + (lane & 3)] = 127;
    __syncthreads();
    if (__hip_atomic_load(ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;

    const __amdgpu_buffer_rsrc_t rL = ffhip_rsrc(ia.lines + (long long)blockIdx.x * (long long)(ia.nslot + 1) * (long long)ia.slot_bytes,
                                                 (unsigned)ia.nslot * ia.slot_bytes);
    fr_cslot *const S = (fr_cslot *)ia.sched + ((fr_cu32 *)ia.wg_first)[blockIdx.x];
    int e = 0;
    for (int g = w;; g += NW) {
        while (S[e].frame >= 0 && g >= S[e + 1].row0) e++;
        const int fi = S[e].frame;
        if (fi < 0) break;
        fr_cdesc *const fd = (fr_cdesc *)ia.frames + fi;
        Vp8FrameArgs a = {};
        a.modes = fd->modes; a.residual = fd->residual; a.resmap = fd->resmap; a.bgra = fd->bgra;
        a.lines = ia.lines; a.ctrl = ia.ctrl; a.async_err = ia.async_err;
        a.res_stride = fd->res_stride; a.pitch = fd->pitch; a.mbcols = fd->mbcols; a.mbrows = fd->mbrows; a.n_images = 1;
        a.nslot = ia.nslot; a.slot_bytes = ia.slot_bytes;
        const long long img = 0;
        const int y = g - S[e].row0;
        const int ys = 16 * a.mbcols, us = 8 * a.mbcols, n_mb = a.mbcols * a.mbrows;
#if FR_SPEC /* the frame's planes stand behind each other where the BGRA instances have their picture */
        a.bgra = nullptr; a.y = fd->bgra; a.u = a.y + 256LL * n_mb; a.v = a.u + 64LL * n_mb;
#endif
        const int off_fu = 6 * ys, off_fv = 6 * ys + 4 * us, off_ul = 6 * ys + 8 * us, off_uu = off_ul + ys, off_uv = off_uu + us;
        if (TYPE != 0 && lane < 24) FT[lane] = fd->filters[lane];
#include "ffhip_vp8_frame_lanes.inc"
        const bool real_row = y < a.mbrows;
        const int wp = (w + NW - 1) % NW;
        const u32 my_base = S[e].base0 + (u32)y * (u32)(a.mbcols + 2), up_base = y > 0 ? my_base - (u32)(a.mbcols + 2) : 0u;
#include "ffhip_vp8_frame_row.inc"
    }
