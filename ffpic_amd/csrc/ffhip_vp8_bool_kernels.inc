/* ffhip_vp8_bool_kernels.inc -- the two kernels of the device front end as text, included by ffhip_vp8_bool_gpu.hip once per WebpPixelRule
 * (ffhip_vp8_bool.h) with WEBP_K_HEADERS, WEBP_K_TOKENS (the kernels' names), WEBP_K_MB_TOKENS (the rule's ffb_mb_tokens) and WEBP_K_RULE (the rule, a literal) defined. */
/* kernel A: one lane = the first partition of one frame.  Under WEBP_RULE_LIBWEBP a
 * skipped macroblock shows its own (zero) residual; what else the rule changes here the host's header reader has put into D.mb */
__global__ __launch_bounds__(64) void WEBP_K_HEADERS(const WebpDesc *descs, int n, int pack, int32_t *verdict)
{
    const int lane = threadIdx.x, i = blockIdx.x * pack + lane;
    if (lane >= pack || i >= n) return;
    const WebpDesc &D = descs[i];
    ffb_dec d;
    d.p = D.bytes;
    d.pos = D.pos;
    d.len = D.p0_len;
    d.value = D.value;
    d.range = D.range;
    d.count = D.count;
    d.err = 0;
    const ffb_mbhdr_probs fp = D.mb;
    const int cols = D.mbcols, rows = D.mbrows;
    int32_t last_coded = -1;
    for (int y = 0; y < rows; y++) {
        uint32_t left4 = 0;
        for (int x = 0; x < cols; x++) {
            const int32_t mb = y * cols + x;
            uint8_t *rec = D.modes + (size_t)mb * 20;
            const uint32_t above4 = y > 0 ? ffb_rec_bottom4(rec - (size_t)cols * 20) : 0;
            uint8_t r[20];
            const int skip = ffb_mb_header(&d, &fp, above4, &left4, r);
            uint32_t *rw = (uint32_t *)rec; /* records are 4-byte aligned */
#pragma unroll
            for (int k = 0; k < 5; k++) rw[k] = (uint32_t)r[4 * k] | (uint32_t)r[4 * k + 1] << 8 | (uint32_t)r[4 * k + 2] << 16 | (uint32_t)r[4 * k + 3] << 24;
            D.skip[mb] = (uint8_t)skip;
            if (!skip) last_coded = mb;
            D.resmap[mb] = WEBP_K_RULE != WEBP_RULE_LIBWEBP && skip && last_coded >= 0 ? last_coded : mb;
        }
    }
    verdict[2 * i] = d.err;
}

/* kernel B: one lane = the token partitions of one frame (WEBP_RULE_LIBWEBP: cat6 extra bits are not wrapped) */
__global__ __launch_bounds__(64) void WEBP_K_TOKENS(const WebpDesc *descs, int n, int pack, int32_t *verdict)
{
    extern __shared__ uint32_t s_probs[]; /* [pack][264] */
    for (int s = 0; s < pack; s++) {
        const int f = blockIdx.x * pack + s;
        if (f < n) {
            const uint32_t *src = (const uint32_t *)descs[f].probs;
            for (int k = threadIdx.x; k < 264; k += 64) s_probs[s * 264 + k] = src[k];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x, i = blockIdx.x * pack + lane;
    if (lane >= pack || i >= n) return;
    const WebpDesc &D = descs[i];
    const uint8_t *probs = (const uint8_t *)(s_probs + lane * 264);
    const int cols = D.mbcols, rows = D.mbrows, nparts = D.nparts;
    ffb_dec d;
    int err = 0;
    for (int k = nparts - 1; k >= 0; k--) { /* bool_dec_init of every partition (webp.c:1905-1911); partition 0 stays in registers */
        ffb_init(&d, D.bytes + D.part_off[k], D.part_len[k]); /* loads nothing: a partition no row reads may be empty */
        if (nparts > 1) {
            D.parked[4 * k] = d.value; D.parked[4 * k + 1] = d.range; D.parked[4 * k + 2] = (uint32_t)d.count; D.parked[4 * k + 3] = d.pos;
        }
    }
    int cur = 0;
    for (int y = 0; y < rows; y++) {
        const int want = y & (nparts - 1);
        if (want != cur) { /* park the row's decoder, take the next row's */
            D.parked[4 * cur] = d.value; D.parked[4 * cur + 1] = d.range; D.parked[4 * cur + 2] = (uint32_t)d.count; D.parked[4 * cur + 3] = d.pos;
            err |= d.err;
            d.p = D.bytes + D.part_off[want];
            d.len = D.part_len[want];
            d.value = D.parked[4 * want]; d.range = D.parked[4 * want + 1]; d.count = (int32_t)D.parked[4 * want + 2]; d.pos = D.parked[4 * want + 3];
            d.err = 0;
            cur = want;
        }
        uint32_t left9 = 0;
        for (int x = 0; x < cols; x++) {
            const size_t mb = (size_t)y * cols + x;
            const int has_y2 = D.modes[mb * 20] != 4;
            uint8_t *info = D.mbinfo + mb * 32;
            uint32_t top9 = D.top[x];
            if (!D.skip[mb]) {
                WEBP_K_MB_TOKENS(&d, probs, has_y2, &top9, &left9, D.levels + mb * 400, info);
            } else {
                top9 = ffb_skip_ctx(top9, has_y2);
                left9 = ffb_skip_ctx(left9, has_y2);
            }
            D.top[x] = (uint16_t)top9;
            info[25] = (uint8_t)has_y2;
            info[26] = D.modes[mb * 20 + 18];
        }
    }
    verdict[2 * i + 1] = err | d.err;
}
