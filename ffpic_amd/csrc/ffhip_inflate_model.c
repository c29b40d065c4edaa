/*
 * ffhip_inflate_model.c -- the host model of k_inflate (ffhip_inflate_gpu.hip): ffhip_inflate_body.h with the wave's 64
 * lanes emulated.  Plain C11, host only.  The serial part runs once (on the device every lane runs it, to the same values); a step of
 * the writer part runs as ALL 64 loads, then ALL 64 stores, as the lanes of a wave execute one load and one store instruction: a step
 * whose lanes depended on each other's stores gives wrong bytes here as it would there.
 */
#include "ffpic_hip.h"
#include "ffhip_inflate_body.h"
#include "ffhip_png_internal.h"

/* how a step is emulated.  0: the kernel's.  The others exist for the test that shows the emulation sees a same-step hazard
 * (tests/test_inflate_model.py): 1 reads a match's source where a byte-by-byte copy would, dst[to - distance + k], still all loads before
 * all stores -- wrong bytes for distance < 64; 2 reads there and runs lane after lane, load and store together -- the byte-by-byte copy
 * itself, right again; 3 is the kernel's addresses run lane after lane, right as well: those addresses have no hazard to see */
enum { MODEL_STEPS = 0, MODEL_NAIVE_STEPS = 1, MODEL_NAIVE_LANEWISE = 2, MODEL_LANEWISE = 3 };

static int model_load(const ffhip_inf_step *s, const ffhip_inf_store *m, const uint8_t *src, const uint8_t *dst, int lane, uint8_t *v, int naive)
{
    if (naive && s->kind == FFHIP_INF_MATCH) {
        if (lane >= (int)s->n) return 0;
        *v = dst[s->to - s->dist + (uint64_t)lane];
        return 1;
    }
    return ffhip_inf_step_load(s, m, src, dst, lane, v);
}

int ffhip_inflate_model_mode(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial, int mode)
{
    if (!src || (!dst && cap) || !out_len || mode < MODEL_STEPS || mode > MODEL_LANEWISE) return FFHIP_EINVAL;
    *out_len = 0;
    ffhip_inf_state st;
    ffhip_inf_store store;
    int rc = ffhip_inf_begin(&st, src, len, cap, partial);
    const int naive = mode == MODEL_NAIVE_STEPS || mode == MODEL_NAIVE_LANEWISE, lanewise = mode == MODEL_NAIVE_LANEWISE || mode == MODEL_LANEWISE;
    while (!rc && !st.done) {
        const int n = ffhip_inf_batch(&st, &store);
        if (n < 0) { rc = n; break; }
        for (int k = 0; k < n; k++) {
            const ffhip_inf_step *s = &store.step[k];
            uint8_t v[FFHIP_INF_LANES];
            int has[FFHIP_INF_LANES];
            if (lanewise) {
                for (int lane = 0; lane < FFHIP_INF_LANES; lane++)
                    if (model_load(s, &store, src, dst, lane, &v[lane], naive)) ffhip_inf_step_store(s, dst, lane, v[lane]);
                continue;
            }
            for (int lane = 0; lane < FFHIP_INF_LANES; lane++) has[lane] = model_load(s, &store, src, dst, lane, &v[lane], naive);
            for (int lane = 0; lane < FFHIP_INF_LANES; lane++)
                if (has[lane]) ffhip_inf_step_store(s, dst, lane, v[lane]);
        }
    }
    *out_len = (size_t)st.out_len;
    if (rc || st.full) return rc; /* full: the caller wanted no more than this; the check value is not looked at */
    uint32_t a = 1, b = 0;
    for (uint64_t at = 0; at < st.out_len; at += FFHIP_INF_ADLER_BLOCK) {
        const uint32_t m = st.out_len - at < FFHIP_INF_ADLER_BLOCK ? (uint32_t)(st.out_len - at) : FFHIP_INF_ADLER_BLOCK;
        uint32_t s1 = 0, s2 = 0;
        for (int lane = 0; lane < FFHIP_INF_LANES; lane++) {
            uint32_t l1, l2;
            ffhip_inf_adler_lane(dst + at, m, lane, &l1, &l2);
            s1 += l1;
            s2 += l2;
        }
        ffhip_inf_adler_fold(&a, &b, m, s1, s2);
    }
    return st.want == (b << 16 | a) ? FFHIP_OK : FFHIP_EINVAL;
}

int ffhip_inflate_model(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial)
{
    return ffhip_inflate_model_mode(src, len, dst, cap, out_len, partial, MODEL_STEPS);
}
