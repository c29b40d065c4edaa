/* check_tensor_alpha_body.cpp -- the alpha forms of the tensor sink's body (ffpic_amd/csrc/ffhip_tensor_body.h) run lane by lane on the CPU,
 * as the kernel deals its units out: every destination offset 0..15 elements x width 1..40 x height 1..3, both layouts, both orders, the
 * three dtypes, the three modes with straight and with premultiplied sources.  The output is held against a plain loop that states the
 * rule by divisions (tests/alpha_spec.py states it by shifts), and 0xA5 everywhere else: row padding, plane padding and 64 guard bytes
 * either side.  Picture and output come from malloc at their exact size, so built with -fsanitize=address,undefined the run also shows
 * that nothing is read or written outside them:
 *     clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=alignment -Iinclude -Iffpic_amd/csrc \
 *             tests/tools/check_tensor_alpha_body.cpp -o check_tensor_alpha_body && ./check_tensor_alpha_body
 * Then the premultiplying resize: the row staging of the kernel (resize_staged<true>, ffhip_resize_body.h) and its tap loop over a row
 * buffer of the exact chunk size, the tables from the rule's own functions, against premultiply-by-division and the double sum in 64 bits.
 * A program of its own, never loaded into another process.  Needs clang: the body uses ext_vector_type. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ffhip_tensor_body.h"
#include "ffhip_resize_body.h"

/* ---- the rule, by divisions ---- */
static uint32_t w_div255(uint32_t t) { return (2u * t + 255u) / 510u; } /* floor(t / 255 + 1/2) */
static uint32_t w_step(int mode, bool pre, uint32_t c, uint32_t a, uint32_t g)
{
    if (mode == FFHIP_ALPHA_STRAIGHT) return !pre ? c : (a == 0 ? 0u : (255u * c / a > 255u ? 255u : 255u * c / a));
    if (mode == FFHIP_ALPHA_PREMULTIPLIED) return pre ? c : w_div255(c * a);
    if (!pre) return w_div255(c * a + g * (255u - a));
    const uint32_t v = c + w_div255(g * (255u - a));
    return v > 255u ? 255u : v;
}
static int policy_of(int mode, bool pre)
{
    if (mode == FFHIP_ALPHA_STRAIGHT) return pre ? TENSOR_ALPHA_UNPREMUL : TENSOR_ALPHA_KEEP;
    if (mode == FFHIP_ALPHA_PREMULTIPLIED) return pre ? TENSOR_ALPHA_KEEP : TENSOR_ALPHA_PREMUL;
    return pre ? TENSOR_ALPHA_OVER_P : TENSOR_ALPHA_OVER_S;
}

template <int DT, bool PLANAR, bool BGR, int NC, int AP> static void run_all(const TensorItemDesc &d, const TensorScale &s, const TensorAlpha &al)
{
    for (uint32_t wg = 0; wg < d.n_wgs; wg++)
        for (uint32_t tid = 0; tid < 256; tid++)
            for (int i = 0; i < FFHIP_TENSOR_UNITS_PER_LANE; i++) {
                uint32_t t = wg * FFHIP_TENSOR_WG_UNITS + tid + i * 256;
                if (t >= d.total) break;
                tensor_unit<DT, PLANAR, BGR, NC, AP>(d, s, t, al);
            }
}
typedef void (*Fn)(const TensorItemDesc &, const TensorScale &, const TensorAlpha &);
template <int DT, bool PLANAR, bool BGR> static Fn pick3(int policy)
{
    switch (policy) {
    case TENSOR_ALPHA_KEEP: return run_all<DT, PLANAR, BGR, 4, TENSOR_ALPHA_KEEP>;
    case TENSOR_ALPHA_PREMUL: return run_all<DT, PLANAR, BGR, 4, TENSOR_ALPHA_PREMUL>;
    case TENSOR_ALPHA_UNPREMUL: return run_all<DT, PLANAR, BGR, 4, TENSOR_ALPHA_UNPREMUL>;
    case TENSOR_ALPHA_OVER_S: return run_all<DT, PLANAR, BGR, 3, TENSOR_ALPHA_OVER_S>;
    default: return run_all<DT, PLANAR, BGR, 3, TENSOR_ALPHA_OVER_P>;
    }
}
template <int DT> static Fn pick(bool planar, bool bgr, int policy)
{
    return planar ? (bgr ? pick3<DT, true, true>(policy) : pick3<DT, true, false>(policy)) : (bgr ? pick3<DT, false, true>(policy) : pick3<DT, false, false>(policy));
}

static const uint8_t ALPHAS[] = {0, 1, 127, 128, 254, 255};

/* a picture with the alphas that matter and random ones over random colour; premultiplied: every colour byte at most its alpha */
static void fill_picture(uint8_t *src, long pixels, bool pre)
{
    for (long i = 0; i < pixels; i++) {
        const int r = rand();
        const uint32_t a = (r & 1) ? ALPHAS[(r >> 1) % 6] : (uint32_t)((r >> 4) & 255);
        for (int c = 0; c < 3; c++) src[4 * i + c] = (uint8_t)(pre ? (uint32_t)rand() % (a + 1u) : (uint32_t)rand() & 255u);
        src[4 * i + 3] = (uint8_t)a;
    }
}

static long check_sink(long *checked)
{
    long bad = 0;
    for (int dt = 0; dt < 3; dt++)
        for (int planar = 0; planar < 2; planar++)
            for (int bgr = 0; bgr < 2; bgr++)
                for (int mode = FFHIP_ALPHA_STRAIGHT; mode <= FFHIP_ALPHA_OVER; mode++)
                    for (int pre = 0; pre < 2; pre++) {
                        const int es = dt == 0 ? 1 : dt == 1 ? 2 : 4, nc = mode == FFHIP_ALPHA_OVER ? 3 : 4;
                        TensorScale s;
                        for (int c = 0; c < 3; c++) { s.scale[c] = dt ? 1.0f / (255.0f * (0.2f + 0.01f * c)) : 1.0f; s.bias[c] = dt ? -0.4f - 0.03f * c : 0.0f; }
                        TensorAlpha al;
                        const uint8_t bg[3] = {37, 200, 254}; /* B, G, R */
                        al.background = bg[0] | bg[1] << 8 | bg[2] << 16;
                        al.alpha_scale = dt ? 1.0f / 255.0f : 1.0f;
                        al.alpha_bias = dt ? 0.125f : 0.0f;
                        const int policy = policy_of(mode, pre != 0);
                        Fn fn = dt == 0 ? pick<0>(planar, bgr, policy) : dt == 1 ? pick<1>(planar, bgr, policy) : pick<2>(planar, bgr, policy);
                        for (int w = 1; w <= 40; w++) for (int h = 1; h <= 3; h++) for (int off = 0; off < 16; off++) {
                            const int x0 = off % 3, y0 = off & 1, extra = (w + off) % 3;
                            const int pw = x0 + w, ph = y0 + h; /* the picture is exactly as large as the rectangle needs */
                            const long pitch = 4L * pw;
                            uint8_t *src = (uint8_t *)malloc(pitch * ph);
                            fill_picture(src, (long)pw * ph, pre != 0);
                            const long run_len = planar ? w : nc * w, rs = run_len + extra, ps = rs * (h - 1) + w + extra;
                            const long n_el = off + (planar ? (nc - 1) * ps + rs * (h - 1) + w : rs * (h - 1) + run_len);
                            const long G = 64; /* guard bytes; malloc returns 16-byte alignment, `off` elements move the output off it */
                            uint8_t *raw = (uint8_t *)malloc(n_el * es + 2 * G), *dst = raw + G;
                            memset(raw, 0xA5, n_el * es + 2 * G);
                            std::vector<uint8_t> exp_raw(n_el * es + 2 * G, 0xA5);
                            uint8_t *exp = exp_raw.data() + G;
                            TensorItemDesc d;
                            memset(&d, 0, sizeof d);
                            d.src = src + y0 * pitch + 4 * x0; d.dst = dst + off * es; d.pitch = pitch; d.row_stride = rs; d.plane_stride = planar ? ps : 0;
                            d.width = w; d.height = h;
                            const long runs = (planar ? nc : 1) * h, units = (run_len * es + 15) / 16 + 1;
                            d.units = units; d.total = runs * units; d.n_wgs = (runs * units + FFHIP_TENSOR_WG_UNITS - 1) / FFHIP_TENSOR_WG_UNITS;
                            fn(d, s, al);
                            for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) for (int c = 0; c < nc; c++) {
                                const uint8_t *px = src + (y0 + y) * pitch + 4 * (x0 + x);
                                const int pos = bgr ? c : 2 - c;
                                const uint32_t byte = c == 3 ? px[3] : w_step(mode, pre != 0, px[pos], px[3], bg[pos]);
                                const long e = off + (planar ? c * ps + y * rs + x : y * rs + nc * x + c);
                                const float prod = (float)byte * (c == 3 ? al.alpha_scale : s.scale[c]);
                                const float f = prod + (c == 3 ? al.alpha_bias : s.bias[c]);
                                if (dt == 0) exp[e] = (uint8_t)byte;
                                else if (dt == 1) { _Float16 hf = (_Float16)f; memcpy(&exp[e * 2], &hf, 2); }
                                else memcpy(&exp[e * 4], &f, 4);
                            }
                            (*checked)++;
                            if (memcmp(exp_raw.data(), raw, n_el * es + 2 * G)) {
                                bad++;
                                if (bad < 10) printf("MISMATCH dt=%d planar=%d bgr=%d mode=%d pre=%d w=%d h=%d off=%d\n", dt, planar, bgr, mode, pre, w, h, off);
                            }
                            free(raw); free(src);
                        }
                    }
    return bad;
}

/* the un-premultiply for every (p, a) with p <= a, the other steps for every pair of bytes */
static long check_steps()
{
    long bad = 0;
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t c = 0; c < 256; c++) {
            bad += alpha_premultiply(c, a) != w_div255(c * a);
            if (c <= a) bad += alpha_unpremultiply(c, a) != (a ? 255u * c / a : 0u);
            bad += alpha_unpremultiply(c, a) > 255u;
            for (uint32_t g : {0u, 1u, 37u, 128u, 200u, 254u, 255u}) {
                bad += alpha_over_straight(c, a, g) != w_div255(c * a + g * (255u - a));
                if (c <= a) bad += alpha_over_premultiplied(c, a, g) != c + w_div255(g * (255u - a));
                bad += alpha_over_premultiplied(c, a, g) > 255u;
            }
        }
    return bad;
}

/* ---- the premultiplying resize: staging and tap loop as the kernel has them, one output row and column tile at a time ---- */
#define LDS_PIXELS 4096 /* FFHIP_RESIZE_LDS_PIXELS of ffhip_resize.hip */
static long check_resize(long *checked)
{
    const int shapes[][4] = {{5, 3, 2, 2}, {37, 53, 8, 8}, {3, 3, 7, 5}, {300, 2, 7, 1}, {4100, 1, 3, 1}}; /* w, h, out w, out h */
    long bad = 0;
    for (const int *sh : shapes)
        for (int filter = FFHIP_RESIZE_BILINEAR; filter <= FFHIP_RESIZE_ANTIALIAS; filter++) {
            const uint32_t w = sh[0], h = sh[1], ow = sh[2], oh = sh[3];
            uint32_t *src = (uint32_t *)malloc(4ul * w * h);
            fill_picture((uint8_t *)src, (long)w * h, false);
            /* the tables as k_resize_tables writes them: first | count << 16, the weights tap-major */
            std::vector<uint32_t> fcx(ow), fcy(oh);
            const uint32_t tx = resize_axis_max_taps(w, ow, filter), ty = resize_axis_max_taps(h, oh, filter);
            std::vector<uint16_t> qx((size_t)tx * ow, 0), qy((size_t)ty * oh, 0);
            for (uint32_t o = 0; o < ow; o++) {
                const ResizeRun t = resize_axis_run(w, ow, filter, o);
                fcx[o] = t.first | t.count << 16;
                resize_axis_weights(t, ow, [&](uint32_t j, uint32_t q) { qx[j * ow + o] = (uint16_t)q; });
            }
            for (uint32_t o = 0; o < oh; o++) {
                const ResizeRun t = resize_axis_run(h, oh, filter, o);
                fcy[o] = t.first | t.count << 16;
                resize_axis_weights(t, oh, [&](uint32_t j, uint32_t q) { qy[j * oh + o] = (uint16_t)q; });
            }
            for (uint32_t oy = 0; oy < oh; oy++) {
                const uint32_t seg0 = fcx[0] & 0xffffu, seg1 = (fcx[ow - 1] & 0xffffu) + (fcx[ow - 1] >> 16); /* one tile: out widths are below 256 */
                const uint32_t fy = fcy[oy] & 0xffffu, cy = fcy[oy] >> 16;
                std::vector<uint32_t> acc(4 * ow, 0);
                for (uint32_t t = 0; t < cy; t++) {
                    const uint32_t wy = qy[t * oh + oy];
                    const uint32_t *line = src + (size_t)(fy + t) * w;
                    std::vector<uint32_t> hsum(4 * ow, 0);
                    for (uint32_t c0 = seg0; c0 < seg1; c0 += LDS_PIXELS) {
                        const uint32_t len = seg1 - c0 < LDS_PIXELS ? seg1 - c0 : LDS_PIXELS;
                        uint32_t *row = (uint32_t *)malloc(4ul * len); /* exactly the chunk */
                        for (uint32_t i = 0; i < len; i++) row[i] = resize_staged<true>(line[c0 + i]);
                        for (uint32_t ox = 0; ox < ow; ox++) {
                            const uint32_t fx = fcx[ox] & 0xffffu, cx = fcx[ox] >> 16;
                            const uint32_t j_lo = c0 > fx ? c0 - fx : 0u;
                            const uint32_t j_hi = c0 + len > fx ? (c0 + len - fx < cx ? c0 + len - fx : cx) : 0u;
                            for (uint32_t j = j_lo; j < j_hi; j++) {
                                const uint32_t q = qx[j * ow + ox];
                                const uint32_t v = row[fx + j - c0];
                                hsum[4 * ox] += q * (v & 0xffu);
                                hsum[4 * ox + 1] += q * ((v >> 8) & 0xffu);
                                hsum[4 * ox + 2] += q * ((v >> 16) & 0xffu);
                                hsum[4 * ox + 3] += q * (v >> 24);
                            }
                        }
                        free(row);
                    }
                    for (uint32_t k = 0; k < 4 * ow; k++) acc[k] += wy * hsum[k];
                }
                /* the witness: premultiply by division, the double sum in 64 bits over the runs */
                for (uint32_t ox = 0; ox < ow; ox++) {
                    const uint32_t fx = fcx[ox] & 0xffffu, cx = fcx[ox] >> 16;
                    uint64_t sum[4] = {0, 0, 0, 0};
                    uint64_t wsum = 0;
                    for (uint32_t t = 0; t < cy; t++)
                        for (uint32_t j = 0; j < cx; j++) {
                            const uint8_t *px = (const uint8_t *)(src + (size_t)(fy + t) * w + fx + j);
                            const uint64_t q = (uint64_t)qy[t * oh + oy] * qx[j * ow + ox];
                            for (int c = 0; c < 3; c++) sum[c] += q * w_div255((uint32_t)px[c] * px[3]);
                            sum[3] += q * px[3];
                            wsum += q;
                        }
                    uint32_t out[4];
                    for (int c = 0; c < 4; c++) {
                        out[c] = (uint32_t)((sum[c] + (1u << 23)) >> 24);
                        const uint32_t got = (acc[4 * ox + c] + (1u << 23)) >> 24;
                        bad += got != out[c];
                    }
                    bad += wsum != (1u << 24);
                    bad += out[0] > out[3] || out[1] > out[3] || out[2] > out[3]; /* the output is a premultiplied pixel */
                    (*checked)++;
                }
            }
            free(src);
        }
    return bad;
}

int main()
{
    srand(1);
    long sink_cases = 0, pixels = 0;
    const long bad_steps = check_steps();
    const long bad_sink = check_sink(&sink_cases);
    const long bad_resize = check_resize(&pixels);
    printf("steps: %ld bad\nsink: checked %ld cases, %ld bad\nresize: checked %ld pixels, %ld bad\n", bad_steps, sink_cases, bad_sink, pixels, bad_resize);
    return (bad_steps || bad_sink || bad_resize) != 0;
}
