/* check_tensor_body.cpp -- the tensor sink's body (ffpic_amd/csrc/ffhip_tensor_body.h) run lane by lane on the CPU, as the kernel deals its
 * units out, over every width x height x x0 x output offset x row stride of the alignment test in all twelve formats: the bytes of a plain
 * loop, and 0xA5 everywhere else (64 guard bytes either side of the output included).  The picture is exactly as large as the rectangle
 * needs and both buffers come from malloc at their exact size, so built with -fsanitize=address,undefined the run also shows that nothing
 * is READ outside the picture:
 *     clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=alignment -Iinclude -Iffpic_amd/csrc \
 *             tests/tools/check_tensor_body.cpp -o check_tensor_body && ./check_tensor_body
 * (tests/test_tensor_capi.py builds it without a sanitizer.)  Needs clang: the body uses ext_vector_type. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ffhip_tensor_body.h"

template <int DT, bool PLANAR, bool BGR> static void run_all(const TensorItemDesc &d, const TensorScale &s)
{
    for (uint32_t wg = 0; wg < d.n_wgs; wg++)
        for (uint32_t tid = 0; tid < 256; tid++)
            for (int i = 0; i < FFHIP_TENSOR_UNITS_PER_LANE; i++) {
                uint32_t t = wg * FFHIP_TENSOR_WG_UNITS + tid + i * 256;
                if (t >= d.total) break;
                tensor_unit<DT, PLANAR, BGR>(d, s, t);
            }
}
typedef void (*Fn)(const TensorItemDesc &, const TensorScale &);
template <int DT> static Fn pick(bool planar, bool bgr)
{
    return planar ? (bgr ? run_all<DT, true, true> : run_all<DT, true, false>) : (bgr ? run_all<DT, false, true> : run_all<DT, false, false>);
}

int main()
{
    const int widths[] = {1, 2, 3, 4, 5, 7, 13, 16, 17, 63, 64, 65, 67, 255, 257};
    const int heights[] = {1, 2, 3, 17};
    const int x0s[] = {0, 1, 2, 3, 5};
    long checked = 0, bad = 0;
    srand(1);
    for (int dt = 0; dt < 3; dt++)
        for (int planar = 0; planar < 2; planar++)
            for (int bgr = 0; bgr < 2; bgr++) {
                const int es = dt == 0 ? 1 : dt == 1 ? 2 : 4;
                TensorScale s;
                for (int c = 0; c < 3; c++) { s.scale[c] = dt ? 1.0f / (255.0f * (0.2f + 0.01f * c)) : 1.0f; s.bias[c] = dt ? -0.4f - 0.03f * c : 0.0f; }
                Fn fn = dt == 0 ? pick<0>(planar, bgr) : dt == 1 ? pick<1>(planar, bgr) : pick<2>(planar, bgr);
                for (int w : widths) for (int h : heights) for (int x0 : x0s) for (int off = 0; off < 4; off++) for (int extra : {0, 1, 3}) {
                    const int y0 = x0 & 1;
                    const int pw = x0 + w, ph = y0 + h; /* the picture is exactly as large as the rectangle needs */
                    const long pitch = 4L * pw;
                    uint8_t *src = (uint8_t *)malloc(pitch * ph);
                    for (long i = 0; i < pitch * ph; i++) src[i] = rand();
                    const long run_len = planar ? w : 3 * w, rs = run_len + extra, ps = rs * (h - 1) + w + extra;
                    const long n_el = off + (planar ? 2 * ps + rs * (h - 1) + w : rs * (h - 1) + run_len);
                    const long G = 64; /* guard bytes; malloc returns 16-byte alignment, `off` elements move the output off it */
                    uint8_t *raw = (uint8_t *)malloc(n_el * es + 2 * G), *dst = raw + G;
                    memset(raw, 0xA5, n_el * es + 2 * G);
                    std::vector<uint8_t> exp_raw(n_el * es + 2 * G, 0xA5);
                    uint8_t *exp = exp_raw.data() + G;
                    TensorItemDesc d;
                    memset(&d, 0, sizeof d);
                    d.src = src + y0 * pitch + 4 * x0; d.dst = dst + off * es; d.pitch = pitch; d.row_stride = rs; d.plane_stride = planar ? ps : 0;
                    d.width = w; d.height = h;
                    const long runs = (planar ? 3 : 1) * h, units = (run_len * es + 15) / 16 + 1;
                    d.units = units; d.total = runs * units; d.n_wgs = (runs * units + FFHIP_TENSOR_WG_UNITS - 1) / FFHIP_TENSOR_WG_UNITS;
                    fn(d, s);
                    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) for (int c = 0; c < 3; c++) {
                        const uint8_t byte = src[(y0 + y) * pitch + 4 * (x0 + x) + (bgr ? c : 2 - c)];
                        const long e = off + (planar ? c * ps + y * rs + x : y * rs + 3 * x + c);
                        const float f = (float)byte * s.scale[c] + s.bias[c];
                        if (dt == 0) exp[e] = byte;
                        else if (dt == 1) { _Float16 hf = (_Float16)f; memcpy(&exp[e * 2], &hf, 2); }
                        else memcpy(&exp[e * 4], &f, 4);
                    }
                    checked++;
                    if (memcmp(exp_raw.data(), raw, n_el * es + 2 * G)) { bad++; if (bad < 10) printf("MISMATCH dt=%d planar=%d bgr=%d w=%d h=%d x0=%d off=%d extra=%d\n", dt, planar, bgr, w, h, x0, off, extra); }
                    free(raw); free(src);
                }
            }
    printf("checked %ld cases, %ld bad\n", checked, bad);
    return bad != 0;
}
