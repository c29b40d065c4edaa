/* check_parts.cpp -- the part loop of the calls that answer per item (ffpic_amd/csrc/ffhip_parts.h: ffhip_parts_run) on the CPU, over a few
 * hundred seeded lists of weights -- zeros, weights above the budget and n = 0 among them -- with and without a cap on a part's items:
 * the parts are contiguous and cover [0, n) in order, no part has more than max_items items, no part of two or more items exceeds the
 * budget, every cut is greedy, each of the four fatal codes ends the call at its part with that code, and of the other codes the first
 * that is not FFHIP_OK is the call's while the later parts still run.  This is the only run of the JPEG and deflate calls' part boundary:
 * they have no cap, so a second part takes a gigabyte of input.
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iffpic_amd/csrc tests/tools/check_parts.cpp \
 *         -o check_parts && ./check_parts
 * (tests/test_png_encode_capi.py builds and runs exactly that.) */
#include "ffhip_parts.h"

#include <stdint.h>
#include <stdio.h>
#include <vector>

static uint64_t g_seed;
static uint32_t rnd(void)
{
    g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(g_seed >> 33);
}

struct Part { int first, cnt; };
static int g_bad;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (g_bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                      \
    } while (0)

/* the call over `w` whose part k returns script[k] (FFHIP_OK beyond the script); the parts it ran */
static int run(const std::vector<size_t> &w, size_t budget, int max_items, const std::vector<int> &script, std::vector<Part> *parts)
{
    parts->clear();
    return ffhip_parts_run((int)w.size(), budget, max_items, [&](int i) { return w[(size_t)i]; }, [&](int first, int cnt) {
        parts->push_back({first, cnt});
        return parts->size() <= script.size() ? script[parts->size() - 1] : FFHIP_OK;
    });
}

static void check_cut(const std::vector<size_t> &w, size_t budget, int max_items, const std::vector<Part> &parts)
{
    const int n = (int)w.size();
    int at = 0;
    for (const Part &p : parts) {
        CHECK(p.first == at && p.cnt >= 1 && p.cnt <= max_items && p.first + p.cnt <= n);
        size_t sum = 0;
        for (int i = p.first; i < p.first + p.cnt && i < n; i++) sum += w[(size_t)i];
        CHECK(p.cnt < 2 || sum <= budget);
        at = p.first + p.cnt;
        CHECK(at == n || p.cnt == max_items || sum + w[(size_t)at] > budget); /* greedy: the next item would not have fitted */
    }
    CHECK(at == n);
}

int main(void)
{
    static const int fatal[4] = {FFHIP_EINVAL, FFHIP_ENOMEM, FFHIP_EIO, FFHIP_ENODEV};
    static const int verdicts[3] = {FFHIP_EPNG_NOSPACE, FFHIP_EJPEG_RANGE, 7};
    int lists = 0, n_parts = 0;
    std::vector<Part> parts, again;
    for (int seed = 0; seed < 400; seed++) {
        g_seed = 0x9E3779B97F4A7C15ULL * (uint64_t)(seed + 1);
        const int n = seed % 25 == 0 ? 0 : 1 + (int)(rnd() % (seed % 7 == 0 ? 300 : 40));
        const size_t budget = 1 + rnd() % 1000;
        const int max_items = seed % 3 == 0 ? FFHIP_PARTS_NO_CAP : 1 + (int)(rnd() % 9);
        std::vector<size_t> w((size_t)n);
        for (size_t &v : w) {
            const uint32_t kind = rnd() % 10;
            v = kind == 0 ? 0 : kind == 1 ? budget + 1 + rnd() % 1000 : kind == 2 ? budget : rnd() % (budget / 2 + 1);
        }
        CHECK(run(w, budget, max_items, {}, &parts) == FFHIP_OK);
        check_cut(w, budget, max_items, parts);
        CHECK((n == 0) == parts.empty());
        lists++;
        n_parts += (int)parts.size();
        if (parts.empty()) continue;
        const size_t k = rnd() % parts.size(), k2 = k + rnd() % (parts.size() - k);
        for (int code : fatal) { /* ends the call at part k, whatever came before */
            std::vector<int> script(k + 1, FFHIP_OK);
            if (k > 0) script[rnd() % k] = FFHIP_EPNG_NOSPACE;
            script[k] = code;
            CHECK(run(w, budget, max_items, script, &again) == code);
            CHECK(again.size() == k + 1);
        }
        for (int code : verdicts) { /* the first is kept, a later one is not, and every part runs */
            std::vector<int> script(k2 + 1, FFHIP_OK);
            script[k2] = FFHIP_EVP8L_NOSPACE;
            script[k] = code;
            CHECK(run(w, budget, max_items, script, &again) == code);
            CHECK(again.size() == parts.size());
            for (size_t p = 0; p < again.size() && p < parts.size(); p++) CHECK(again[p].first == parts[p].first && again[p].cnt == parts[p].cnt);
        }
    }
    if (g_bad) {
        fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    printf("ok: %d lists, %d parts\n", lists, n_parts);
    return 0;
}
