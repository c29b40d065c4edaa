/* check_slots.cpp -- the arithmetic of the JPEG file pipeline's slots (ffpic_amd/csrc/ffhip_planes.h) on the CPU.
 * A slot's block is sized for a whole chunk, PlaneBlock(chunk * yb, chunk * cb, chunk), and every chunk of cnt <= chunk pictures lays its
 * own PlaneBlock(cnt * yb, cnt * cb, cnt) over the start of it, on the device and in the pinned twin, and uploads `bytes` of it in one copy.
 * Over every layout class's plane sizes, some MCU counts and every cnt <= chunk: the chunk's block fits the slot's; Y, U, V and the tables
 * lie in this order without overlap, the planes 2-byte and the tables 16-byte aligned, the last table ending at `bytes`; a grey batch has
 * no chroma planes; and every picture's share of each plane, written through the pointers `at` returns into an allocation of exactly the
 * slot's bytes (so that ASan sees a byte too far), lies inside its plane.  Then copy_out's split: for rows up to a few thousand and every
 * thread count asked for, the threads are 1 below 64 rows and 16 at most, and the ranges are contiguous, in order and cover [0, rows).
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iffpic_amd/csrc tests/tools/check_slots.cpp \
 *         -o check_slots && ./check_slots
 * (tests/test_jpeg_mixed_capi.py builds and runs exactly that.) */
#include "ffhip_planes.h"

#include <stdio.h>
#include <string.h>
#include <vector>

static int g_bad;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (g_bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                      \
    } while (0)

int main(void)
{
    /* (h * v, components) of the seven layout classes: 4:2:0, 4:4:4, 4:2:2, 4:4:0, h4v1, h1v4, grey */
    static const int classes[7][2] = {{4, 3}, {1, 3}, {2, 3}, {2, 3}, {4, 3}, {4, 3}, {1, 1}};
    static const size_t mcu_counts[] = {1, 2, 3, 57, 640};
    int blocks = 0, splits = 0;
    for (const auto &c : classes)
        for (size_t mcus : mcu_counts)
            for (int chunk = 1; chunk <= 5; chunk++) {
                const size_t yb = mcus * (size_t)c[0] * 64, cb = c[1] == 3 ? mcus * 64 : 0; /* int16 elements per picture, as chunk_loop has them */
                const PlaneBlock slot(chunk * yb, chunk * cb, (size_t)chunk);
                std::vector<uint8_t> mem(slot.bytes);
                for (int cnt = 1; cnt <= chunk; cnt++) {
                    const PlaneBlock blk(cnt * yb, cnt * cb, (size_t)cnt);
                    CHECK(blk.bytes <= slot.bytes);
                    if (blk.bytes > slot.bytes) continue;
                    const Planes p = blk.at(mem.data());
                    uint8_t *const y = (uint8_t *)p.y, *const q = (uint8_t *)p.q;
                    CHECK(y == mem.data() && q + (size_t)cnt * 512 == mem.data() + blk.bytes && blk.q_off % 16 == 0);
                    if (cb) {
                        uint8_t *const u = (uint8_t *)p.u, *const v = (uint8_t *)p.v;
                        CHECK(u == y + cnt * yb * 2 && v == u + cnt * cb * 2 && v + cnt * cb * 2 <= q && q < v + cnt * cb * 2 + 16);
                    } else {
                        CHECK(!p.u && !p.v && y + cnt * yb * 2 <= q && q < y + cnt * yb * 2 + 16);
                    }
                    for (int i = 0; i < cnt; i++) { /* picture i's share of each plane and its tables, as the decoders write them */
                        memset(p.y + (size_t)i * yb, i, yb * 2);
                        if (cb) memset(p.u + (size_t)i * cb, i, cb * 2);
                        if (cb) memset(p.v + (size_t)i * cb, i, cb * 2);
                        memset(p.q + (size_t)i * 256, i, 512);
                    }
                    blocks++;
                }
            }
    for (long long rows = 0; rows <= 4200; rows += rows < 70 ? 1 : 59)
        for (int asked = -1; asked <= 70; asked++) {
            const int nt = ffhip_copy_threads(rows, asked);
            CHECK(nt >= 1 && nt <= 16 && (rows >= 64 || nt == 1) && (asked < 1 || asked > 16 || rows < 64 || nt == asked));
            long long at = 0;
            for (int t = 0; t < nt; t++) {
                const FfhipRows r = ffhip_copy_rows(rows, t, nt);
                CHECK(r.lo == at && r.hi >= r.lo);
                at = r.hi;
            }
            CHECK(at == rows);
            splits++;
        }
    if (g_bad) {
        fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    printf("ok: %d blocks, %d splits\n", blocks, splits);
    return 0;
}
