/* The orientation stage's per-lane bodies (ffpic_amd/csrc/ffhip_orient_body.h) run on the CPU, lane by lane in the kernel's order, over
 * exact-size allocations: built with -fsanitize=address,undefined, a read outside the stored picture or a write outside the upright one
 * ends the program.  The result is held against the coordinate map applied pixel by pixel, and the destination's row padding against its
 * fill.  Exit 0 and no output when all is well. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffhip_orient_body.h"

static int run(int w, int h, int x0, int y0, int extra, int o)
{
    const int pw = x0 + w + (x0 ? 2 : 0), ph = y0 + h + (y0 ? 1 : 0); /* the picture around the rectangle */
    const long long sp = 4LL * pw, uw = FFHIP_ORIENT_TRANSPOSE(o) ? h : w, uh = FFHIP_ORIENT_TRANSPOSE(o) ? w : h, dp = 4 * uw + extra;
    const size_t src_bytes = (size_t)(sp * ph), dst_bytes = (size_t)(dp * (uh - 1) + 4 * uw);
    uint8_t *src = (uint8_t *)malloc(src_bytes), *dst = (uint8_t *)malloc(dst_bytes);
    for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)(i * 2654435761u >> 13);
    memset(dst, 0xA5, dst_bytes);
    OrientItemDesc d;
    memset(&d, 0, sizeof d);
    d.src = src + y0 * sp + 4 * x0; d.dst = dst; d.src_pitch = sp; d.dst_pitch = dp;
    d.ws = w; d.hs = h; d.orientation = o;
    d.tiles_x = (uint32_t)((w + FFHIP_ORIENT_TILE - 1) / FFHIP_ORIENT_TILE);
    const uint32_t tiles_y = (uint32_t)((h + FFHIP_ORIENT_TILE - 1) / FFHIP_ORIENT_TILE);
    std::vector<uint32_t> tile(FFHIP_ORIENT_TILE * FFHIP_ORIENT_LDS_PITCH);
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        for (uint32_t tx = 0; tx < d.tiles_x; tx++) {
            const OrientTile t = orient_tile(d, tx, ty);
            if (!FFHIP_ORIENT_TRANSPOSE(o)) {
                for (int row = 0; row < FFHIP_ORIENT_TILE; row++)
                    for (int lane = 0; lane < 64; lane++) {
                        int c, r;
                        const uint32_t v = orient_straight_source(d, t, lane, row, &c, &r) ? orient_load(d, t, c, r) : 0u;
                        if (lane < t.uw && row < t.uh) orient_store(d, t, lane, row, v);
                    }
                continue;
            }
            for (int row = 0; row < FFHIP_ORIENT_TILE; row++)
                for (int lane = 0; lane < 64; lane++)
                    tile[(size_t)(row * FFHIP_ORIENT_LDS_PITCH + lane)] = lane < t.tw && row < t.th ? orient_load(d, t, lane, row) : 0u;
            for (int row = 0; row < FFHIP_ORIENT_TILE; row++)
                for (int lane = 0; lane < 64; lane++) {
                    int at;
                    const uint32_t v = orient_transposed_source(d, t, lane, row, &at) ? tile.at((size_t)at) : 0u;
                    if (lane < t.uw && row < t.uh) orient_store(d, t, lane, row, v);
                }
        }
    int bad = 0;
    for (int y = 0; y < uh && !bad; y++) {
        for (int x = 0; x < uw && !bad; x++) {
            int sx, sy, bx, by;
            ffhip_orient_stored_of(o, w, h, x, y, &sx, &sy);
            ffhip_orient_upright_of(o, w, h, sx, sy, &bx, &by);
            bad = bx != x || by != y || sx < 0 || sx >= w || sy < 0 || sy >= h || memcmp(dst + y * dp + 4 * x, d.src + sy * sp + 4 * sx, 4) != 0;
        }
        for (long long b = 4 * uw; b < dp && y + 1 < uh && !bad; b++) bad = dst[y * dp + b] != 0xA5;
    }
    if (bad) fprintf(stderr, "orientation %d of %d x %d at (%d, %d): wrong\n", o, w, h, x0, y0);
    free(src);
    free(dst);
    return bad;
}

int main(void)
{
    static const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 200}, {63, 65}, {64, 64}, {65, 63}, {130, 67}, {257, 129}};
    int bad = 0;
    for (const auto &s : sizes)
        for (int o = 1; o <= 8; o++) bad += run(s[0], s[1], 0, 0, 0, o) + run(s[0], s[1], 5, 3, 12, o);
    return bad ? 1 : 0;
}
