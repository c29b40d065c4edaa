/* ffhip_orient_body.h -- the coordinate map of the eight EXIF orientations, the record and the per-lane bodies of the orientation stage
 * (ffhip_orient.hip).  Plain C / C++ without builtins, __host__ too: ffhip_exif.c maps rectangles with the same function the kernel maps
 * its tiles with, and a CPU program can run the bodies lane by lane over host buffers and hold their addressing against exact-size
 * allocations.
 *
 * Every orientation is a transpose (5..8) or none, then a mirror of the stored x axis (2, 3, 7, 8) and of the stored y axis (3, 4, 6, 7):
 * with (a, b) = (x, y) of the upright pixel, swapped where there is a transpose, the stored pixel is (flip_x ? Ws-1-a : a,
 * flip_y ? Hs-1-b : b).  That is the table of include/ffpic_hip.h line by line.
 *
 * The work: the STORED rectangle is cut into tiles of 64 x 64 pixels, one workgroup of four waves each, wave w the rows w, w + 4, ...
 * of its tile.  A tile of the stored rectangle is a tile of the upright one (at the mapped corner), so:
 *   1..4   lane i of row j loads stored pixel (flip_x ? tw-1-i : i, flip_y ? th-1-j : j) of the tile and stores upright pixel (i, j): a wave
 *          reads 64 consecutive dwords (backwards where x is mirrored) and stores 64 consecutive dwords.  No LDS.
 *   5..8   the waves load the tile's rows (64 consecutive dwords) into tile[row * 65 + lane]; behind a barrier lane i of upright row j
 *          reads tile[r * 65 + c], r = flip_y ? th-1-i : i, c = flip_x ? tw-1-j : j, and stores upright pixel (i, j): 64 consecutive dwords
 *          of a destination row again.  The mirrors are index arithmetic on the tile.
 * LDS banks (ds_write_b32 / ds_read_b32: bank = dword address mod 32, conflicts only among the 32 lanes of a half wave): the row write has
 * dword address row * 65 + lane, 32 consecutive addresses per half: 32 different banks.  The column read has (+-i + const) * 65 + c
 * = +-i * 65 + const': mod 32 that is +-i + const'' (65 = 2 * 32 + 1), over 32 consecutive i again 32 different banks.  At a pitch of 64
 * the column read would put the 32 lanes on ONE bank (32-way). */
#ifndef FFHIP_ORIENT_BODY_H
#define FFHIP_ORIENT_BODY_H

#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#ifdef __HIP_DEVICE_COMPILE__
#define ORIENT_GLOBAL __attribute__((address_space(1)))
#else
#define ORIENT_GLOBAL
#endif

#define FFHIP_ORIENT_TILE 64
#define FFHIP_ORIENT_LDS_PITCH 65 /* dwords: see the bank arithmetic above */
#define FFHIP_ORIENT_WG_THREADS 256
#define FFHIP_ORIENT_ROWS_PER_WAVE (FFHIP_ORIENT_TILE / (FFHIP_ORIENT_WG_THREADS / 64))

#define FFHIP_ORIENT_TRANSPOSE(o) ((o) >= 5)
#define FFHIP_ORIENT_FLIP_X(o) ((o) == 2 || (o) == 3 || (o) == 7 || (o) == 8)
#define FFHIP_ORIENT_FLIP_Y(o) ((o) == 3 || (o) == 4 || (o) == 6 || (o) == 7)

/* upright pixel (ux, uy) of orientation o (1..8) of a stored ws x hs picture -> the stored pixel it shows */
__host__ __device__ static inline void ffhip_orient_stored_of(int o, int ws, int hs, int ux, int uy, int *sx, int *sy)
{
    const int a = FFHIP_ORIENT_TRANSPOSE(o) ? uy : ux, b = FFHIP_ORIENT_TRANSPOSE(o) ? ux : uy;
    *sx = FFHIP_ORIENT_FLIP_X(o) ? ws - 1 - a : a;
    *sy = FFHIP_ORIENT_FLIP_Y(o) ? hs - 1 - b : b;
}
/* and back: the upright pixel that shows stored pixel (sx, sy) */
__host__ __device__ static inline void ffhip_orient_upright_of(int o, int ws, int hs, int sx, int sy, int *ux, int *uy)
{
    const int a = FFHIP_ORIENT_FLIP_X(o) ? ws - 1 - sx : sx, b = FFHIP_ORIENT_FLIP_Y(o) ? hs - 1 - sy : sy;
    *ux = FFHIP_ORIENT_TRANSPOSE(o) ? b : a;
    *uy = FFHIP_ORIENT_TRANSPOSE(o) ? a : b;
}

#ifdef __cplusplus
struct OrientItemDesc { /* 64 bytes, 16-byte aligned: scalar loads */
    const uint8_t *src;            /* pixel (x0, y0) of the stored picture */
    uint8_t *dst;                  /* pixel (0, 0) of the upright picture */
    long long src_pitch, dst_pitch;
    int ws, hs;                    /* the stored rectangle */
    int orientation;
    uint32_t tiles_x;              /* tiles side by side: (ws + 63) / 64 */
    uint32_t first_wg, n_wgs;      /* its workgroups: one tile each, row by row */
    uint32_t pad_[2];
};

struct OrientTile {
    int sx0, sy0, tw, th; /* the tile in the stored rectangle: its corner, what of its 64 x 64 lies inside */
    int ux0, uy0;         /* the corner (lowest x, lowest y) of the same pixels in the upright picture */
    int uw, uh;           /* their extent there: (tw, th), swapped under a transpose */
};

__host__ __device__ inline OrientTile orient_tile(const OrientItemDesc &d, uint32_t tx, uint32_t ty)
{
    OrientTile t;
    t.sx0 = (int)tx * FFHIP_ORIENT_TILE;
    t.sy0 = (int)ty * FFHIP_ORIENT_TILE;
    t.tw = d.ws - t.sx0 < FFHIP_ORIENT_TILE ? d.ws - t.sx0 : FFHIP_ORIENT_TILE;
    t.th = d.hs - t.sy0 < FFHIP_ORIENT_TILE ? d.hs - t.sy0 : FFHIP_ORIENT_TILE;
    /* the stored pixel of the tile that the upright tile's corner shows: the far end of every mirrored axis */
    const int cx = FFHIP_ORIENT_FLIP_X(d.orientation) ? t.sx0 + t.tw - 1 : t.sx0;
    const int cy = FFHIP_ORIENT_FLIP_Y(d.orientation) ? t.sy0 + t.th - 1 : t.sy0;
    ffhip_orient_upright_of(d.orientation, d.ws, d.hs, cx, cy, &t.ux0, &t.uy0);
    t.uw = FFHIP_ORIENT_TRANSPOSE(d.orientation) ? t.th : t.tw;
    t.uh = FFHIP_ORIENT_TRANSPOSE(d.orientation) ? t.tw : t.th;
    return t;
}

/* the tile's stored pixel (c, r), c < tw, r < th */
__host__ __device__ inline uint32_t orient_load(const OrientItemDesc &d, const OrientTile &t, int c, int r)
{
    return *(const ORIENT_GLOBAL uint32_t *)((const ORIENT_GLOBAL uint8_t *)d.src + (long long)(t.sy0 + r) * d.src_pitch + 4LL * (t.sx0 + c));
}
/* the tile's upright pixel (i, j), i < uw, j < uh */
__host__ __device__ inline void orient_store(const OrientItemDesc &d, const OrientTile &t, int i, int j, uint32_t v)
{
    *(ORIENT_GLOBAL uint32_t *)((ORIENT_GLOBAL uint8_t *)d.dst + (long long)(t.uy0 + j) * d.dst_pitch + 4LL * (t.ux0 + i)) = v;
}

/* 1..4, lane i of upright row j: is there a pixel, and which stored pixel of the tile it shows */
__host__ __device__ inline bool orient_straight_source(const OrientItemDesc &d, const OrientTile &t, int i, int j, int *c, int *r)
{
    *c = FFHIP_ORIENT_FLIP_X(d.orientation) ? t.tw - 1 - i : i;
    *r = FFHIP_ORIENT_FLIP_Y(d.orientation) ? t.th - 1 - j : j;
    return i < t.tw && j < t.th;
}
/* 5..8, lane i of upright row j: is there a pixel, and the dword of the LDS tile that holds it */
__host__ __device__ inline bool orient_transposed_source(const OrientItemDesc &d, const OrientTile &t, int i, int j, int *at)
{
    const int r = FFHIP_ORIENT_FLIP_Y(d.orientation) ? t.th - 1 - i : i;
    const int c = FFHIP_ORIENT_FLIP_X(d.orientation) ? t.tw - 1 - j : j;
    *at = r * FFHIP_ORIENT_LDS_PITCH + c;
    return i < t.th && j < t.tw;
}
#endif /* __cplusplus */

#endif
