/*
 * ffhip_heif.hip -- HEIF image-grid compositing.
 *
 * The reference parses the ImageGrid item (format/heif.c:273-298) and then decodes every tile
 * into the SAME buffer (heif.c:305: `decode_hvc1(..., &p->pixels, ...)`), so it never places
 * tiles; what ships here is the placement ISO/IEC 23008-12 6.6.2.3.1 prescribes, which is new
 * behaviour relative to the reference (documented in DESIGN.md, parity for it is unpinned):
 * tile j of the row-major `dimg` list lands at (j % cols * tile_w, j / cols * tile_h) and the
 * canvas is cropped to output_width x output_height.
 *
 * HBM-bound 2-D copy: 4 B read + 4 B written per canvas pixel.
 */
#include "ffhip_internal.h"

extern "C" int ffhip_heif_grid_parse(const uint8_t *item, size_t length, ffhip_heif_grid *out)
{
    if (!item || !out || length < 8) return FFHIP_EINVAL;
    out->version = item[0];
    out->flags = item[1];
    out->rows = item[2] + 1;
    out->cols = item[3] + 1;
    if ((item[1] & 1) == 0) { /* 16-bit big-endian fields, item length 8 (heif.c:284-289) */
        if (length != 8) return FFHIP_EINVAL;
        out->output_width = (uint32_t)item[4] << 8 | item[5];
        out->output_height = (uint32_t)item[6] << 8 | item[7];
    } else {                  /* 32-bit big-endian fields, item length 12 (heif.c:290-296) */
        if (length != 12) return FFHIP_EINVAL;
        out->output_width = (uint32_t)item[4] << 24 | (uint32_t)item[5] << 16 | (uint32_t)item[6] << 8 | item[7];
        out->output_height = (uint32_t)item[8] << 24 | (uint32_t)item[9] << 16 | (uint32_t)item[10] << 8 | item[11];
    }
    return out->output_width && out->output_height ? 0 : FFHIP_EINVAL;
}

extern "C" int ffhip_hevc_picture_layout(int pic_width, int pic_height, int ctb_log2, ffhip_hevc_layout *out)
{
    if (!out || pic_width <= 0 || pic_height <= 0 || ctb_log2 < 4 || ctb_log2 > 6) return FFHIP_EINVAL;
    const int ctb = 1 << ctb_log2;
    out->height = ((pic_height + 3) >> 2) << 2;      /* hevc.c:7224 */
    out->y_stride = ((pic_width + 3) >> 2) << 2;     /* hevc.c:7225 */
    out->uv_stride = out->y_stride >> 1;             /* hevc.c:7226 */
    out->size = (int64_t)out->height * out->y_stride; /* hevc.c:7228 */
    out->u_offset = out->size;                       /* hevc.c:7260 */
    out->v_offset = out->size * 3 / 2;
    out->pitch = ((out->y_stride * 32 + 32 - 1) >> 5) << 2; /* hevc.c:7259 */
    out->ctbrows = (out->height + ctb - 1) / ctb;    /* divceil, hevc.c:7260-7261 */
    out->ctbcols = (pic_width + ctb - 1) / ctb;
    return FFHIP_OK;
}

struct GridArgs {
    uint8_t *canvas;
    const uint8_t *tiles;
    long long canvas_pitch, tile_pitch, tile_stride;
    int out_w, out_h, tile_w, tile_h, cols;
};

/* VEC pixels per thread; VEC == 4 requires tile_w % 4 == 0 and 16-byte aligned pitches/bases */
template <int VEC>
__global__ __launch_bounds__(256) void k_grid_compose(GridArgs a)
{
    const int y = blockIdx.y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (x >= a.out_w) return;
    const int tr = y / a.tile_h, tc = x / a.tile_w; /* tile_h uniform per block row: scalar division */
    const uint8_t *src = a.tiles + ((long long)tr * a.cols + tc) * a.tile_stride + (long long)(y - tr * a.tile_h) * a.tile_pitch +
                         (long long)(x - tc * a.tile_w) * 4;
    uint8_t *dst = a.canvas + (long long)y * a.canvas_pitch + (long long)x * 4;
    if (VEC == 4) {
        const u32x4 v = __builtin_nontemporal_load((const u32x4 *)src);
        if (x + 4 <= a.out_w) {
            __builtin_nontemporal_store(v, (u32x4 *)dst);
        } else {
            for (int k = 0; k < a.out_w - x; k++) ((u32 *)dst)[k] = v[k];
        }
    } else {
        *(u32 *)dst = *(const u32 *)src;
    }
}

extern "C" int ffhip_heif_grid_compose(uint8_t *d_canvas, int64_t canvas_pitch, int out_w, int out_h, const uint8_t *d_tiles,
                                       int64_t tile_pitch, int64_t tile_stride, int tile_w, int tile_h, int rows, int cols,
                                       void *stream)
{
    if (!ffhip_have_device()) return FFHIP_ENODEV;
    if (!d_canvas || !d_tiles || out_w <= 0 || out_h <= 0 || tile_w <= 0 || tile_h <= 0 || rows <= 0 || cols <= 0) return FFHIP_EINVAL;
    /* 23008-12: the tiles must cover the canvas; the last row/column may overhang and is cropped */
    if ((long long)tile_w * cols < out_w || (long long)tile_h * rows < out_h) return FFHIP_EINVAL;
    if ((long long)tile_w * (cols - 1) >= out_w || (long long)tile_h * (rows - 1) >= out_h) return FFHIP_EINVAL;
    if (canvas_pitch < (int64_t)out_w * 4 || tile_pitch < (int64_t)tile_w * 4 || tile_stride < tile_pitch * tile_h) return FFHIP_EINVAL;
    if (((uintptr_t)d_canvas | (uintptr_t)d_tiles | (uintptr_t)canvas_pitch | (uintptr_t)tile_pitch | (uintptr_t)tile_stride) & 3) return FFHIP_EINVAL;
    GridArgs a = {d_canvas, d_tiles, canvas_pitch, tile_pitch, tile_stride, out_w, out_h, tile_w, tile_h, cols};
    const bool vec = !(tile_w & 3) && !(((uintptr_t)d_canvas | (uintptr_t)d_tiles | (uintptr_t)canvas_pitch | (uintptr_t)tile_pitch |
                                         (uintptr_t)tile_stride) & 15); /* groups of 4 px never straddle a tile */
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        dim3 grid((unsigned)((out_w + 1023) / 1024), (unsigned)out_h);
        hipLaunchKernelGGL(k_grid_compose<4>, grid, dim3(256), 0, st, a);
    } else {
        dim3 grid((unsigned)((out_w + 255) / 256), (unsigned)out_h);
        hipLaunchKernelGGL(k_grid_compose<1>, grid, dim3(256), 0, st, a);
    }
    FFHIP_CHECK(hipGetLastError(), FFHIP_EIO);
    return 0;
}
