/*
 * ffhip_exif.c -- the EXIF orientation tag of a JPEG, WebP or PNG file, and the host side of the eight orientations: sizes, rectangles,
 * inverses (include/ffpic_hip.h, "EXIF orientation").  Plain C11, no HIP.
 *
 * The reference skips APP1 (format/jpg.c:836-840) and does not look at the WebP `EXIF` chunk, and so do the decoders here: these
 * functions read the files a second time, on their own, and nothing they find can fail a decode.  Written from the EXIF 2.3 / TIFF 6.0
 * layout:
 *   JPEG   SOI, marker segments; APP1 (FFE1) with payload "Exif\0\0" + TIFF
 *   WebP   "RIFF" size "WEBP", chunks (tag, 32-bit little-endian size, payload, a padding byte behind an odd size); `EXIF` = TIFF
 *   PNG    the signature, chunks (32-bit big-endian length, type, payload, CRC); the first `eXIf` = TIFF
 *   TIFF   "II*\0" (little-endian) or "MM\0*" (big-endian), the 32-bit offset of IFD0 from the header's first byte; IFD0 = a 16-bit entry
 *          count and that many 12-byte entries: tag (16), type (16), count (32), value or offset (32, a value shorter than that left-aligned)
 * Every read is checked against the end of its segment or chunk, which is checked against the end of the file; every loop moves forward
 * by at least one byte per turn or counts entries that were checked to exist.
 */
#include "ffpic_hip.h"
#include "ffhip_orient_body.h"
#include "ffhip_jpeg_front.h"

#include <string.h>

static uint32_t tiff16(const uint8_t *p, int be) { return be ? (uint32_t)p[0] << 8 | p[1] : (uint32_t)p[1] << 8 | p[0]; }
static uint32_t tiff32(const uint8_t *p, int be)
{
    return be ? (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]
              : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
}

/* the TIFF structure t[0 .. n): the orientation, 1 where there is none to be had */
static int tiff_orientation(const uint8_t *t, size_t n)
{
    if (n < 8) return 1;
    int be;
    if (t[0] == 'I' && t[1] == 'I' && t[2] == 0x2a && t[3] == 0) be = 0;
    else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2a) be = 1;
    else return 1;
    const size_t ifd = tiff32(t + 4, be);
    if (ifd > n || n - ifd < 2) return 1;
    const size_t count = tiff16(t + ifd, be);
    if ((n - ifd - 2) / 12 < count) return 1; /* more entries than the structure holds */
    for (size_t e = 0; e < count; e++) {
        const uint8_t *p = t + ifd + 2 + 12 * e;
        if (tiff16(p, be) != 0x0112) continue;
        const uint32_t type = tiff16(p + 2, be);
        if (tiff32(p + 4, be) != 1) return 1;
        const uint32_t v = type == 3 ? tiff16(p + 8, be) : type == 4 ? tiff32(p + 8, be) : 0;
        return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
}

int ffhip_jpeg_exif_orientation(const uint8_t *file, size_t len, int *orientation)
{
    if (!file || !orientation) return FFHIP_EINVAL;
    *orientation = 1;
    struct jpeg_walk w;
    if (ffhip_jpeg_walk_open(&w, file, len)) return FFHIP_OK;
    for (;;) {
        const enum jpeg_event ev = ffhip_jpeg_walk_next(&w);
        if (ev == JPEG_STANDALONE) continue;
        if (ev != JPEG_SEGMENT || w.marker == 0xDA) break; /* EOI, SOS: no tag in front of the picture; a malformed file or its end fails nothing */
        if (w.marker == 0xE1 && w.seg_len >= 6 && memcmp(w.seg, "Exif\0\0", 6) == 0) {
            *orientation = tiff_orientation(w.seg + 6, w.seg_len - 6);
            break;
        }
    }
    return FFHIP_OK;
}

int ffhip_webp_exif_orientation(const uint8_t *file, size_t len, int *orientation)
{
    if (!file || !orientation) return FFHIP_EINVAL;
    *orientation = 1;
    if (len < 12 || memcmp(file, "RIFF", 4) != 0 || memcmp(file + 8, "WEBP", 4) != 0) return FFHIP_OK;
    size_t p = 12;
    while (len - p >= 8) {
        const size_t size = tiff32(file + p + 4, 0);
        if (size > len - p - 8) return FFHIP_OK;
        if (memcmp(file + p, "EXIF", 4) == 0) {
            const uint8_t *t = file + p + 8;
            const size_t skip = size >= 6 && memcmp(t, "Exif\0\0", 6) == 0 ? 6 : 0;
            *orientation = tiff_orientation(t + skip, size - skip);
            return FFHIP_OK;
        }
        const size_t step = 8 + size + (size & 1);
        if (step > len - p) return FFHIP_OK; /* the padding byte is missing: the last chunk */
        p += step;
    }
    return FFHIP_OK;
}

int ffhip_png_exif_orientation(const uint8_t *file, size_t len, int *orientation)
{
    if (!file || !orientation) return FFHIP_EINVAL;
    *orientation = 1;
    if (len < 8 || memcmp(file, "\x89PNG\r\n\x1a\n", 8) != 0) return FFHIP_OK;
    size_t p = 8;
    while (len - p >= 12) { /* length, type, payload, CRC: walked by the lengths; eXIf may stand behind the picture */
        const size_t size = tiff32(file + p, 1);
        if (size > len - p - 12) return FFHIP_OK;
        if (memcmp(file + p + 4, "eXIf", 4) == 0) {
            *orientation = tiff_orientation(file + p + 8, size);
            return FFHIP_OK;
        }
        p += size + 12;
    }
    return FFHIP_OK;
}

int ffhip_orient_size(int w, int h, int o, int *uw, int *uh)
{
    if (o < 1 || o > 8 || w < 1 || h < 1 || !uw || !uh) return FFHIP_EINVAL;
    *uw = FFHIP_ORIENT_TRANSPOSE(o) ? h : w;
    *uh = FFHIP_ORIENT_TRANSPOSE(o) ? w : h;
    return FFHIP_OK;
}

int ffhip_orient_rect(int ws, int hs, int o, const ffhip_rect *upright, ffhip_rect *stored)
{
    int uw, uh;
    if (!upright || !stored || ffhip_orient_size(ws, hs, o, &uw, &uh)) return FFHIP_EINVAL;
    const ffhip_rect r = *upright;
    if (r.x0 < 0 || r.y0 < 0 || r.width < 1 || r.height < 1 || (long long)r.x0 + r.width > uw || (long long)r.y0 + r.height > uh) return FFHIP_EINVAL;
    /* two opposite corners, mapped; the stored rectangle lies between them */
    int ax, ay, bx, by;
    ffhip_orient_stored_of(o, ws, hs, r.x0, r.y0, &ax, &ay);
    ffhip_orient_stored_of(o, ws, hs, r.x0 + r.width - 1, r.y0 + r.height - 1, &bx, &by);
    stored->x0 = ax < bx ? ax : bx;
    stored->y0 = ay < by ? ay : by;
    stored->width = FFHIP_ORIENT_TRANSPOSE(o) ? r.height : r.width;
    stored->height = FFHIP_ORIENT_TRANSPOSE(o) ? r.width : r.height;
    return FFHIP_OK;
}

int ffhip_orient_inverse(int o)
{
    if (o < 1 || o > 8) return FFHIP_EINVAL;
    return o == 6 ? 8 : o == 8 ? 6 : o;
}
