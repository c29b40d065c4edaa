/*
 * ffhip_png.c -- the host side of the PNG calls (include/ffpic_hip.h, "PNG"): the probe, the chunk walk with its CRCs, the
 * filtered picture out of the IDAT chunks (ffhip_inflate.c), and ffhip_png_picture, the whole decode on the host with the functions of
 * ffhip_png_body.h that the kernels compile too.  Plain C11, no HIP.
 *
 * Written from the PNG specification (ISO/IEC 15948):
 *   file    the 8-byte signature, then chunks: length (32, big-endian), type (4 letters), payload, CRC-32 of type and payload
 *   IHDR    width (32), height (32), bit depth, colour type, compression, filter, interlace: 13 bytes, the first chunk
 *   PLTE    up to 256 RGB triples;  tRNS  alpha per palette entry, or the 16-bit grey sample / RGB triple that is transparent
 *   IDAT    one zlib stream over all of them: per pass of the picture, per row, a filter byte and the row's packed samples
 * Every read is checked against the end of its chunk, which is checked against the end of the file.
 */
#include "ffhip_png_internal.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

/* CRC-32 (reflected 0xEDB88320), eight bytes at a time over eight tables made at first use */
static uint32_t crc_table[8][256];
static pthread_once_t crc_once = PTHREAD_ONCE_INIT;

static void crc_make(void)
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        crc_table[0][i] = c;
    }
    for (int t = 1; t < 8; t++)
        for (uint32_t i = 0; i < 256; i++) crc_table[t][i] = crc_table[0][crc_table[t - 1][i] & 255] ^ (crc_table[t - 1][i] >> 8);
}

static uint32_t crc32_of(const uint8_t *p, size_t n)
{
    pthread_once(&crc_once, crc_make);
    uint32_t c = 0xffffffffu;
    for (; n >= 8; n -= 8, p += 8) {
        const uint32_t a = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        c = crc_table[7][a & 255] ^ crc_table[6][(a >> 8) & 255] ^ crc_table[5][(a >> 16) & 255] ^ crc_table[4][a >> 24] ^
            crc_table[3][p[4]] ^ crc_table[2][p[5]] ^ crc_table[1][p[6]] ^ crc_table[0][p[7]];
    }
    while (n--) c = crc_table[0][(c ^ *p++) & 255] ^ (c >> 8);
    return ~c;
}

static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

/* the chunk at file[at]: its payload length, 0 where it does not fit the file */
static int chunk_at(const uint8_t *file, size_t len, size_t at, uint32_t *size)
{
    if (len - at < 12) return 0;
    *size = be32(file + at);
    return *size <= 0x7fffffffu && *size <= len - at - 12;
}
static int chunk_is(const uint8_t *file, size_t at, const char *type) { return memcmp(file + at + 4, type, 4) == 0; }
static int chunk_crc_ok(const uint8_t *file, size_t at, uint32_t size) { return crc32_of(file + at + 4, (size_t)size + 4) == be32(file + at + 8 + size); }

/* the header's fields and what follows from them; the chunks behind IHDR are not looked at */
static int png_header(const uint8_t *file, size_t len, ffhip_png_info *info)
{
    uint32_t size;
    memset(info, 0, sizeof(*info));
    if (len < 8 || memcmp(file, png_sig, 8) != 0) return FFHIP_EINVAL;
    if (!chunk_at(file, len, 8, &size) || size != 13 || !chunk_is(file, 8, "IHDR") || !chunk_crc_ok(file, 8, 13)) return FFHIP_EINVAL;
    const uint8_t *h = file + 16;
    const uint32_t w = be32(h), ht = be32(h + 4);
    const int depth = h[8], ctype = h[9], channels = ffhip_png_channels(ctype, depth);
    if (w < 1 || w > 65535 || ht < 1 || ht > 65535 || !channels || h[10] != 0 || h[11] != 0 || h[12] > 1) return FFHIP_EINVAL;
    info->width = (int32_t)w;
    info->height = (int32_t)ht;
    info->bit_depth = depth;
    info->color_type = ctype;
    info->interlace = h[12];
    for (int p = 0; p < (h[12] ? 7 : 1); p++) {
        uint32_t pw = w, ph = ht;
        if (h[12]) ffhip_png_adam7_size(p, w, ht, &pw, &ph);
        if (!pw || !ph) continue;
        info->pass_rows[p] = (int32_t)ph;
        info->pass_row_bytes[p] = (int32_t)(((uint64_t)pw * (uint32_t)(channels * depth) + 7) / 8);
        info->filtered_bytes += (uint64_t)ph * ((uint64_t)info->pass_row_bytes[p] + 1);
        info->n_passes++;
    }
    return FFHIP_OK;
}

/* the chunks between IHDR and the first IDAT: PLTE and tRNS, each checked only where `crc`.  *idat is the first IDAT's offset */
static int png_front(const uint8_t *file, size_t len, int crc, ffhip_png_file *pf, size_t *idat)
{
    ffhip_png_info *info = &pf->info;
    const int ctype = info->color_type, depth = info->bit_depth;
    size_t at = 8 + 25;
    uint32_t size;
    int have_plte = 0;
    const uint8_t *trns = NULL;
    uint32_t trns_len = 0;
    for (;; at += (size_t)size + 12) {
        if (!chunk_at(file, len, at, &size)) return FFHIP_EINVAL; /* no IDAT */
        if (chunk_is(file, at, "IDAT")) break;
        if (chunk_is(file, at, "PLTE")) {
            if (crc && !chunk_crc_ok(file, at, size)) return FFHIP_EINVAL;
            if (have_plte || size == 0 || size % 3 || size > 768) return FFHIP_EINVAL;
            have_plte = 1;
            if (ctype != 3) continue; /* a suggested palette: not used */
            info->palette_size = (int32_t)(size / 3);
            for (uint32_t k = 0; k < size / 3; k++) {
                const uint8_t *e = file + at + 8 + 3 * k;
                pf->palette[k] = ffhip_png_bgra(e[2], e[1], e[0], 255);
            }
        } else if (chunk_is(file, at, "tRNS")) {
            if (crc && !chunk_crc_ok(file, at, size)) return FFHIP_EINVAL;
            if (!trns) { trns = file + at + 8; trns_len = size; }
        } else if (chunk_is(file, at, "IEND") || chunk_is(file, at, "IHDR") || !(file[at + 4] & 0x20)) {
            return FFHIP_EINVAL; /* the end before the picture, a second header, a critical chunk this decoder does not know */
        }
    }
    *idat = at;
    if (ctype == 3 && !have_plte) return FFHIP_EINVAL;
    /* tRNS as libpng takes it: of the right length for the colour type (at most the palette's), and in front of IDAT; otherwise ignored */
    if (trns && ctype == 3 && trns_len >= 1 && trns_len <= (uint32_t)info->palette_size) {
        info->has_trns = 1;
        for (uint32_t k = 0; k < trns_len; k++) pf->palette[k] = (pf->palette[k] & 0x00ffffffu) | (uint32_t)trns[k] << 24;
    } else if (trns && ((ctype == 0 && trns_len == 2) || (ctype == 2 && trns_len == 6))) {
        const uint32_t mask = depth == 16 ? 0xffffu : (1u << depth) - 1;
        info->has_trns = 1;
        for (uint32_t k = 0; k < trns_len / 2; k++) pf->rule.key[k] = (uint16_t)(((uint32_t)trns[2 * k] << 8 | trns[2 * k + 1]) & mask);
    }
    pf->rule.ctype = (uint8_t)ctype;
    pf->rule.depth = (uint8_t)depth;
    pf->rule.has_trns = (uint8_t)info->has_trns;
    pf->rule.interlace = (uint8_t)info->interlace;
    return FFHIP_OK;
}

int ffhip_png_probe(const uint8_t *file, size_t len, ffhip_png_info *info)
{
    if (!file || !info) return FFHIP_EINVAL;
    ffhip_png_file pf;
    memset(&pf, 0, sizeof(pf));
    int rc = png_header(file, len, &pf.info);
    size_t idat;
    if (!rc) rc = png_front(file, len, 0, &pf, &idat);
    *info = pf.info;
    if (rc) memset(info, 0, sizeof(*info));
    return rc;
}

int ffhip_png_open(const uint8_t *file, size_t len, ffhip_png_file *pf)
{
    if (!file || !pf) return FFHIP_EINVAL;
    memset(pf, 0, sizeof(*pf));
    int rc = png_header(file, len, &pf->info);
    if (!rc) rc = png_front(file, len, 1, pf, &pf->first_idat);
    if (rc) return rc;
    /* from the first IDAT on: every IDAT checked and counted, ancillary chunks skipped by their length, IEND checked and required */
    size_t at = pf->first_idat;
    uint32_t size;
    for (;; at += (size_t)size + 12) {
        if (!chunk_at(file, len, at, &size)) return FFHIP_EINVAL; /* the file ends without IEND, or in the middle of a chunk */
        if (chunk_is(file, at, "IDAT")) {
            if (!chunk_crc_ok(file, at, size)) return FFHIP_EINVAL;
            pf->idat_bytes += size;
            pf->idat_chunks++;
        } else if (chunk_is(file, at, "IEND")) {
            return chunk_crc_ok(file, at, size) ? FFHIP_OK : FFHIP_EINVAL;
        } else if (chunk_is(file, at, "tRNS") || chunk_is(file, at, "PLTE")) {
            if (!chunk_crc_ok(file, at, size)) return FFHIP_EINVAL; /* out of place and not used, but a chunk whose damage counts */
        } else if (!(file[at + 4] & 0x20)) {
            return FFHIP_EINVAL;
        }
    }
}

void ffhip_png_join_idat(const uint8_t *file, const ffhip_png_file *pf, uint8_t *joined)
{
    uint32_t size = 0;
    size_t at = pf->first_idat, got = 0;
    for (int k = 0; k < pf->idat_chunks; at += (size_t)size + 12) { /* the walk ffhip_png_open has made: every chunk fits the file */
        size = be32(file + at);
        if (!chunk_is(file, at, "IDAT")) continue;
        memcpy(joined + got, file + at + 8, size);
        got += size;
        k++;
    }
}

int ffhip_png_read_filtered(const uint8_t *file, size_t len, const ffhip_png_file *pf, uint8_t *filtered)
{
    const ffhip_png_info *info = &pf->info;
    const uint8_t *z = NULL;
    uint8_t *joined = NULL;
    if (pf->idat_chunks == 1) { /* the stream lies in the file as it is */
        z = file + pf->first_idat + 8;
    } else {
        joined = (uint8_t *)malloc(pf->idat_bytes ? pf->idat_bytes : 1);
        if (!joined) return FFHIP_ENOMEM;
        ffhip_png_join_idat(file, pf, joined);
        z = joined;
    }
    (void)len;
    size_t out = 0;
    int rc = ffhip_inflate_upto(z, pf->idat_bytes, filtered, (size_t)info->filtered_bytes, &out, 1);
    free(joined);
    if (rc) return rc;
    if (out != info->filtered_bytes) return FFHIP_EINVAL; /* the stream ends short of the picture */
    const uint8_t *sub = filtered;
    for (int p = 0; p < 7; p++) {
        const uint64_t pitch = (uint64_t)info->pass_row_bytes[p] + 1;
        for (int32_t y = 0; y < info->pass_rows[p]; y++)
            if (sub[y * pitch] > 4) return FFHIP_EINVAL;
        sub += pitch * (uint64_t)info->pass_rows[p];
    }
    if (!ffhip_png_short_palette(info)) return FFHIP_OK;
    /* a palette shorter than its indices' range: the indices are known only once the rows are unfiltered, which is done on a copy -- the
     * caller's rows stay filtered, for the device or the host to unfilter as every other file's */
    uint8_t *copy = (uint8_t *)malloc((size_t)info->filtered_bytes);
    if (!copy) return FFHIP_ENOMEM;
    memcpy(copy, filtered, (size_t)info->filtered_bytes);
    uint8_t *s = copy;
    for (int p = 0; p < 7 && !rc; p++) {
        const uint64_t pitch = (uint64_t)info->pass_row_bytes[p] + 1;
        if (!info->pass_rows[p]) continue;
        ffhip_png_unfilter_rows(s, (uint32_t)info->pass_rows[p], (uint32_t)info->pass_row_bytes[p], 1);
        uint32_t w = (uint32_t)info->width, h = (uint32_t)info->height;
        if (info->interlace) ffhip_png_adam7_size(p, (uint32_t)info->width, (uint32_t)info->height, &w, &h);
        for (int32_t y = 0; y < info->pass_rows[p] && !rc; y++)
            for (uint32_t x = 0; x < w; x++)
                if (ffhip_png_sample(s + y * pitch + 1, x, info->bit_depth) >= (uint32_t)info->palette_size) { rc = FFHIP_EINVAL; break; }
        s += pitch * (uint64_t)info->pass_rows[p];
    }
    free(copy);
    return rc;
}

/* the unfiltered sub-images -> the picture, by the rule's pixel function and the Adam7 map */
static void png_expand(const ffhip_png_file *pf, const uint8_t *rows, uint8_t *bgra, int64_t pitch)
{
    const ffhip_png_info *info = &pf->info;
    const uint8_t *base[7];
    uint64_t at = 0;
    for (int p = 0; p < 7; p++) {
        base[p] = rows + at;
        at += ((uint64_t)info->pass_row_bytes[p] + 1) * (uint64_t)info->pass_rows[p];
    }
    for (uint32_t y = 0; y < (uint32_t)info->height; y++) {
        uint8_t *out = bgra + (int64_t)y * pitch;
        for (uint32_t x = 0; x < (uint32_t)info->width; x++) {
            uint32_t px = x, py = y;
            const int p = info->interlace ? ffhip_png_adam7_of(x, y, &px, &py) : 0;
            const uint32_t v = ffhip_png_pixel(&pf->rule, base[p] + py * ((uint64_t)info->pass_row_bytes[p] + 1) + 1, px, pf->palette);
            out[4 * x] = (uint8_t)v;
            out[4 * x + 1] = (uint8_t)(v >> 8);
            out[4 * x + 2] = (uint8_t)(v >> 16);
            out[4 * x + 3] = (uint8_t)(v >> 24);
        }
    }
}

int ffhip_png_picture(const uint8_t *file, size_t len, uint8_t *bgra, int64_t pitch)
{
    if (!file || !bgra) return FFHIP_EINVAL;
    ffhip_png_file *pf = (ffhip_png_file *)malloc(sizeof(*pf));
    if (!pf) return FFHIP_ENOMEM;
    int rc = ffhip_png_open(file, len, pf);
    if (!rc && pitch < 4LL * pf->info.width) rc = FFHIP_EINVAL;
    uint8_t *rows = NULL;
    if (!rc && !(rows = (uint8_t *)malloc((size_t)pf->info.filtered_bytes))) rc = FFHIP_ENOMEM;
    if (!rc) rc = ffhip_png_read_filtered(file, len, pf, rows);
    if (!rc) {
        uint8_t *sub = rows;
        const int bpp = ffhip_png_bpp(pf->info.color_type, pf->info.bit_depth);
        for (int p = 0; p < 7; p++) {
            if (!pf->info.pass_rows[p]) continue;
            ffhip_png_unfilter_rows(sub, (uint32_t)pf->info.pass_rows[p], (uint32_t)pf->info.pass_row_bytes[p], bpp);
            sub += ((uint64_t)pf->info.pass_row_bytes[p] + 1) * (uint64_t)pf->info.pass_rows[p];
        }
        png_expand(pf, rows, bgra, pitch);
    }
    free(rows);
    free(pf);
    return rc;
}
