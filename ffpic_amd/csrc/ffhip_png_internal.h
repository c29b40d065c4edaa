/* ffhip_png_internal.h -- what ffhip_inflate.c, ffhip_png.c and ffhip_png_gpu.hip share besides include/ffpic_hip.h.  Plain C. */
#ifndef FFHIP_PNG_INTERNAL_H
#define FFHIP_PNG_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_png_body.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ffhip_inflate with `partial`: a stream that holds more than cap bytes is cut there and is FFHIP_OK (*out_len == cap), the bytes behind
 * the cut and the check value not looked at: PNG's "extra bytes are ignored" */
int ffhip_inflate_upto(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial);
/* The host model of k_inflate (ffhip_inflate_model.c): ffhip_inflate_body.h with the wave's lanes emulated, every step as all 64 loads,
 * then all 64 stores.  Arguments, verdicts and bytes of ffhip_inflate_upto.  _mode: the emulation's variants, for the test of the
 * emulation itself (0 is the kernel's) */
int ffhip_inflate_model(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial);
int ffhip_inflate_model_mode(const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *out_len, int partial, int mode);

/* A file whose chunks have been walked and checked: everything of it but the picture's bytes */
typedef struct ffhip_png_file {
    ffhip_png_info info;
    ffhip_png_expand_rule rule;
    uint32_t palette[256];       /* BGRA, the tRNS alpha in it, 255 beyond tRNS; zero beyond PLTE */
    size_t first_idat;           /* offset of the first IDAT chunk's length field */
    size_t idat_bytes;           /* all IDAT payloads together */
    int idat_chunks;
} ffhip_png_file;

/* the chunk walk: signature, IHDR, PLTE, tRNS, every IDAT's and IEND's CRC.  FFHIP_EINVAL for everything "The pixel rule" refuses that
 * can be seen without inflating */
int ffhip_png_open(const uint8_t *file, size_t len, ffhip_png_file *pf);
/* the filtered picture, info.filtered_bytes of it, into `filtered`: the IDAT payloads concatenated and inflated, every row's filter byte
 * checked, and for a palette shorter than its indices' range every index.  The rows are left FILTERED */
int ffhip_png_read_filtered(const uint8_t *file, size_t len, const ffhip_png_file *pf, uint8_t *filtered);
/* the IDAT payloads of a file ffhip_png_open took, one behind the other: pf->idat_bytes into `joined` */
void ffhip_png_join_idat(const uint8_t *file, const ffhip_png_file *pf, uint8_t *joined);
/* whether ffhip_png_read_filtered checks the file's indices against its palette, for which it needs the rows unfiltered */
static inline int ffhip_png_short_palette(const ffhip_png_info *info) { return info->color_type == 3 && info->palette_size < (1 << info->bit_depth); }

#ifdef __cplusplus
}
#endif

#endif
