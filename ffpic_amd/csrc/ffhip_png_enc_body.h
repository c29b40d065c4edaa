/* ffhip_png_enc_body.h -- the PNG encoder's rule (include/ffpic_hip.h "PNG encoding") as one body for ffhip_png_enc.c (gcc)
 * and ffhip_png_enc_gpu.hip (hipcc): a source sample, the five filters of one byte, the row's choice, and the pieces of the file around the
 * deflate chunks (ffhip_deflate_body.h). */
#ifndef FFHIP_PNG_ENC_BODY_H
#define FFHIP_PNG_ENC_BODY_H

#include "ffpic_hip.h"
#include "ffhip_deflate_body.h"

#ifdef __HIPCC__
#define FFHIP_PE_FN __host__ __device__ static inline
#else
#define FFHIP_PE_FN static inline
#endif

#define FFHIP_PE_HEADER 33 /* signature and IHDR */
#define FFHIP_PE_TAIL 28   /* the IDAT of the Adler-32 and IEND */

/* byte j of row `row` of the picture in file order; 0 in front of the row and above the picture */
FFHIP_PE_FN int ffhip_pe_sample(const ffhip_png_source *s, int row, int64_t j)
{
    if (row < 0 || j < 0) return 0;
    const int64_t x = j / s->channels;
    return s->pixels[(int64_t)row * s->row_stride + x * s->pixel_stride + s->chan[j - x * s->channels]];
}

/* the five filtered values of byte j of a row, types 0..4 */
FFHIP_PE_FN void ffhip_pe_filter5(const ffhip_png_source *s, int row, int64_t j, int f[5])
{
    const int bpp = s->channels;
    const int cur = ffhip_pe_sample(s, row, j), a = ffhip_pe_sample(s, row, j - bpp), b = ffhip_pe_sample(s, row - 1, j), c = ffhip_pe_sample(s, row - 1, j - bpp);
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    const int paeth = pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
    f[0] = cur;
    f[1] = (cur - a) & 255;
    f[2] = (cur - b) & 255;
    f[3] = (cur - ((a + b) >> 1)) & 255;
    f[4] = (cur - paeth) & 255;
}

/* f[type] without a run-time index */
FFHIP_PE_FN int ffhip_pe_pick(const int f[5], int type) { return type == 0 ? f[0] : type == 1 ? f[1] : type == 2 ? f[2] : type == 3 ? f[3] : f[4]; }

/* a filtered byte read as signed 8-bit, its absolute value */
FFHIP_PE_FN uint32_t ffhip_pe_cost(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

/* the type of the smallest sum, the lowest of equal ones */
FFHIP_PE_FN int ffhip_pe_choose(const uint32_t sums[5])
{
    int t = 0;
    for (int k = 1; k < 5; k++)
        if (sums[k] < sums[t]) t = k;
    return t;
}

FFHIP_PE_FN uint64_t ffhip_pe_filtered_len(int width, int height, int channels) { return (uint64_t)height * (1 + (uint64_t)width * (uint64_t)channels); }

FFHIP_PE_FN void ffhip_pe_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

/* The IDAT chunk of deflate chunk c: length, "IDAT", the zlib header in front of chunk 0's bytes, the chunk's out_len bytes, the CRC-32.
 * ffhip_pe_idat_size: its bytes in the file.  ffhip_pe_idat_head_len: the 8 or 10 bytes in front of the deflate bytes, ffhip_pe_idat_head_byte:
 * byte k of them.  ffhip_pe_idat_crc: the chunk's CRC-32 from the CRC-32 of the deflate bytes. */
#define FFHIP_PE_CRC_IDAT 0x35AF061Eu      /* CRC-32 of "IDAT" */
#define FFHIP_PE_CRC_IDAT_ZLIB 0xEC1A7ED2u /* CRC-32 of "IDAT" 78 01 */
FFHIP_PE_FN uint32_t ffhip_pe_idat_size(int first, uint32_t out_len) { return 12u + (first ? 2u : 0u) + out_len; }
FFHIP_PE_FN int ffhip_pe_idat_head_len(int first) { return first ? 10 : 8; }
FFHIP_PE_FN uint8_t ffhip_pe_idat_head_byte(int first, uint32_t out_len, int k)
{
    const uint32_t len = out_len + (first ? 2u : 0u);
    if (k < 4) return (uint8_t)(len >> (24 - 8 * k));
    return (uint8_t)(k == 4 ? 'I' : k == 5 ? 'D' : k == 6 ? 'A' : k == 7 ? 'T' : k == 8 ? 0x78 : 0x01);
}
FFHIP_PE_FN uint32_t ffhip_pe_idat_crc(int first, uint32_t out_len, uint32_t data_crc)
{
    return ffhip_def_crc_join(first ? FFHIP_PE_CRC_IDAT_ZLIB : FFHIP_PE_CRC_IDAT, data_crc, ffhip_def_crc_x8n(out_len));
}

/* behind the last deflate chunk: an IDAT of the four bytes of the Adler-32 (a, b), then IEND */
FFHIP_PE_FN void ffhip_pe_tail(uint32_t a, uint32_t b, uint8_t tail[FFHIP_PE_TAIL])
{
    ffhip_pe_be32(tail, 4);
    tail[4] = 'I'; tail[5] = 'D'; tail[6] = 'A'; tail[7] = 'T';
    ffhip_pe_be32(tail + 8, (b << 16) | a);
    ffhip_pe_be32(tail + 12, ffhip_def_crc_bytes(0, tail + 4, 8));
    ffhip_pe_be32(tail + 16, 0);
    tail[20] = 'I'; tail[21] = 'E'; tail[22] = 'N'; tail[23] = 'D';
    ffhip_pe_be32(tail + 24, ffhip_def_crc_bytes(0, tail + 20, 4));
}

#endif
