/* ffhip_entropy_internal.h -- what ffhip_entropy.c shares with the GPU entropy decoder (ffhip_huff_gpu.hip):
 * the parsed JPEG header with its Huffman look-up tables (struct huff: ffhip_jpeg_front.h).  Internal to libffpic_hip.so. */
#ifndef FFHIP_ENTROPY_INTERNAL_H
#define FFHIP_ENTROPY_INTERNAL_H

#include "ffhip_jpeg_front.h"

#ifdef __cplusplus
extern "C" {
#endif

struct jpeg_hdr {
    struct jpeg_frame fr;
    int restart;
    int td[3], ta[3];
    struct huff dc[4], ac[4];
    const uint8_t *scan;
    size_t scan_len;
};

/* marker loop, SOF/DQT/DHT/DRI/SOS parsing (format/jpg.c:78-105, 640-655, 771-855); 0 or FFHIP_EINVAL */
int ffhip_jpeg_parse(const uint8_t *file, size_t len, struct jpeg_hdr *j);
int ffhip_jpeg_probe_restart(const uint8_t *file, size_t len); /* DRI value, 0 = none, -1 = does not parse */

#ifdef __cplusplus
}
#endif
#endif
