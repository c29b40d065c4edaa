/* ffhip_inflate_gpu.h -- k_inflate's record and launch (ffhip_inflate_gpu.hip), for its two callers: ffhip_inflate_streams_device there and
 * the FFHIP_PNG_INFLATE_DEVICE front end of ffhip_png_gpu.hip. */
#ifndef FFHIP_INFLATE_GPU_H
#define FFHIP_INFLATE_GPU_H

#include "ffhip_internal.h"

/* One zlib stream.  The kernel reads src[0 .. len), writes dst[0 .. out_len) with out_len <= cap, and status and out_len here */
struct FfhipInflateRec {
    const uint8_t *src; /* device */
    uint8_t *dst;       /* device */
    unsigned long long len, cap;
    unsigned long long out_len;
    int status;
    u32 partial;        /* ffhip_inflate_upto's: output beyond cap ends the decode with success */
    u32 index;          /* the caller's: records are sorted */
    u32 png;            /* the PNG tail: the output must be exactly cap bytes, and every row of rows[p] rows at pitch[p] starts with a filter byte <= 4 */
    u32 rows[7], pitch[7];
};

/* longest stream first: the tail of a launch is then the short streams, and a workgroup's record is its index */
void ffhip_inflate_sort(std::vector<FfhipInflateRec> &rec);
/* k_inflate over d_rec[0 .. n), one 64-thread workgroup per record.  Only enqueues */
int ffhip_inflate_launch(FfhipInflateRec *d_rec, size_t n, void *stream);

#endif
