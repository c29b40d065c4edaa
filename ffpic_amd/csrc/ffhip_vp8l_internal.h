/* ffhip_vp8l_internal.h -- what ffhip_vp8l.c and ffhip_vp8l_gpu.hip share besides include/ffpic_hip.h.  Plain C. */
#ifndef FFHIP_VP8L_INTERNAL_H
#define FFHIP_VP8L_INTERNAL_H

#include "ffpic_hip.h"
#include "ffhip_vp8l_body.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A file whose container, header and transform list have been read: everything of it but the residual image.  The block images are the
 * transforms' sub-images as the stream holds them, one ARGB word a block, on the heap: ffhip_vp8l_close frees them */
typedef struct ffhip_vp8l_file {
    ffhip_vp8l_info info;
    ffhip_vp8l_steps steps;      /* the device form; valid while device_form */
    int device_form;             /* colour indexing absent, or the first transform of the file */
    const uint8_t *stream;       /* the VP8L chunk behind its signature byte and header: the first transform bit on */
    size_t stream_len;
    int lenient_end;             /* an ALPH stream whose one transform is colour indexing: see ffhip_vp8l_open_stream */
    uint64_t image_bit;          /* where the residual image begins in it */
    uint32_t xsize[4];           /* by transform: the width of the image it is undone on */
    uint32_t *predictor_image, *cross_image;
    uint32_t predictor_words, cross_words;
    uint32_t palette[256];       /* 0x00000000 beyond the file's entries */
} ffhip_vp8l_file;

/* FFHIP_EINVAL for everything "lossless WebP" refuses in front of the residual image */
int ffhip_vp8l_open(const uint8_t *file, size_t len, ffhip_vp8l_file *pf);
/* The same behind container and header -- ffhip_vp8l_open is those two and a call of this: a bare stream that starts at the first
 * transform bit, of a width x height picture.  alpha_plane: the stream of a lossy file's ALPH chunk ("lossy WebP, the alpha plane").
 * libwebp decodes such a stream by a loop of its own when colour indexing is its one transform, the residual image has no colour
 * cache and all its red, blue and alpha codes have one symbol, and that loop lets the LAST token of the image take bits from behind
 * the chunk's end; ffhip_vp8l_read_residual does the same for these streams (lenient_end) and for no other, and reads that token as
 * libwebp's reader does (ffhip_vp8l.c, tail_*) */
int ffhip_vp8l_open_stream(const uint8_t *stream, size_t len, int32_t width, int32_t height, int32_t has_alpha, int alpha_plane, ffhip_vp8l_file *pf);
void ffhip_vp8l_close(ffhip_vp8l_file *pf);
/* the residual image, info.residual_width x height words, into `residual` */
int ffhip_vp8l_read_residual(const ffhip_vp8l_file *pf, uint32_t *residual);
/* every transform undone on the host by the functions of ffhip_vp8l_body.h: residual -> width x height ARGB words at `argb` (rows
 * packed), the alpha rule not yet applied.  residual is used up */
int ffhip_vp8l_invert_host(const ffhip_vp8l_file *pf, uint32_t *residual, uint32_t *argb);

#ifdef __cplusplus
}

#include <vector>

/* opened files and their owner: the block images are the files' own heap */
struct Vp8lFiles {
    std::vector<ffhip_vp8l_file> v;
    explicit Vp8lFiles(size_t n) : v(n) {}
    Vp8lFiles(const Vp8lFiles &) = delete;
    ~Vp8lFiles() { for (ffhip_vp8l_file &f : v) ffhip_vp8l_close(&f); }
};

struct StageClock; /* ffhip_staged.h */

/* ---- what ffhip_vp8l_gpu.hip lends ffhip_webp_alpha_gpu.hip, the block marked so there: its part layout, its host stage and its two
 * kernels' launches ----
 * a file's place in its part's staging: the residual image (a host-form file: its finished pixels), then what the kernels read beside it */
struct Vp8lPartFile { int idx; size_t res_off, modes_off, cross_off, palette_off; };
/* file `idx` behind *res bytes of residual images and *side bytes beside them; both grow; -> the part's bytes so far */
size_t vp8l_part_add(std::vector<Vp8lPartFile> &part, const ffhip_vp8l_file &f, int idx, size_t *res, size_t *side);
/* behind the part's last file: the side data follow the `res` bytes of residual images */
void vp8l_part_seal(std::vector<Vp8lPartFile> &part, size_t res);
/* a host thread's work on one file: its stream decoded into the staging at `pin`; -> the file's status */
int vp8l_stage_file(const ffhip_vp8l_file &f, const Vp8lPartFile &p, uint8_t *pin);
/* k_vp8l_predict's levels and k_vp8l_finish over the part's files with status[idx] == 0, the staging uploaded to `dev`; pf, d_bgra, pitch
 * and status are indexed by Vp8lPartFile::idx; the records go through scratch kinds kind + 1 and kind + 2.  counts[0] += launches of
 * k_vp8l_predict, counts[1] += files the host inverted; a clock is marked from 2 behind the predict launches and from 3 behind the finish
 * launch, NULL is not */
int vp8l_enqueue_part(const std::vector<Vp8lPartFile> &part, uint8_t *dev, const ffhip_vp8l_file *pf, uint8_t *const *d_bgra, const int64_t *pitch,
                      const int *status, void *stream, int kind, int counts[2], StageClock *clock);
#endif

#endif
