/* ffhip_jpeg_prog_body.h -- the per-scan steps of a progressive JPEG (ITU-T T.81 Annex G), one body for both front ends:
 * the host decoder (ffhip_jpeg_progressive.c) and the kernel k_jpeg_huff_prog (ffhip_huff_prog_gpu.hip) instantiate the same functions
 * over the same records.  Plain C / C++ without builtins, __host__ too, so that a CPU program under a sanitizer exercises the bounds
 * logic the device runs.
 *
 * The bit source is abstract in what it stands on, not in its rules: a scan's bytes WITHOUT their stuffing (FF 00 -> FF), cut at the RSTn
 * markers into restart intervals [seg[i], seg[i + 1]).  Behind an interval's end it reads zeros and counts them (`dry`): a well-formed
 * stream looks ahead there but consumes none of it, so an interval that ends with more zero bits consumed than it holds is malformed.
 * Both front ends stage with ffhip_prog_stage_scan and therefore give the same verdict for the same bytes.
 *
 * The four steps, per block (G.1.2): DC first (G.1.2.1), DC refine (one raw bit), AC first with EOBRUN (G.1.2.2), AC refine with
 * correction bits (G.1.2.3, Figure G.7).  ffhip_prog_interval walks one restart interval of one scan and is the only caller: it owns the
 * block addressing, so nothing is written outside the picture's planes whatever the bits say.
 *
 * Verdicts (any of these makes the interval, and with it the file, FFHIP_EINVAL): a code that matches no symbol; a DC-first category
 * above 11; an AC-refine symbol with s other than 0 or 1; a run that carries k past Se (first scan or refinement, ZRL included); an EOBRUN
 * larger than the blocks left in its restart interval; more bits consumed than the interval holds. */
#ifndef FFHIP_JPEG_PROG_BODY_H
#define FFHIP_JPEG_PROG_BODY_H

#include <stdint.h>
#include "ffhip_entropy_internal.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define PROG_HD static inline __host__ __device__

/* One scan of one picture, as both front ends read it. */
struct prog_scan {
    uint32_t pic;          /* its picture among the call's */
    uint32_t ncomp;        /* components in the scan: more than one = interleaved (DC only) */
    uint32_t comp[3];      /* their indices in the frame */
    uint32_t tab[3];       /* per scan component its Huffman table among the call's tables (DC tables in a DC scan, the AC table in an AC scan) */
    uint32_t ss, se, ah, al;
    uint32_t units;        /* MCUs of an interleaved scan, blocks of the component's own grid otherwise */
    uint32_t restart;      /* units per restart interval (no DRI: units) */
    uint32_t bw;           /* blocks per row of the component's own grid (non-interleaved) */
    uint32_t data;         /* where its clean bytes start among the call's */
    uint32_t seg_base;     /* its n_seg + 1 interval bounds among the call's, relative to `data` */
    uint32_t n_seg;
    uint32_t level;        /* 1 + the largest level of the earlier scans of the picture it overlaps */
};

/* One picture: its layout and where its blocks start in the planes. */
struct prog_pic {
    uint32_t ncomp, h, v;  /* of the first component; the others are 1 x 1 */
    uint32_t mcu_cols, mcu_rows;
    uint32_t mcu_base;     /* MCUs of the call's pictures before this one */
};

struct prog_bits {
    const uint8_t *p;
    uint32_t pos, end;
    uint64_t acc;
    int n;        /* valid bits in acc */
    uint32_t dry; /* zero bytes fed behind the end */
};

/* the zig-zag order: constant memory on the device (a table local to the function is copied into LDS per lane there), a static table on the host */
#ifdef __HIP_DEVICE_COMPILE__
#define PROG_TABLE static __constant__ const
#else
#define PROG_TABLE static const
#endif
PROG_TABLE uint8_t prog_zz[64] = FFHIP_JPEG_ZIGZAG;
PROG_HD int prog_zigzag(int k) { return prog_zz[k & 63]; }

PROG_HD void prog_bits_open(struct prog_bits *b, const uint8_t *p, uint32_t pos, uint32_t end)
{
    b->p = p; b->pos = pos; b->end = end; b->acc = 0; b->n = 0; b->dry = 0;
}
PROG_HD void prog_bits_fill(struct prog_bits *b)
{
    while (b->n <= 56) {
        unsigned c = 0;
        if (b->pos < b->end) c = b->p[b->pos++];
        else b->dry++;
        b->acc = (b->acc << 8) | c;
        b->n += 8;
    }
}
PROG_HD int prog_bits_get(struct prog_bits *b, int k) /* k <= 16 */
{
    if (k == 0) return 0;
    if (b->n < k) prog_bits_fill(b);
    b->n -= k;
    return (int)((b->acc >> b->n) & ((1u << k) - 1));
}
/* one Huffman symbol, -1 if no code matches: the 9-bit look-up and canonical-code walk of the baseline host decoder */
PROG_HD int prog_huff(struct prog_bits *b, const struct huff *h)
{
    if (b->n < 16) prog_bits_fill(b);
    const unsigned peek = (unsigned)((b->acc >> (b->n - LOOK)) & ((1u << LOOK) - 1));
    const unsigned e = h->look[peek];
    if (e) { b->n -= (int)(e >> 8); return (int)(e & 0xff); }
    int code = (int)peek, len = LOOK;
    while (code > h->maxcode[len]) {
        if (++len > 16) return -1;
        code = (int)((b->acc >> (b->n - len)) & ((1u << len) - 1));
    }
    b->n -= len;
    return h->vals[(h->valptr[len] + code - h->mincode[len]) & 255]; /* & 255: a malformed DHT must not index outside the table */
}
PROG_HD int prog_extend(int v, int t) { return (t && v < (1 << (t - 1))) ? v - (1 << t) + 1 : v; }
/* the bits consumed so far do not reach behind the interval's end */
PROG_HD int prog_bits_ok(const struct prog_bits *b) { return (int)(b->dry * 8u) <= b->n; }

/* ---- the four steps: 0, or 1 for a malformed block ---- */
PROG_HD int prog_dc_first(struct prog_bits *b, const struct huff *h, int *pred, int al, int16_t *blk)
{
    const int t = prog_huff(b, h);
    if (t < 0 || t > 11) return 1;
    *pred += prog_extend(prog_bits_get(b, t), t);
    blk[0] = (int16_t)((uint32_t)*pred << al);
    return 0;
}
PROG_HD int prog_dc_refine(struct prog_bits *b, int al, int16_t *blk)
{
    if (prog_bits_get(b, 1)) blk[0] = (int16_t)(blk[0] | (1 << al));
    return 0;
}
/* left: blocks of the restart interval from this one on */
PROG_HD int prog_ac_first(struct prog_bits *b, const struct huff *h, int ss, int se, int al, uint32_t *eobrun, uint32_t left, int16_t *blk)
{
    if (*eobrun) { (*eobrun)--; return 0; }
    for (int k = ss; k <= se; k++) {
        const int rs = prog_huff(b, h);
        if (rs < 0) return 1;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > se) return 1;
            blk[prog_zigzag(k)] = (int16_t)(prog_extend(prog_bits_get(b, s), s) * (1 << al));
        } else if (r == 15) {
            k += 15;
            if (k > se) return 1; /* sixteen zeros, the last one at k */
        } else {
            const uint32_t run = (1u << r) + (uint32_t)prog_bits_get(b, r); /* this block included */
            if (run > left) return 1;
            *eobrun = run - 1;
            break;
        }
    }
    return 0;
}
/* the correction bit of an already non-zero coefficient (G.1.2.3): one step away from zero where the bit of this pass is not set yet */
PROG_HD void prog_correct(struct prog_bits *b, int al, int16_t *c)
{
    if (prog_bits_get(b, 1) && !(*c & (1 << al))) *c = (int16_t)(*c + (*c >= 0 ? (1 << al) : -(1 << al)));
}
/* The walk reads and rewrites the block where it lies.  Two forms that copy the block first and walk the copy were measured and lost (DESIGN.md
 * 4.14): 64 registers indexed by a variable, and 64 int16 of LDS per lane. */
PROG_HD int prog_ac_refine(struct prog_bits *b, const struct huff *h, int ss, int se, int al, uint32_t *eobrun, uint32_t left, int16_t *blk)
{
    int k = ss;
    if (!*eobrun) {
        for (; k <= se; k++) {
            const int rs = prog_huff(b, h);
            if (rs < 0) return 1;
            int r = rs >> 4, s = rs & 15, v = 0;
            if (s) {
                if (s != 1) return 1;
                v = prog_bits_get(b, 1) ? (1 << al) : -(1 << al); /* the new coefficient's sign comes BEFORE the correction bits */
            } else if (r != 15) {
                const uint32_t run = (1u << r) + (uint32_t)prog_bits_get(b, r); /* this block included: its correction bits follow below */
                if (run > left) return 1;
                *eobrun = run;
                break;
            }
            /* over r still-zero coefficients, correcting the non-zero ones passed on the way (Figure G.7) */
            for (; k <= se; k++) {
                int16_t *c = blk + prog_zigzag(k);
                if (*c) prog_correct(b, al, c);
                else if (--r < 0) break;
            }
            if (k > se) return 1; /* the run does not end inside the band */
            if (s) blk[prog_zigzag(k)] = (int16_t)v;
        }
    }
    if (*eobrun) {
        for (; k <= se; k++) {
            int16_t *c = blk + prog_zigzag(k);
            if (*c) prog_correct(b, al, c);
        }
        (*eobrun)--;
    }
    return 0;
}

/* Block (bx, by) of component c's own grid, as a block index into the picture's plane of that component: MCU order, h x v blocks a MCU. */
PROG_HD uint32_t prog_block_of(const struct prog_pic *pc, int first_comp, uint32_t bx, uint32_t by)
{
    const uint32_t h = first_comp ? pc->h : 1u, v = first_comp ? pc->v : 1u;
    return ((by / v) * pc->mcu_cols + bx / h) * (h * v) + (by % v) * h + bx % h;
}

/* Restart interval `iv` of scan `sc`: 0, or FFHIP_EINVAL's cause as 1.  clean = the call's staged bytes, seg = the call's interval bounds,
 * tabs = the call's tables, plane[c] = the CALL's planes (the picture's blocks start at mcu_base).  An interval the scan does not have
 * is nothing to do. */
PROG_HD int ffhip_prog_interval(const struct prog_scan *sc, const struct prog_pic *pc, uint32_t iv, const uint8_t *clean, const uint32_t *seg,
                                const struct huff *tabs, int16_t *const plane[3])
{
    if (iv >= sc->n_seg) return 0;
    struct prog_bits b;
    prog_bits_open(&b, clean + sc->data, seg[sc->seg_base + iv], seg[sc->seg_base + iv + 1]);
    uint32_t u = iv * sc->restart;
    const uint32_t u_end = sc->units - u < sc->restart ? sc->units : u + sc->restart;
    int pred[3] = {0, 0, 0};
    uint32_t eobrun = 0;
    const int ss = (int)sc->ss, se = (int)sc->se, al = (int)sc->al;
    const int refine = sc->ah != 0;
    if (sc->ncomp > 1 || ss == 0) { /* DC: interleaved over the MCUs, or one component over its own grid */
        for (; u < u_end; u++) {
            for (uint32_t k = 0; k < sc->ncomp; k++) {
                const uint32_t c = sc->comp[k], nb = c == 0 ? pc->h * pc->v : 1u;
                for (uint32_t q = 0; q < (sc->ncomp > 1 ? nb : 1u); q++) {
                    const uint32_t block = sc->ncomp > 1 ? u * nb + q : prog_block_of(pc, c == 0, u % sc->bw, u / sc->bw);
                    int16_t *blk = plane[c] + ((size_t)pc->mcu_base * nb + block) * 64;
                    if (refine ? prog_dc_refine(&b, al, blk) : prog_dc_first(&b, tabs + sc->tab[k], &pred[k], al, blk)) return 1;
                }
            }
        }
    } else {
        const uint32_t c = sc->comp[0], nb = c == 0 ? pc->h * pc->v : 1u;
        const struct huff *h = tabs + sc->tab[0];
        for (; u < u_end; u++) {
            int16_t *blk = plane[c] + ((size_t)pc->mcu_base * nb + prog_block_of(pc, c == 0, u % sc->bw, u / sc->bw)) * 64;
            if (refine ? prog_ac_refine(&b, h, ss, se, al, &eobrun, u_end - u, blk) : prog_ac_first(&b, h, ss, se, al, &eobrun, u_end - u, blk)) return 1;
        }
    }
    return prog_bits_ok(&b) ? 0 : 1;
}

#endif
