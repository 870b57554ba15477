/* peekvit_hip_ee.h - C ABI of the early-exit forward (reference models/eeresidualvit.py, EEResidualVisionTransformer).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises,
 * launches on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG / PV_ERR_UNSUPPORTED).
 *
 * The reference computes every layer for every image and returns one logit row per layer.  Here an image that is confident enough at a
 * checked layer leaves the batch, and the later layers run on the images that are left:
 *
 *   pv_exit_head_f32      one exit head: LayerNorm of class row 0 of every image + the fp32 linear, in one launch.
 *   pv_exit_step          max softmax per live image, the exit decision, the exiting images' results scattered to their original index,
 *                         and the stable compaction plan of the survivors (a scan: two runs give the same bits).
 *   pv_gather_images_f32  whole images copied into the compacted batch.
 */
#ifndef PEEKVIT_HIP_EE_H
#define PEEKVIT_HIP_EE_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest hidden width pv_exit_head_f32 takes (as pv_cls_pool). */
#define PV_EE_MAX_D 4096

/* Exit head of one layer.  x fp32: image b's class row is x + b * img_stride (img_stride % 4 == 0, >= D; 16-byte aligned) - row 0 of a
 * [B, S, D] block output with img_stride = S * D.  ln_gamma / ln_beta fp32 [D], w fp32 [C, D], bias fp32 [C] or null, logits fp32 [B, C].
 *   y = LayerNorm(row) with the arithmetic of pv_cls_pool (num_cls = 1), logits = w . y + bias with the arithmetic of pv_head_f32 (a fused
 *   multiply-add chain per 32-column K step, the step sums added in order): bit-identical to pv_cls_pool followed by pv_head_f32 at every
 *   batch size (B <= 16 runs one thread per logit, larger batches 32 x 64 tiles, as pv_head_f32).
 * Limits: D % 4 == 0, D <= PV_EE_MAX_D; x, ln_gamma, ln_beta and w 16-byte aligned. */
int pv_exit_head_f32(const float* x, int64_t img_stride, const float* ln_gamma, const float* ln_beta, float ln_eps, const float* w,
                     const float* bias, float* logits, int64_t B, int64_t D, int64_t C, void* stream);

/* Exit decision of one checked layer over the n_live images still running.
 *   logits   fp32 [n_live rows, ldl] (ldl >= C): the exit head's output for the live images
 *   live     int32 [n_live]: the original index of each live image, ascending, every one in [0, n_total)
 * Per row r: conf = max softmax = 1 / sum_c exp(logits[r][c] - max_c logits[r]) in fp32 (expf; one wave per row: lane l adds its columns
 * l, l + 64, ... in order, then the 64 lane sums are added by pv_wave_sum's fixed tree).  The row EXITS when conf >= threshold.
 * Outputs:
 *   row_conf   fp32 [n_live]: conf of every live row
 *   out_logits fp32 [n_total, ldo], out_layer int64 [n_total], out_conf fp32 [n_total]: for an exiting row r, row live[r] receives the logits
 *              row, `layer` and conf; the rows of surviving images are not touched
 *   next_live  int32 [n_live]: the original indices of the survivors, ascending (the first *count entries)
 *   src_row    int32 [n_live]: the row r of each survivor (what pv_gather_images_f32 takes)
 *   count      int32 [1]: the number of survivors
 * threshold = -infinity: EVERY row exits, whatever its confidence (a row with a NaN logit too, whose conf is NaN and which a finite threshold
 * keeps in the batch); count = 0 and next_live / src_row are not written (one launch).
 * A row whose live index is outside [0, n_total) exits nowhere and survives nowhere.  Limits: n_live, n_total < 2^31, C < 2^31. */
int pv_exit_step(const float* logits, int64_t ldl, const int32_t* live, int64_t n_live, int64_t C, float threshold, int64_t layer,
                 float* row_conf, float* out_logits, int64_t ldo, int64_t* out_layer, float* out_conf, int64_t n_total, int32_t* next_live,
                 int32_t* src_row, int32_t* count, void* stream);

/* Compaction of whole images: out[j] = x[src_row[j]] for j < n_out, each image_elems fp32 values (image_elems % 4 == 0, 16-byte aligned
 * buffers).  x holds n_in images; an index outside [0, n_in) copies nothing.  out must not overlap x. */
int pv_gather_images_f32(const float* x, int64_t n_in, const int32_t* src_row, int64_t n_out, int64_t image_elems, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_EE_H */
