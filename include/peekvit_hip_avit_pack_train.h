/* peekvit_hip_avit_pack_train.h - C ABI of A-ViT's halting step IN TRAINING ON THE PACKED LIVE ROWS (DESIGN.md section 30;
 * peekvit_amd.train_engine.AViTPackStepFn): pv_avit_act_fwd's state update (include/peekvit_hip_avit_train.h) on the packed block output of
 * pv_act_step's layout (include/peekvit_hip.h), the stable compaction into the next packed input, and the backward of both.
 *
 * The packed matrix: image b is the row segment [seg_start[b], seg_start[b+1]) of y fp32 [R, D] - its live tokens in token order
 * (pos = token index) and, when n_halted[b] > 0, ONE representative row for its n_halted[b] halted tokens, last (pos = -1).  A halted token's
 * block input is 0, so its block output is the same vector for every halted token of the image; the representative's key counts n times
 * (log_mult = ln n) and its LayerNorm outputs are 0 (row_scale 0).
 *
 * What a halted token still gives the loss is h = sigmoid(y[0] * gate_scale - gate_center) in the layer's score mean(h[1:]); its gradient
 * is g = (b >= 1 ? gh / ((B - 1) S) : 0) * h (1 - h) * gate_scale on channel 0, at this layer and - the masking being invisible to autograd -
 * passed through from every later one: dy = G e_0 with G[b] = the sum of g over the layers from this one on, one fp32 scalar per image that the
 * backward walks from the last layer to the first.  A packed row that stands for n tokens carries the TOTAL gradient of its n members.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches
 * on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, n_cls outside
 * [1, S], a misaligned pointer; PV_ERR_UNSUPPORTED: S > PV_AVIT_PACK_MAX_S, n_cls > PV_AVIT_PACK_MAX_CLS, D % 4 != 0, D > PV_AVIT_PACK_MAX_D,
 * B * S or a row count beyond 2^31 - 1).  Plain vector stores, no atomics: every output element has one owner and every sum a fixed order, so two runs
 * give identical bits.  A segment that does not lie inside [0, R), is longer than S + 1 rows or names a token outside [0, S) is skipped
 * (segment) or ignored (row): nothing is read or written outside the stated sizes.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build). */
#ifndef PEEKVIT_HIP_AVIT_PACK_TRAIN_H
#define PEEKVIT_HIP_AVIT_PACK_TRAIN_H

#include "peekvit_hip.h"

#define PV_AVIT_PACK_MAX_S 256
#define PV_AVIT_PACK_MAX_CLS 16
#define PV_AVIT_PACK_MAX_D 4096
/* bits of the flag word the forward saves per INPUT ROW (as a small fp32 integer); the first three are peekvit_hip_avit_train.h's */
#define PV_AVIT_PACK_REACHED 1
#define PV_AVIT_PACK_NOT_REACHED 2
#define PV_AVIT_PACK_LIVE 4
#define PV_AVIT_PACK_MERGED 8 /* a live row whose token halts at this step: it merges into the next layer's representative row */
#define PV_AVIT_PACK_REP 16   /* the representative row */

#ifdef __cplusplus
extern "C" {
#endif

/* One halting step on the packed block output y fp32 [R, D], three launches (state update, segment scan, compaction; one when last != 0).
 * Per live row (token t = pos of the row), with the dense fp32 [B, S] state (c, R, rho, counter, m) and thr = threshold, pv_avit_act_fwd's arithmetic:
 *     h  = sigmoid(y[row, 0] * gate_scale - gate_center)        hh = last ? 1 : h        c' = c + hh
 *     reached = (c' > thr) * m        nr = (c' < thr)
 *     rho' = (rho + m) + R * reached        R' = R - nr * hh        counter' = counter + nr        m' = nr
 *     w  = m * (R * reached + hh * nr)
 *     acc_out[b, t, :] = acc_in[b, t, :] + y[row, :] * w        for t < n_cls (acc fp32 [B, n_cls, D])
 * A token without a row (halted before) keeps c, R, rho, counter and its acc row, and gets m' = 0.  h_part[b] = the sum of h over the image's live
 * rows (one per thread, summed over the wave, the four wave sums in order) + n_halted[b] * h of the representative row: the true h, on the last
 * layer too.  Every *_out pointer may be the matching *_in pointer; otherwise the state arrays must not overlap.
 * Unless `last`, the next packed input: x_next fp32 [<= R, D] = the rows with m' = 1 in order, then one ZERO row when the image has any halted
 * token (an image whose tokens have all halted keeps a segment of that one row); row_scale_next fp32 (0 on that row, 1 elsewhere), log_mult_next
 * fp32 (ln n on it, 0 elsewhere), pos_next int32, each [<= R]; seg_next int32 [B + 1]; n_halted_next int32 [B]; totals int32 [2] = (R', longest
 * segment).  With `last` these eight and src_next may be null and are not touched.
 * Saved for the backward: sv fp32 [3, R] = (h, w, flags) per input row (flags: the PV_AVIT_PACK_* bits; w = 0 on a representative row);
 * ycls fp32 [B, n_cls, D] = the class rows of y as read (zeros for a class token without a row); src_next int32 [<= R] = the input row every
 * written row came from, relative to its segment's start (-1: the zero row).
 * D % 4 == 0; y, x_next, acc_in, acc_out, ycls 16-byte aligned, everything else 4-byte aligned. */
int pv_avit_pack_step_train(const float* y, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, int64_t B, int64_t S, int64_t D,
                            int64_t R, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in,
                            float* c_out, float* R_out, float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out,
                            int64_t n_cls, float* h_part, float gate_scale, float gate_center, float threshold, int last, float* x_next,
                            float* row_scale_next, int32_t* seg_next, int32_t* n_halted_next, float* log_mult_next, int32_t* pos_next,
                            int32_t* totals, float* sv, float* ycls, int32_t* src_next, void* stream);

/* Its backward, one launch, one workgroup per image, a wave per input row.  Inputs: seg_start, n_halted, pos, sv, ycls as the forward read / wrote
 * them; seg_next, src_next and g_next fp32 [R', D] = the gradient of x_next (all three null when last != 0); gR, grho fp32 [B, S] = the gradients of
 * R' and rho'; gacc fp32 [B, n_cls, D] that of acc_out; gh = one fp32 value on the device, the gradient of the layer's score mean(h[1:]) (null: none);
 * G fp32 [B], in / out: on entry the sum of g over the LATER layers (zeros at the last layer).  With gs = (b >= 1 ? gh / ((B - 1) S) : 0):
 *     representative row:   G_new = G + gs * h (1 - h) * gate_scale;    dy[row, :] = n_halted[b] * G_new * e_0        (no such row: G_new = G)
 *     live row, token t:    dy[row, :] = its g_next row if it survived, else (merged, or last) 0, plus (merged and not last) G * e_0 - the pass-through
 *                           of every later layer's score term - and then pv_avit_act_bwd's edits with m = 1:
 *         dot = sum over d of gacc[b, t, d] * ycls[b, t, d]   (t < n_cls; 0 elsewhere)
 *         dy[row, :] += gacc[b, t, :] * w                      (t < n_cls)
 *         dh = gs + (last ? 0 : nr * (dot - gR));    dy[row, 0] += dh * h * (1 - h) * gate_scale
 *         dR[b, t] = gR + grho * reached + reached * dot
 *     token without a row:  dR[b, t] = gR[b, t]
 * and G[b] = G_new on exit.  The gradients of rho and acc pass through unchanged (grho, gacc).  dy fp32 [R, D] is written in full; dy16, optional
 * (null: none), is its 16-bit copy.  dR must not be gR.
 * D % 4 == 0; dy, g_next, gacc, ycls 16-byte aligned, dy16 8-byte aligned, everything else 4-byte aligned. */
int pv_avit_pack_step_bwd(const float* g_next, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, const int32_t* seg_next,
                          const int32_t* src_next, const float* sv, const float* ycls, const float* gR, const float* grho, const float* gacc,
                          const float* gh, float* G, float* dy, uint16_t* dy16, float* dR, int64_t B, int64_t S, int64_t D, int64_t R,
                          int64_t R_next, int64_t n_cls, float gate_scale, int last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_AVIT_PACK_TRAIN_H */
