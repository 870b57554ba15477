/* peekvit_hip_avit_train.h - C ABI of A-ViT's halting step between two encoder blocks IN TRAINING (reference models/adavit.py:170-217;
 * peekvit_amd.train_engine.ActStepFn): the update of the per-token ACT state, the halting-weighted accumulation of
 * the class rows and the masking of the halted rows in one launch, and its backward in one launch.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches
 * on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, n_cls outside
 * [1, S], a misaligned pointer; PV_ERR_UNSUPPORTED: S > PV_AVIT_MAX_S, D % 4 != 0, D > PV_AVIT_MAX_D, B * S >= 2^31).  One wave per token
 * row, plain vector stores, no atomics: every output element has one owner and every sum a fixed order, so two runs give identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build). */
#ifndef PEEKVIT_HIP_AVIT_TRAIN_H
#define PEEKVIT_HIP_AVIT_TRAIN_H

#include "peekvit_hip.h"

#define PV_AVIT_MAX_S 4096
#define PV_AVIT_MAX_D 4096
/* bits of the flag word the forward saves per token (as a small fp32 integer) */
#define PV_AVIT_REACHED 1
#define PV_AVIT_NOT_REACHED 2
#define PV_AVIT_LIVE 4

#ifdef __cplusplus
extern "C" {
#endif

/* One halting step.  y fp32 [B, S, D] is the block output and is UPDATED IN PLACE to the next block's input: the rows whose token is halted
 * after this step (m' = 0) are overwritten with zeros, every other row is left as it is.  Per token, with the fp32 [B, S] state
 * (c, R, rho, counter, m) and thr = threshold:
 *     h  = sigmoid(y[..., 0] * gate_scale - gate_center)        hh = last ? 1 : h        c' = c + hh
 *     reached = (c' > thr) * m        nr = (c' < thr)
 *     rho' = (rho + m) + R * reached        R' = R - nr * hh        counter' = counter + nr        m' = nr
 *     w  = m * (R * reached + hh * nr)
 *     acc_out[b, s, :] = acc_in[b, s, :] + y[b, s, :] * w        for the class rows s < n_cls (acc fp32 [B, n_cls, D])
 *     h_part[b] = sum over s of h        (the true h, on the last layer too; rows added in ascending order per wave, the 16 wave sums in order)
 * Every *_out pointer may be the matching *_in pointer (a token's state is read before it is written, by the same wave); otherwise the ten state
 * arrays must not overlap.  Saved for the backward: sv fp32 [3, B, S] = (h, w, flags) with flags = PV_AVIT_REACHED * reached +
 * PV_AVIT_NOT_REACHED * nr + PV_AVIT_LIVE * m, and ycls fp32 [B, n_cls, D] = the class rows of y as they were read.
 * D % 4 == 0; y / acc_in / acc_out / ycls 16-byte aligned, everything else 4-byte aligned. */
int pv_avit_act_fwd(float* y, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in,
                    float* c_out, float* R_out, float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out,
                    float* h_part, float* sv, float* ycls, int64_t B, int64_t S, int64_t D, int64_t n_cls, float gate_scale,
                    float gate_center, float threshold, int last, void* stream);

/* Its backward.  dy fp32 [B, S, D] holds the gradient of the next block's input on entry and the gradient of y on exit: the masking is invisible
 * to the gradient (the reference masks through .data), so every row passes through, and only channel 0 of each row and the class rows change:
 *     dot = sum over d of gacc[b, s, d] * ycls[b, s, d]   (s < n_cls; 0 elsewhere)
 *     dy[b, s, :] += gacc[b, s, :] * w                     (s < n_cls)
 *     dR[b, s] = gR + grho * reached + reached * dot
 *     dh = (b >= 1 ? gh / ((B - 1) * S) : 0) + (last ? 0 : nr * (m * dot - gR))
 *     dy[b, s, 0] += dh * h * (1 - h) * gate_scale
 * gR, grho fp32 [B, S] = the gradients of R' and rho'; gacc fp32 [B, n_cls, D] that of acc_out (and, unchanged, of acc_in); gh = one fp32 value
 * on the device, the gradient of the layer's score mean(h[1:]) - may be null (no score gradient).  dy16, optional (may be null): the 16-bit copy
 * of dy, whose changed elements are rewritten with the rounded new values.  sv, ycls: as the forward saved them.  dR may be gR.
 * D % 4 == 0; dy / gacc / ycls 16-byte aligned, dy16 8-byte aligned, everything else 4-byte aligned. */
int pv_avit_act_bwd(float* dy, uint16_t* dy16, const float* gR, const float* grho, const float* gacc, const float* gh, const float* sv,
                    const float* ycls, float* dR, int64_t B, int64_t S, int64_t D, int64_t n_cls, float gate_scale, int last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_AVIT_TRAIN_H */
