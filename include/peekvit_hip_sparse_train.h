/* peekvit_hip_sparse_train.h - C ABI of what ResidualViT needs to TRAIN on its packed live rows, on top of
 * include/peekvit_hip_sparse.h (the packed inference forward, section 17).
 *
 * A token whose mask is exactly 0 enters its block as a zero row, leaves it as a constant and receives no gradient (relu's slope is 0 there), so
 * autograd of the packed forward gives the dense model's parameter gradients exactly.  The convention: a packed row that stands for n identical
 * tokens carries the TOTAL gradient of its n members.  Every row-wise layer's backward is linear in that gradient, so weight gradients need no
 * multiplicity factor; the weighted-key attention backward is the textbook one with + ln n on the scores (its dK | dV row is the sum over the
 * members already); the pack step's backward is the transpose of its gather.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer;
 * PV_ERR_UNSUPPORTED: dh != 64, a segment bound above PV_SPARSE_MAX_LEN, D % 4 != 0, D > 4096, more than 2^31 - 1 workgroups).  No atomics: every
 * sum has one owner and a fixed order, so two runs give identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build).  Segment tables are those of peekvit_hip_sparse.h: image
 * b is the row segment [seg_start[b], seg_start[b+1]) of a packed matrix of R rows.  A segment longer than the bound the caller states (max_len, N + 2)
 * drops out: nothing of it is read or written past that bound. */
#ifndef PEEKVIT_HIP_SPARSE_TRAIN_H
#define PEEKVIT_HIP_SPARSE_TRAIN_H

#include "peekvit_hip_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pv_attention_varlen_w_bf16 (its kernel body, arguments and limits) that also writes the rows' statistics: lse fp32 [R, H],
 * lse[r, h] = log2 sum_k exp(score[r, k] + log_mult[k]) over the keys of r's segment (pv_attention_lse_bf16's definition, the weights included).
 * `out` is pv_attention_varlen_w_bf16's, bit for bit.  qkv, out 16-byte aligned; lse, log_mult, seg_start 4-byte. */
int pv_attention_varlen_w_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg_start, const float* log_mult, int64_t B,
                                   int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream);

/* Its backward, two launches (dQ and delta, then dK | dV), every output element owned by one workgroup.
 *   qkv      16-bit [R, 3 H dh]   the forward's input (q pre-scaled)
 *   dout     16-bit [R, H dh]     the gradient of out (the caller normalises it by a power of two in the fp16 build and undoes that on the results)
 *   out, lse                      the forward's results
 *   dqkv16   16-bit [R, 3 H dh]   dq * qscale | dk | dv; the k | v row of a weighted key is the sum over the keys it stands for
 *   dbias_partial fp32 [B * nb, 3 H dh], nb = ceil(max_len / 64); optional (null: skipped): per (image, 64-row block) the column sums of the STORED
 *                                 dqkv16 values; every row is written (zeros for a block beyond its segment), so their sum is the in-projection's
 *                                 bias gradient
 *   delta_ws fp32 [R, H]          scratch; on return delta[r, h] = sum_k p dP
 * log_mult is added, in fp32, wherever p is recomputed.  A weighted key can hold nearly all of a row's probability, where dS = p (dP - delta)
 * cancels: in a segment with any non-zero log_mult, delta is formed in fp32 from sum_k p[q, k] dP[q, k] (one more sweep over the keys in the dQ
 * launch), not from the stored 16-bit output; a segment whose weights are all 0 keeps delta = sum_d dO O, pv_attention_stream_bwd16_bf16's arithmetic.
 * The grid is the worst case, B * H * nb workgroups per launch; a workgroup beyond its segment's end leaves at once.
 * qkv, dout, out, dqkv16 16-byte aligned; the fp32 and int32 arrays 4-byte. */
int pv_attention_varlen_w_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, const int32_t* seg_start,
                                     const float* log_mult, uint16_t* dqkv16, float* dbias_partial, float* delta_ws, int64_t B, int64_t max_len, int64_t H,
                                     int64_t dh, float qscale, void* stream);

/* pv_residual_pack_step (its three launches, arguments, results and limits, bit for bit) with the two tables its backward reads:
 *   gate_arg  fp32 [R]    the sigmoid's argument of every input row, (wg . row + bg) / temp + sigmoid_bias (0 on class and budget rows)
 *   src_next  int32 [R']  the input row every written row came from, relative to its segment's start (-1: the zero row)
 * thr_out is the third thing the backward needs. */
int pv_residual_pack_step_train(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                                const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                                float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                                int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta,
                                float ln_eps, uint16_t* ln_out, float* gate_arg, int32_t* src_next, void* stream);

/* Backward of that step, one launch, one workgroup per image (pv_residual_gate_bwd's arithmetic on packed rows).
 * Inputs: x, seg_start, tok_row, mask_row, gate_arg, thr (= thr_out), seg_next, src_next as the forward read / wrote them, wg, wb, temp, and
 *   g_next      fp32 [R', D]  gradient of x_next
 *   drow_scale  fp32 [R']     gradient of row_scale_next (entries of class, budget and zero rows are ignored)
 *   dmask       fp32 [B, N]   gradient of the dense mask mask_out; optional (null: zeros)
 * Outputs
 *   dx          fp32 [R, D]   class row: its g_next row; a live row: mask * g_next row + dz * wg; a row that merged into the zero row: 0;
 *                             budget row: its g_next row + du * wb
 *   dm_row      fp32 [R]      live rows: dm = <g_next row, x row> + drow_scale + the sum of dmask over the row's tokens (in token order); else 0
 *   dwg_part, dwb_part fp32 [B, D], scal_part fp32 [B, 4] = (dbg, dbb, 0, 0): per-image partials of the gradients of wg, wb, bg, bb, to be
 *                             summed over the images in a fixed order (pv_colsum_f32)
 * with dz = dm * sigmoid'(gate_arg) / temp on live rows, dthr = - sum of dm over the image's live rows, du = dthr * thr (1 - thr).
 * Limits: D % 4 == 0, D <= 4096, N + 2 <= PV_SPARSE_MAX_LEN; x, g_next, dx, wg, wb, dwg_part, dwb_part, scal_part 16-byte aligned. */
int pv_residual_pack_step_bwd(const float* x, const int32_t* seg_start, const int32_t* tok_row, const float* mask_row, const float* gate_arg,
                              const float* thr, const int32_t* seg_next, const int32_t* src_next, const float* g_next, const float* drow_scale,
                              const float* dmask, int64_t B, int64_t N, int64_t D, const float* wg, const float* wb, float temp, float* dx,
                              float* dm_row, float* dwg_part, float* dwb_part, float* scal_part, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_SPARSE_TRAIN_H */
