/* peekvit_hip_rank_train.h - C ABI of what a SORTING point-cloud encoder block needs in train mode on top of include/peekvit_hip_pct_block.h
 * (peekvit_amd.pct_train.RankedPCTBlockFn).  Such a block zeroes all but the first keep of rows 1.. (by descending norm) at its
 * input and again after both LayerNorms, so its m = S - 1 - keep masked rows are identical: the block runs on L = 1 + keep live rows plus ONE tail row
 * per image that stands for the m masked ones - x = 0, both LayerNorm outputs scaled by 0, its attention key weighted by m (+ ln m on the score).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer, k or L
 * out of range, a tail_log_mult that is negative or not finite, a scratch buffer that is too small; PV_ERR_UNSUPPORTED: D % 4 != 0, D > 1024,
 * S - 1 > 4096 or B > 65535 in the four pv_rank_* row movers, dh outside {32, 48, 64}, more than 2^31 - 1 workgroups).  No atomics: every sum has one owner and a fixed order, so two runs give
 * identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build).  keep is int32 [B, k]: indices into rows 1.. (0-based,
 * pv_rank_topk's output), distinct within an image.  Compact tensors are [B, Sc, D] with Sc = L + (L < S), L = 1 + k: row 0, the kept rows in keep's
 * order, then - when a row is masked - the tail row.  fp32 arrays 16-byte aligned, keep and row_scale 4-byte aligned. */
#ifndef PEEKVIT_HIP_RANK_TRAIN_H
#define PEEKVIT_HIP_RANK_TRAIN_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xc[b, 0] = x[b, 0], xc[b, 1 + j] = x[b, 1 + keep[b, j]] (j < k), xc[b, L] = 0 when k < S - 1.  x fp32 [B, S, D]; 1 <= k <= S - 1. */
int pv_rank_pack_f32(const float* x, const int32_t* keep, float* xc, int64_t B, int64_t S, int64_t k, int64_t D, void* stream);

/* y[b, r] = yc[b, min(r, L)]: the live rows, then the tail row in every row L .. S - 1.  yc fp32 [B, L + 1, D], y fp32 [B, S, D]; 1 <= L < S. */
int pv_rank_expand_f32(const float* yc, float* y, int64_t B, int64_t S, int64_t L, int64_t D, void* stream);

/* The transpose of pv_rank_expand_f32: gc[b, r] = g[b, r] (r < L), gc[b, L] = sum of g[b, L .. S - 1] in fp32 - every element by one thread group in a
 * fixed order.  g fp32 [B, S, D], gc fp32 [B, L + 1, D]; 1 <= L < S. */
int pv_rank_reduce_f32(const float* g, float* gc, int64_t B, int64_t S, int64_t L, int64_t D, void* stream);

/* The transpose of pv_rank_pack_f32: dx[b, 0] = dxc[b, 0], dx[b, 1 + keep[b, j]] = dxc[b, 1 + j], every other row of dx = 0 (the tail row of dxc is
 * dropped: the masked rows' input is multiplied by 0); every row of dx is written.  dxc fp32 [B, Sc, D], dx fp32 [B, S, D]; 1 <= k <= S - 1. */
int pv_rank_unpack_grad_f32(const float* dxc, const int32_t* keep, float* dx, int64_t B, int64_t S, int64_t k, int64_t D, void* stream);

/* pv_layernorm_f32_bf16 (include/peekvit_hip_pct.h: its kernel, contiguous rows) with BOTH planes multiplied by row_scale[row] (fp32 [rows]) before
 * they are stored: a scale of 1 changes no bit, a scale of 0 leaves zeros in both planes.  D % 4 == 0, D <= 1024. */
int pv_layernorm_f32_bf16_masked(const float* x, const float* gamma, const float* beta, const float* row_scale, uint16_t* out16, float* out32,
                                 int64_t rows, int64_t D, float eps, void* stream);

/* pv_layernorm_bwd_sum (include/peekvit_hip_pct_block.h: its kernel, limits, scratch and arguments) for y = row_scale[row] * LN(x): the summed dy is
 * multiplied by row_scale[row] (fp32 [rows], a constant of the forward), so a row with scale 0 gives dx = 0 and adds nothing to dgamma / dbeta. */
int pv_layernorm_bwd_sum_masked(const float* x, const uint16_t* dy16, const float* dy32, const float* gamma, const float* row_scale, float* dx_out,
                                uint16_t* dx16, float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate,
                                void* stream);

/* pv_attention_stream_lse_bf16 (include/peekvit_hip_attn_stream.h: its kernel and arguments) where key S - 1 of every image stands for several
 * identical keys: tail_log_mult = ln(their number) >= 0 is added, in fp32, to every score against that key before the running maximum is taken;
 * lse includes it.  range_flag reads the scores without the bias.  tail_log_mult = 0 gives pv_attention_stream_lse_bf16's bits. */
int pv_attention_stream_lse_w_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh, float tail_log_mult,
                                   uint32_t* range_flag, void* stream);

/* pv_attention_stream_bwd16_bf16 (include/peekvit_hip_pct_block.h: its kernels and arguments) for that forward: the same tail_log_mult is added where
 * p is recomputed.  Row S - 1 of dqkv16's k | v thirds is the gradient of the shared key: the sum over the keys it stands for.  With a weight
 * (tail_log_mult > 0) a key can hold nearly all of a row's probability, where dS = p (dP - delta) cancels: delta is then formed in fp32 from what it
 * is the sum of, delta[q] = sum_k p[q, k] dP[q, k] (one more sweep over the keys in the dQ launch), not from the stored 16-bit output, and that value
 * is what delta_ws holds on return.  tail_log_mult = 0 gives pv_attention_stream_bwd16_bf16's bits, delta_ws included. */
int pv_attention_stream_bwd16_w_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16,
                                     float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale,
                                     float tail_log_mult, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_RANK_TRAIN_H */
