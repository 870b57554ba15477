/* peekvit_hip_dropout.h - C ABI of dropout on the training path (peekvit_amd.train_engine): ViT and RankViT blocks keep their
 * hand-written forward and backward kernels when dropout is active.  The mask is never stored: keep(key, site, row, col) is a pure function
 * (peekvit_amd/csrc/pv_dropout.h documents it bit by bit, tests/dropout_ref.py restates it in numpy) that the forward and the backward launches of a
 * site evaluate again.  A site is a matrix [rows, cols]: element sites are [token rows, D] with (row, col) = (token row, channel); attention sites are
 * [B * H * S, S] with row = (b * H + h) * S + q and col = k.  A dropped element is 0, a kept one is multiplied by the fp32 value 1 / (1 - p).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer,
 * p < 0, p >= 1 or NaN; PV_ERR_UNSUPPORTED: D % 4 != 0, D > 4096, dh outside {32, 48, 64}, more than 2^31 - 1 workgroups).  key, site and p travel by
 * value.  No atomics: two runs with the same (key, site) give identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build); values are rounded to it once, to nearest even. */
#ifndef PEEKVIT_HIP_DROPOUT_H
#define PEEKVIT_HIP_DROPOUT_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* keep[rows, cols] (bytes) = the site's 0 / 1 decisions, through the kernels' own device function.  For tests and debugging only. */
int pv_dropout_keep_u8(uint8_t* keep, uint64_t key, uint64_t site, int64_t rows, int64_t cols, float p, void* stream);

/* out = x o keep / (1 - p), x and out fp32 [rows, D], 16-byte aligned; out may be x.  The forward of the encoder-input site and, called on the
 * gradient with the same (key, site), its backward. */
int pv_dropout_f32(const float* x, float* out, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream);

/* out = x + float(u) o keep / (1 - p) as one fused multiply-add per element: x, out fp32 [rows, D] (16-byte aligned; out may be x), u the 16-bit
 * branch output [rows, D] (8-byte aligned).  pv_masked_residual with an element mask. */
int pv_dropout_residual(const float* x, const uint16_t* u, float* out, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream);

/* du = round16(float(d) o keep / (1 - p)), d and du 16-bit [rows, D], 8-byte aligned, OUT OF PLACE (du must not be d): the gradient of the branch
 * output from the gradient behind the residual add.  The out-projection's bias gradient under branch dropout is the column sum of the STORED du. */
int pv_dropout_bwd16(const uint16_t* d, uint16_t* du, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream);

/* pv_attention_stream_lse_bf16 (include/peekvit_hip_attn_stream.h: same arguments, same kernel) with dropout on the probabilities: the softmax is of
 * all keys - the running maximum, the row sum and lse are those of the dropout-free entry point, bit for bit - and a dropped probability is set to 0
 * before it is packed for V^T P^T; 1 / (1 - p) rides in the final 1 / (l (1 - p)).  A row whose keys are all dropped is exactly 0.  p = 0 gives the
 * dropout-free entry point's bits. */
int pv_attention_stream_lse_drop_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh, float p, uint64_t key,
                                      uint64_t site, uint32_t* range_flag, void* stream);

/* pv_attention_stream_bwd16_bf16 (include/peekvit_hip_pct_block.h: same layouts, same delta_ws, same dbias_partial rows, same two launches) for that
 * forward: with M the mask, dP = dO V^T and delta = rowsum(dO o O) of the STORED output, dS = P o (M o dP / (1 - p) - delta) in fp32 with the
 * unrounded P, dQ = dS K, dK = dS^T Q, dV = (P o M)^T dO / (1 - p).  p = 0 gives pv_attention_stream_bwd16_bf16's bits. */
int pv_attention_stream_bwd16_drop_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16,
                                        float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale, float p,
                                        uint64_t key, uint64_t site, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_DROPOUT_H */
