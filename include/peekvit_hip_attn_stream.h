/* peekvit_hip_attn_stream.h - C ABI of the streaming attention core for training: a forward that keeps its row statistics and a backward, both
 * for ANY sequence length (nothing is held per head in the LDS; the resident kernels behind pv_attention_lse_bf16 / pv_attention_bwd_bf16 stop at
 * S = 416 and S = 208 / 416).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer;
 * PV_ERR_UNSUPPORTED: dh outside {32, 48, 64}, or more than 2^31 - 1 workgroups = B * H * ceil(S / 64)).  No atomics: every sum has one owner and a
 * fixed order, so two runs give identical bits.
 *
 * Layouts are those of pv_attention_bf16 / pv_attention_bwd_bf16: qkv 16-bit [B, S, 3 * H * dh], packed q | k | v with q pre-scaled; out, dout 16-bit
 * [B, S, H * dh]; lse fp32 [B, H, S] = log2 sum_k exp(s[q, k]) (pv_attention_lse_bf16's definition).  "16-bit" is the operand type of the library
 * (bf16, or fp16 in the -DPV_OPERAND_F16 build).  16-bit arrays and dqkv 16-byte aligned, fp32 rows and the flag word 4-byte aligned. */
#ifndef PEEKVIT_HIP_ATTN_STREAM_H
#define PEEKVIT_HIP_ATTN_STREAM_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = softmax(q k^T) v and lse, by the streaming kernel (64-key blocks, online softmax) at every S >= 1; out is bit-identical to
 * pv_attention_bf16's where that entry streams too (S > 416).  range_flag as in pv_attention_bf16 (may be null). */
int pv_attention_stream_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh,
                                 uint32_t* range_flag, void* stream);

/* dqkv fp32 [B, S, 3 * H * dh] = the gradient of q | k | v given dout, from the forward's out and lse; the q third is multiplied by qscale (the
 * gradient of the unscaled q, as in pv_attention_bwd_bf16).  delta_ws fp32 [B, H, S] is caller-allocated scratch; on return it holds
 * delta[b, h, q] = sum_d dout[b, q, h, d] * out[b, q, h, d].  Two launches on the stream: dQ (and delta), then dK | dV.  P and dS = P o (dP - delta) are
 * rounded to the operand type for the products that consume them; everything else is fp32.  The fp16 build does not rescale dS: a caller whose dout
 * may be small normalises it by a power of two and undoes the factor on the fp32 result. */
int pv_attention_stream_bwd_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse,
                                 float* dqkv, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_ATTN_STREAM_H */
