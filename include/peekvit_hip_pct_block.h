/* peekvit_hip_pct_block.h - C ABI of the two kernels a whole point-cloud encoder block needs on top of the image models' training kernels
 * (peekvit_amd.pct_train.PCTBlockFn).  PCTBlock adds its first residual to the LayerNorm OUTPUT - u = ln_1(x),
 * v = attn(u) + u, out = mlp(ln_2(v)) + v - so that residual's gradient does not bypass LayerNorm 1: it is a second term of the LayerNorm's own dy.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer, a
 * scratch buffer that is too small; PV_ERR_UNSUPPORTED: D % 4 != 0, D > 1024, dh outside {32, 48, 64}, more than 2^31 - 1 workgroups).  No atomics:
 * every sum has one owner and a fixed order, so two runs give identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build); values are rounded to it once, to nearest even. */
#ifndef PEEKVIT_HIP_PCT_BLOCK_H
#define PEEKVIT_HIP_PCT_BLOCK_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LayerNorm backward whose incoming gradient is a SUM: dy = float(dy16) + dy32, formed in fp32 and never rounded (either term may be null, not
 * both), dx = LN'(x)^T dy with the statistics recomputed from x (fp32 [rows, D], the saved LayerNorm input).  dx_out fp32 and dx16 16-bit are each
 * optional, not both null.  dgb fp32 [3, D] (+)= (dgamma, dbeta, column sums of dx - of its 16-bit values when dx16 is given), as in
 * pv_layernorm_bwd, whose kernel this is: same limits (D % 4 == 0, D <= 1024, any rows), same scratch (pv_workspace_size(PV_WS_LAYERNORM_BWD)
 * bytes in ws, ws_floats of them given), same accumulate flag.  x, dy32, gamma, dx_out, dgb, ws 16-byte aligned; dy16, dx16 8-byte aligned. */
int pv_layernorm_bwd_sum(const float* x, const uint16_t* dy16, const float* dy32, const float* gamma, float* dx_out, uint16_t* dx16,
                         float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate, void* stream);

/* pv_attention_stream_bwd_bf16 (include/peekvit_hip_attn_stream.h: same inputs, same delta_ws, same two launches) with a 16-BIT result:
 * dqkv16 [B, S, 3 * H * dh] holds that entry point's fp32 value - the q third already times qscale - rounded once.  dbias_partial (optional) fp32
 * [B, ceil(S / 64), 3 * H * dh]: row (b, j) = the column sums of the STORED 16-bit values over rows 64 j .. 64 j + 63 of image b (rows >= S
 * contribute nothing); every element is written exactly once, the q third by the dQ launch and the k | v thirds by the dK | dV launch;
 * pv_colsum_f32 over its B * ceil(S / 64) rows ends the bias gradient.  16-bit arrays 16-byte aligned, fp32 rows 4-byte aligned. */
int pv_attention_stream_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16,
                                   float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_PCT_BLOCK_H */
