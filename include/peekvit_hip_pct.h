/* peekvit_hip_pct.h - C ABI of the point-cloud transformer forward (reference models/pct.py, PointCloudTransformer).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises,
 * launches on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG / PV_ERR_UNSUPPORTED).
 *
 * The encoder of the reference is a pre-LN transformer whose blocks add their residuals to the LayerNorm OUTPUT (models/pct.py:49-51); it
 * runs on pv_gemm_bf16 / pv_attention_bf16 of peekvit_hip.h.  What this header adds:
 *
 *   pv_arpe_embed          the stem (models/pct.py:78-90 at eval) in one launch: brute-force k nearest neighbours of every point, the
 *                          6 -> 6 linear on [x, x - neighbour], BatchNorm, ELU, the max over the neighbours, the 6 -> D linear, BatchNorm, ELU.
 *                          Nothing but the [B, N, D] tokens reaches memory.
 *   pv_layernorm_f32_bf16  pv_layernorm_bf16 that also writes the fp32 LayerNorm rows (the residual a PCT block adds).
 *   pv_mean_pool_f32       pooled[b, :] = mean over the S rows of x[b] (models/pct.py:232).
 *   pv_pct_head_f32        logits = lin2(gelu(bn1(lin1(pooled)))) (models/pct.py:139-143 at eval) in fp32.
 */
#ifndef PEEKVIT_HIP_PCT_H
#define PEEKVIT_HIP_PCT_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Points per cloud pv_arpe_embed takes (the cloud of one image stays in the LDS: 12 bytes a point). */
#define PV_ARPE_MIN_N 16
#define PV_ARPE_MAX_N 4096
/* Largest embedding width of pv_arpe_embed. */
#define PV_ARPE_MAX_D 1024
/* Largest input / hidden width of pv_pct_head_f32. */
#define PV_PCT_HEAD_MAX_D 4096

/* The ARPE stem.  points fp32 [B, N, 3]; w1 fp32 [6, 6], b1 fp32 [6]: ARPE.lin1; bn1_scale / bn1_shift fp32 [6]: BatchNorm 1 at eval as
 * y = scale * z + shift (scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale); w2 fp32 [D, 6], b2 fp32 [D]:
 * ARPE.lin2; bn2_scale / bn2_shift fp32 [D].
 * Per query point q of an image: the k points of the SAME image with the smallest squared distance (dx*dx + dy*dy) + dz*dz, every
 * operation rounded to fp32 on its own; exact ties go to the lowest index (as pv_rank_topk breaks ties); q itself is a candidate.  Then
 *   z[j, c] = b1[c] + w1[c, 0:3] . x_q + w1[c, 3:6] . (x_q - x_j)              for the k winners j
 *   h[c]    = elu(scale1[c] * (max_j z[j, c] if scale1[c] >= 0 else min_j z[j, c]) + shift1[c])     (= max_j elu(bn1(z[j, c])): both monotone)
 *   tokens[b, row_off + q, d] = elu(scale2[d] * (b2[d] + w2[d, :] . h) + shift2[d])
 * tokens fp32 [B, S, D]: only the rows [row_off, row_off + N) of every image are written (registers may sit in front).
 * idx_out int32 [B, N, k], optional (may be null): the winners of every query in ascending index order.
 * The k-th smallest distance is found by a radix select on the bit patterns, ties in index order by a prefix count: no result depends on the
 * order of concurrent work, two runs give identical bits.
 * Limits: 16 <= N <= 4096 and D % 4 == 0, D <= 1024 (PV_ERR_UNSUPPORTED outside); 1 <= k <= N, row_off >= 0, row_off + N <= S; tokens, w2,
 * b2, bn2_scale, bn2_shift 16-byte aligned. */
int pv_arpe_embed(const float* points, const float* w1, const float* b1, const float* bn1_scale, const float* bn1_shift, const float* w2,
                  const float* b2, const float* bn2_scale, const float* bn2_shift, float* tokens, int32_t* idx_out, int64_t B, int64_t N, int64_t k,
                  int64_t D, int64_t S, int64_t row_off, void* stream);

/* LayerNorm with both outputs.  x fp32 [rows, ldx]; out16 16-bit [rows, D]: bit-identical to pv_layernorm_bf16's (row_scale null); out32 fp32
 * [rows, ld32]: the same values before the rounding to 16 bits.  D % 4 == 0, D <= 4096, ldx % 4 == 0, ld32 % 4 == 0, x / out32 / gamma / beta
 * 16-byte aligned, out16 8-byte aligned.  out32 must not overlap x. */
int pv_layernorm_f32_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta, uint16_t* out16, float* out32, int64_t ld32,
                          int64_t rows, int64_t D, float eps, void* stream);

/* pooled[b, d] = (sum over s of x[b, s, d]) / S.  x fp32 [B, S, D] contiguous, pooled fp32 [B, D].  Each of 16 row groups sums its rows
 * (s = g, g + 16, ...) with a compensated (Kahan) sum, the 16 partial sums are added in a fixed tree: deterministic, and accurate to an ulp
 * or two at any S.  D % 4 == 0, x and pooled 16-byte aligned. */
int pv_mean_pool_f32(const float* x, float* pooled, int64_t B, int64_t S, int64_t D, void* stream);

/* The classification head of the point-cloud models at eval: hidden[b, j] = gelu_erf(bn_scale[j] * (b1[j] + w1[j, :] . pooled[b, :]) +
 * bn_shift[j]), logits[b, c] = b2[c] + w2[c, :] . hidden[b, :].  pooled fp32 [B, D]; w1 fp32 [Hd, D]; b1, bn_scale, bn_shift fp32 [Hd]; w2 fp32
 * [C, Hd]; b2 fp32 [C] (b1 and b2 may be null); logits fp32 [B, C].  One wave per dot product (lanes stride the columns, one wave sum): the
 * result does not depend on B.  D <= 4096, Hd <= 4096. */
int pv_pct_head_f32(const float* pooled, const float* w1, const float* b1, const float* bn_scale, const float* bn_shift, const float* w2,
                    const float* b2, float* logits, int64_t B, int64_t D, int64_t Hd, int64_t C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_PCT_H */
