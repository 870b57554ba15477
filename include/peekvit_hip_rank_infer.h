/* peekvit_hip_rank_infer.h - C ABI of what a SORTING point-cloud encoder block needs at eval on top of include/peekvit_hip_pct.h
 * (peekvit_amd.engine.rank_pct_forward).  Such a block orders rows 1.. by descending norm, keeps the first L = min(S, ceil(S *
 * budget)) rows of the whole sequence and runs a PCTBlock on them.  The block never uses its input after LayerNorm 1 (both residuals are LayerNorm
 * outputs), so the kept rows are read THROUGH the ranking by that LayerNorm and the gathered fp32 rows never exist in memory.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer, k out
 * of range; PV_ERR_UNSUPPORTED: N > 4096, D % 4 != 0, D > 1024, more than 2^31 - 1 workgroups).  No atomics: every output element has one owner, so
 * two runs give identical bits.
 *
 * "16-bit" is the operand type of the library (bf16, or fp16 in the -DPV_OPERAND_F16 build). */
#ifndef PEEKVIT_HIP_RANK_INFER_H
#define PEEKVIT_HIP_RANK_INFER_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pv_rank_topk_gap's contract (include/peekvit_hip.h) by a SORT: O(N log^2 N) work per image instead of O(N^2).  norms fp32 [B, N]; keep int32
 * [B, k] = the first k indices of the stable descending order of every image's norms: ties go to the lowest index first, NaN ranks above +inf.  The
 * order is specified on +0.0, positive finite values, +inf and the canonical positive NaN (what a norm can be).  gap_min fp32 [B], optional (may be
 * null): gap_min[b] = min(gap_min[b], (n_{k-1} - n_k) / n_{k-1}) with n_r the norm of rank r, when k < N; untouched when k == N.
 * 0 <= k <= N <= 4096; k == 0 returns PV_OK without a launch.  One workgroup per image: a bitonic network on 64-bit keys (the norm's sortable
 * bit pattern | the complemented index - unique, so the network's order is the stable one) in the LDS. */
int pv_rank_order_gap(const float* norms, int32_t* keep, float* gap_min, int64_t B, int64_t N, int64_t k, void* stream);

/* pv_layernorm_f32_bf16 (include/peekvit_hip_pct.h: its kernel) with the rows of x fp32 [B, S, D] read through a ranking: output row b (1 + k) is
 * the LayerNorm of x[b, 0], output row b (1 + k) + 1 + j that of x[b, 1 + keep[b, j]] (j < k).  out16 16-bit and out32 fp32, both contiguous
 * [B (1 + k), D] and bit-identical to pv_gather_tokens followed by pv_layernorm_f32_bf16.  keep int32 [B, k] (may be null when k == 0); an index
 * outside [0, S - 2] is clamped to the image.  D % 4 == 0, D <= 1024, 0 <= k <= S - 1; x / gamma / beta / out32 16-byte aligned, out16 8-byte
 * aligned, keep 4-byte aligned.  out32 must not overlap x. */
int pv_layernorm_gather_f32_bf16(const float* x, const int32_t* keep, const float* gamma, const float* beta, uint16_t* out16, float* out32,
                                 int64_t B, int64_t S, int64_t k, int64_t D, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_RANK_INFER_H */
