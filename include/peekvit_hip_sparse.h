/* peekvit_hip_sparse.h - C ABI of ResidualViT's exact token compaction (reference models/residualvit.py).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises,
 * launches on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG / PV_ERR_UNSUPPORTED).
 *
 * The reference multiplies a gated-off token by zero and keeps it in the sequence.  Every token whose mask is 0 in a block leaves that block
 * with the same value (fc2(gelu(b1)) + b2), and identical rows stay identical in every later block, so the tokens of one image that were
 * masked in the same block travel as ONE packed row with a multiplicity n: as a key it counts n times (+ ln n on its score), as a query and
 * in the row-wise layers it is computed once.  Such a class row may come live again in a later block (its shared value can get a mask above
 * 0), so every packed row carries its own multiplicity.
 *
 *   pv_attention_varlen_w_bf16   ragged attention over packed row segments with a per-key log-multiplicity
 *   pv_residual_pack_step        the gate of one block on the packed rows + the next packed input and its tables
 */
#ifndef PEEKVIT_HIP_SPARSE_H
#define PEEKVIT_HIP_SPARSE_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest row segment (tokens of one image incl. class and budget row) the two entry points take. */
#define PV_SPARSE_MAX_LEN 208

/* pv_attention_varlen_bf16 with a weight per key.  qkv 16-bit [R, 3*H*dh] packed rows (q pre-scaled), out 16-bit [R, H*dh]; image b is the
 * row segment [seg_start[b], seg_start[b+1]); log_mult fp32 [R]: key r's score gets + log_mult[r] before the row maximum is taken (0 for an
 * ordinary row, ln n for a row that stands for n identical tokens), which is dense softmax attention with that key repeated n times.
 * Limits as pv_attention_varlen_bf16: dh = 64, max_len (>= the longest segment) <= PV_SPARSE_MAX_LEN; outside them nothing is launched and
 * PV_ERR_UNSUPPORTED is returned.  range_flag: the score guard of pv_attention_bf16 (fp16 build; may be null). */
int pv_attention_varlen_w_bf16(const uint16_t* qkv, uint16_t* out, const int32_t* seg_start, const float* log_mult, int64_t B,
                               int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream);

/* One gate + compaction step (three launches: per image gate, a one-workgroup scan of the next segment lengths, per image compaction).
 * Inputs
 *   x        fp32 [R, D]       packed residual stream; image b = rows [seg_start[b], seg_start[b+1]), class row first, budget row last,
 *                              2 <= length <= N + 2 <= PV_SPARSE_MAX_LEN
 *   mult     int32 [R]         tokens each row stands for (1 on class and budget rows)
 *   tok_row  int32 [B, N]      image token t -> its row, relative to the segment start
 *   wg [D], bg [1], wb [D], bb [1], temp, sigmoid_bias: the gate, arithmetic of pv_residual_gate in fp32:
 *       thr[b] = sigmoid(wb . budget_row + bb),  mask(row) = max(sigmoid((wg . row + bg) / temp + sigmoid_bias) - thr[b], 0)
 *   mask_row fp32 [R]          scratch (the masks of the input rows; class and budget rows 1)
 * Outputs (every *_next buffer holds R rows; R' <= R rows are written)
 *   x_next          fp32 [R', D]   per image: class row | live rows (mask > 0) as mask * x, in order | one zero row if any row had mask 0 | budget row
 *   row_scale_next  fp32 [R']      1 | mask ... | 0 | 1
 *   mult_next       int32 [R']     multiplicities; the zero row's is the sum over the rows it merges
 *   log_mult_next   fp32 [R']      logf(mult_next)
 *   seg_next        int32 [B + 1]
 *   tok_row_next    int32 [B, N]
 *   mask_out        fp32 [B, N]    the dense mask: mask_row[tok_row]
 *   thr_out         fp32 [B]
 *   totals          int32 [2]      (R', longest next segment)
 *   ln_out          16-bit [R', D] optional (null: skipped): row_scale_next * LayerNorm(x_next row; ln_gamma, ln_beta, ln_eps), from registers
 * Deterministic: no result depends on the order of concurrent work.
 * Limits: D % 4 == 0, D <= 4096, N + 2 <= PV_SPARSE_MAX_LEN, x / x_next / wg / wb / ln_gamma / ln_beta 16-byte aligned, ln_out 8-byte. */
int pv_residual_pack_step(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                          const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                          float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                          int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta,
                          float ln_eps, uint16_t* ln_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_SPARSE_H */
