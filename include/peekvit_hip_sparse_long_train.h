/* peekvit_hip_sparse_long_train.h - C ABI of ResidualViT TRAINING on its packed live rows past PV_SPARSE_MAX_LEN rows per image (DESIGN.md
 * section 35): the four entry points of include/peekvit_hip_sparse_train.h for the row range of include/peekvit_hip_sparse_long.h.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG: a null pointer, a size < 1, a misaligned pointer;
 * PV_ERR_UNSUPPORTED: dh != 64, a segment bound above PV_SPARSE_LONG_MAX_LEN, D % 4 != 0, D > 4096, more than 2^31 - 1 workgroups; nothing is
 * launched in either case).  No floating-point atomics: every sum has one owner and a fixed order, so two runs give identical bits.
 *
 * The entry points of peekvit_hip_sparse_train.h keep their limit of PV_SPARSE_MAX_LEN rows and every bit of their results; at a bound within that
 * limit the entry points below give the same results (bit for bit where stated).  Conventions - the operand type, the segment tables, a packed row
 * that stands for n tokens carrying the total gradient of its members - are that header's.
 *
 *   pv_attention_varlen_w_stream_lse_bf16     pv_attention_varlen_w_stream_bf16 that also writes the rows' statistics
 *   pv_attention_varlen_w_stream_bwd16_bf16   pv_attention_varlen_w_bwd16_bf16 for max_len <= PV_SPARSE_LONG_MAX_LEN
 *   pv_residual_pack_step_long_train          pv_residual_pack_step_long with the two tables its backward reads
 *   pv_residual_pack_step_long_bwd            pv_residual_pack_step_bwd for N + 2 <= PV_SPARSE_LONG_MAX_LEN
 */
#ifndef PEEKVIT_HIP_SPARSE_LONG_TRAIN_H
#define PEEKVIT_HIP_SPARSE_LONG_TRAIN_H

#include "peekvit_hip_sparse_train.h"
#include "peekvit_hip_sparse_long.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pv_attention_varlen_w_stream_bf16 (its kernel body, arguments, grid and limits; `out` bit for bit) that also writes lse fp32 [R, H],
 * lse[r, h] = log2 sum_k exp(score[r, k] + log_mult[k]) over the keys of r's segment: pv_attention_varlen_w_lse_bf16's definition, so either
 * forward can feed either backward (the two sum in different orders: the values agree to rounding, not bit for bit).  Rows of out / lse behind
 * the last segment, and segments longer than max_len, are not touched.  qkv 16-byte, out 8-byte, lse, log_mult, seg_start 4-byte aligned. */
int pv_attention_varlen_w_stream_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg_start, const float* log_mult, int64_t B,
                                          int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream);

/* pv_attention_varlen_w_bwd16_bf16 - its argument list, outputs, two launches and arithmetic - for max_len <= PV_SPARSE_LONG_MAX_LEN.  Both
 * launches already stream the dimension they sum over; what differs is that the dQ launch looks at EVERY key of a segment when it decides whether
 * the segment carries a weight (and so whether delta is sum_k p dP in fp32 or sum_d dO O).  dbias_partial is [B * ceil(max_len / 64), 3 H dh],
 * every row written.  At max_len <= PV_SPARSE_MAX_LEN every output has pv_attention_varlen_w_bwd16_bf16's bits. */
int pv_attention_varlen_w_stream_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, const int32_t* seg_start,
                                            const float* log_mult, uint16_t* dqkv16, float* dbias_partial, float* delta_ws, int64_t B, int64_t max_len,
                                            int64_t H, int64_t dh, float qscale, void* stream);

/* pv_residual_pack_step_long (its three launches, arguments, results and limits, bit for bit) with gate_arg fp32 [R] and src_next int32 [R'] as
 * pv_residual_pack_step_train defines them.  At N + 2 <= PV_SPARSE_MAX_LEN every result has pv_residual_pack_step_train's bits. */
int pv_residual_pack_step_long_train(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                                     const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                                     float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                                     int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma,
                                     const float* ln_beta, float ln_eps, uint16_t* ln_out, float* gate_arg, int32_t* src_next, void* stream);

/* pv_residual_pack_step_bwd - its argument list, outputs and arithmetic - for N + 2 <= PV_SPARSE_LONG_MAX_LEN.  One launch, one workgroup per image;
 * the image's inverse table (16-bit) and the per-row sums of dmask live in LDS.  The sum of dmask over a row's tokens is taken in token order by one
 * owner: a row that stands for one token gets that token's value, a live row that stands for several is walked by one wave.  The row loop and every
 * sum keep pv_residual_pack_step_bwd's order: at N + 2 <= PV_SPARSE_MAX_LEN every output has its bits. */
int pv_residual_pack_step_long_bwd(const float* x, const int32_t* seg_start, const int32_t* tok_row, const float* mask_row, const float* gate_arg,
                                   const float* thr, const int32_t* seg_next, const int32_t* src_next, const float* g_next, const float* drow_scale,
                                   const float* dmask, int64_t B, int64_t N, int64_t D, const float* wg, const float* wb, float temp, float* dx,
                                   float* dm_row, float* dwg_part, float* dwb_part, float* scal_part, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_SPARSE_LONG_TRAIN_H */
