/* peekvit_hip_sparse_long.h - C ABI of ResidualViT's exact token compaction past PV_SPARSE_MAX_LEN rows per image.
 *
 * Additive to include/peekvit_hip.h and include/peekvit_hip_sparse.h (same library, same conventions, ABI v10 unchanged): stateless, never
 * allocates, never synchronises, launches on the caller's stream, validates every argument before touching the GPU.  Inference only.
 *
 * The two entry points of peekvit_hip_sparse.h keep a whole row segment resident (the attention in LDS, the pack step one thread per row) and
 * stop at 208 rows.  These two take the row range the training engine admits: the attention streams its keys, the pack step walks a segment in
 * chunks.
 *
 *   pv_attention_varlen_w_stream_bf16   pv_attention_varlen_w_bf16 for segments of any length: 64-key blocks, online softmax
 *   pv_residual_pack_step_long          pv_residual_pack_step for N + 2 <= PV_SPARSE_LONG_MAX_LEN
 */
#ifndef PEEKVIT_HIP_SPARSE_LONG_H
#define PEEKVIT_HIP_SPARSE_LONG_H

#include "peekvit_hip_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest row segment (tokens of one image incl. class and budget row) the two entry points take. */
#define PV_SPARSE_LONG_MAX_LEN 4096

/* pv_attention_varlen_w_bf16's contract (qkv 16-bit [R, 3*H*dh] packed rows with q pre-scaled, out 16-bit [R, H*dh], image b = the row segment
 * [seg_start[b], seg_start[b+1]), log_mult fp32 [R] added to key r's score in fp32 before the running maximum is taken) for segments of
 * 1 .. max_len <= PV_SPARSE_LONG_MAX_LEN rows, dh = 64.  One workgroup = 64 queries of one (segment, head); the segment's keys pass through LDS
 * in blocks of 64 with an online softmax (the arithmetic of the streaming forward, include/peekvit_hip_attn_stream.h: with equal segments and
 * log_mult = 0 `out` has its bits).  The grid is B * H * ceil(max_len / 64) workgroups; one whose first query lies past its segment returns at
 * once, and a segment longer than max_len is not touched.  No atomics: the same bits run to run.
 * range_flag: the score guard of pv_attention_bf16 on the scores without log_mult (fp16 build; may be null).
 * PV_ERR_INVALID_ARG: a null qkv / out / seg_start / log_mult, B, H or max_len < 1, qkv not 16-byte, out not 8-byte, seg_start or log_mult not
 * 4-byte aligned.  PV_ERR_UNSUPPORTED: dh != 64, max_len > PV_SPARSE_LONG_MAX_LEN, a grid above 2^31 - 1.  Nothing is launched in either case. */
int pv_attention_varlen_w_stream_bf16(const uint16_t* qkv, uint16_t* out, const int32_t* seg_start, const float* log_mult, int64_t B,
                                      int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream);

/* pv_residual_pack_step (include/peekvit_hip_sparse.h: the same arguments, outputs, three launches and limits, field for field) for
 * 2 <= segment length <= N + 2 <= PV_SPARSE_LONG_MAX_LEN.  The per-image workgroup walks its segment in chunks of 256 rows and carries the number
 * of kept rows from chunk to chunk: the compaction is stable (class row | live rows in order | one zero row | budget row).  The segment's tables
 * are held in LDS (no scratch beyond mask_row).  The row arithmetic is pv_residual_pack_step's: at N + 2 <= PV_SPARSE_MAX_LEN every output has
 * its bits.  Deterministic. */
int pv_residual_pack_step_long(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                               const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                               float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                               int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta,
                               float ln_eps, uint16_t* ln_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_SPARSE_LONG_H */
