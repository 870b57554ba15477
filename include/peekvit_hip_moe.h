/* peekvit_hip_moe.h - C ABI of the routed top-1 mixture-of-experts forward (reference models/moevit.py, VisionTransformerMoE).
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises,
 * launches on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG / PV_ERR_UNSUPPORTED).
 *
 * At inference the reference's gate is one_hot(argmax(Linear(LN(x)))) (models/blocks.py:19-25) and its MoE output is the selected expert's
 * output (models/moevit.py:49-61, 84-96), but it runs EVERY expert on EVERY token.  Here each token row runs through its own expert only:
 *
 *   pv_moe_route          LayerNorm + fp32 gate + argmax per row, then a deterministic counting sort of the rows by expert into
 *                         "packed" order: expert e owns the packed rows [seg[e], seg[e+1]), its count rounded up to PV_MOE_TILE_ROWS so that
 *                         no GEMM tile spans two experts.  perm maps a packed row to its source row (-1 on pad rows).
 *   pv_gemm_grouped_bf16  the 256 x 256 GEMM tile of pv_gemm_bf16 over the packed rows, each M-tile with its expert's weight slice.
 *   pv_moe_gather_bf16    packed rows taken from per-expert planes (the attention MoE: every expert attends over all rows, the routed
 *                         row keeps its own expert's result).
 */
#ifndef PEEKVIT_HIP_MOE_H
#define PEEKVIT_HIP_MOE_H

#include "peekvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Packed rows per expert segment are a multiple of this (the M extent of the GEMM tile pv_gemm_grouped_bf16 runs). */
#define PV_MOE_TILE_ROWS 256
/* Largest expert count the routing kernels take. */
#define PV_MOE_MAX_EXPERTS 64

/* Worst-case packed row count for M rows and E experts: (ceil(M / 256) + E) * 256.  Every packed buffer (perm, the 16-bit rows, the
 * grouped GEMM's A and 16-bit output) is sized for it, so the host never needs the actual segment sizes.  Negative on bad arguments. */
int64_t pv_moe_packed_rows(int64_t M, int64_t E);

/* Scratch bytes pv_moe_route needs for M rows and E experts.  Negative on bad arguments. */
int64_t pv_moe_route_scratch_size(int64_t M, int64_t E);

/* Routing of one MoE layer.  x fp32 [M rows, ldx] (ldx % 4 == 0, 16-byte aligned); ln_gamma / ln_beta fp32 [D]; gate_w fp32 [E, D],
 * gate_b fp32 [E]: the TopKGate's nn.Linear (models/moevit.py:23-33).  Per row: y = LayerNorm(x) (the arithmetic of pv_layernorm_bf16),
 * logits = gate_w . y + gate_b in fp32, expert = argmax (the LOWEST index among equal maxima, as torch.argmax).
 * Outputs:
 *   expert      int32 [M]
 *   gap         fp32 [M], optional: top-1 minus top-2 logit (+inf when E == 1)
 *   probs       fp32 [M, E], optional: one_hot(expert)
 *   seg         int32 [E + 1]: padded segment offsets, seg[0] = 0, seg[e+1] - seg[e] = count_e rounded up to PV_MOE_TILE_ROWS
 *   perm        int32 [pv_moe_packed_rows(M, E)]: packed row -> source row, ascending within a segment; -1 on every other row
 *   tile_expert int32 [pv_moe_packed_rows(M, E) / PV_MOE_TILE_ROWS]: the expert of each 256-row tile, -1 for a tile past seg[E]
 *   xln         16-bit [pv_moe_packed_rows(M, E), D], optional: y of the source row perm[p] in row p (bit-identical to pv_layernorm_bf16's
 *               row), zeros on pad rows
 * The sort is a per-block histogram, an exclusive scan and a stable scatter: no result depends on the order of concurrent work, two runs
 * give identical bits.  Limits: 1 <= E <= 64, D % 4 == 0, D <= 4096, M < 2^31 - 2^24.  scratch: pv_moe_route_scratch_size(M, E) bytes,
 * 16-byte aligned, scratch_bytes its size. */
int pv_moe_route(const float* x, int64_t ldx, int64_t M, int64_t D, const float* ln_gamma, const float* ln_beta, float ln_eps,
                 const float* gate_w, const float* gate_b, int64_t E, int32_t* expert, float* gap, float* probs, int32_t* seg, int32_t* perm,
                 int32_t* tile_expert, uint16_t* xln, void* scratch, int64_t scratch_bytes, void* stream);

/* Grouped GEMM over packed rows: tile row t (rows [256 t, 256 t + 256) of A) with e = tile_expert[t] >= 0 computes
 *   epilogue(A[rows] . W_e^T + bias_e),  W_e = W + e * w_stride (16-bit [N, K], row stride ldw), bias_e = bias + e * N (fp32 [E, N]);
 * a tile with e < 0 exits without reading or writing anything.  args->M = tiles_m * 256 (the worst-case grid: pv_moe_packed_rows),
 * args->A / lda the packed 16-bit rows.  Epilogues:
 *   PV_EPI_BIAS_GELU_BF16  out[p] = 16-bit gelu(.) in packed order (row stride ldo);
 *   PV_EPI_BIAS_RES_F32    out[perm[p]] = res[perm[p]] + . for every packed row with 0 <= perm[p] < out_rows (fp32, row strides ldo / ldr);
 *                          pad rows write nothing.  perm int32 [args->M]; out and res hold out_rows rows.
 * The arithmetic of a tile is pv_gemm_bf16's 256 x 256 tile (bias-initialised accumulators, same K order, same epilogue): a row's result is
 * bit-identical to pv_gemm_bf16 on that expert's rows when pv_gemm_bf16 runs the 256-row tile.  range_flag as pv_gemm_bf16 (the fp16 build
 * ORs 1 for a 16-bit output out of range).  Limits: K % 128 == 0, N % 8 == 0, 1 <= E <= 64, tile_expert int32 [tiles_m].  Everything else
 * in args must be unset (no row_scale, LayerNorm fusion or folding, split-K, qcols). */
int pv_gemm_grouped_bf16(const pv_gemm_args* args /* HOST pointer */, const int32_t* tile_expert, int64_t tiles_m, int64_t E, int64_t w_stride,
                         const int32_t* perm, int64_t out_rows, void* stream);

/* Packed rows from per-expert planes: out[p] = src[expert[perm[p]] * plane_stride + perm[p] * ld, 0 .. D) for perm[p] >= 0, zeros where
 * perm[p] < 0.  src 16-bit [E planes][M rows][ld], out 16-bit [M_pad, D].  D % 8 == 0, ld % 8 == 0, 16-byte aligned. */
int pv_moe_gather_bf16(const uint16_t* src, int64_t plane_stride, int64_t ld, const int32_t* expert, const int32_t* perm, int64_t M,
                       int64_t M_pad, int64_t D, int64_t E, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_MOE_H */
