/* peekvit_hip_avit_long.h - C ABI of A-ViT's halting step on the PACKED live rows past PV_AVIT_PACK_MAX_S tokens per image:
 * pv_avit_pack_step_train and pv_avit_pack_step_bwd (include/peekvit_hip_avit_pack_train.h, whose packed-row layout, flag bits and arithmetic these
 * entry points share) for 1 <= S <= PV_AVIT_LONG_MAX_S tokens and segments of up to S + 1 rows.  Where the resident kernels give every token of an
 * image one thread of one 256-thread workgroup, these walk the image's tokens and its segment in chunks of 256 and carry the number of surviving rows
 * from chunk to chunk, so the compaction stays stable: live rows in token order, then the one zero representative row.  The per-image tables live in
 * LDS at their long size (forward: token -> row, 16 KiB, and the source row of every written row, 8 KiB; backward: both inverse tables, 32 KiB).
 *
 * Where S <= PV_AVIT_PACK_MAX_S EVERY output has the resident entry point's bits - h_part included: its order is the resident one per chunk of 256
 * tokens (one h per thread, summed over the wave, the four wave sums as (w0 + w1) + (w2 + w3)), the chunk sums added in chunk order, then
 * + n_halted[b] * h of the representative row.  One chunk is the resident order.
 *
 * Additive to include/peekvit_hip.h (same library, same conventions, ABI v10 unchanged): stateless, never allocates, never synchronises, launches on
 * the caller's stream, validates every argument before touching the GPU with the resident entry points' rules and codes (PV_ERR_UNSUPPORTED:
 * S > PV_AVIT_LONG_MAX_S, n_cls > PV_AVIT_PACK_MAX_CLS, D % 4 != 0, D > PV_AVIT_PACK_MAX_D, B * S or a row count beyond 2^31 - 1).  Plain vector
 * stores, no atomics, one owner per output element, every sum in a fixed order: two runs give identical bits.  A segment that does not lie inside
 * [0, R) or is longer than S + 1 rows is skipped, a row that names a token outside [0, S) is ignored: nothing is read or written outside the stated
 * sizes. */
#ifndef PEEKVIT_HIP_AVIT_LONG_H
#define PEEKVIT_HIP_AVIT_LONG_H

#include "peekvit_hip_avit_pack_train.h"

#define PV_AVIT_LONG_MAX_S 4096

#ifdef __cplusplus
extern "C" {
#endif

/* pv_avit_pack_step_train's contract, field for field (state update on the dense [B, S] arrays, class-row accumulation, h_part, the stable compaction
 * into x_next / row_scale_next / log_mult_next / pos_next / seg_next / n_halted_next / totals, the saves sv [3, R], ycls [B, n_cls, D] and
 * src_next [<= R]), for 1 <= S <= PV_AVIT_LONG_MAX_S.  Three launches (one when last != 0), one workgroup per image.
 * sv, ycls and src_next may ALL be null: the inference step, which saves nothing and writes every other output with the same bits.  Any other
 * combination with a null among them is PV_ERR_INVALID_ARG, except src_next alone with last != 0 (as in the resident step). */
int pv_avit_pack_step_long(const float* y, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, int64_t B, int64_t S, int64_t D,
                           int64_t R, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in,
                           float* c_out, float* R_out, float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out,
                           int64_t n_cls, float* h_part, float gate_scale, float gate_center, float threshold, int last, float* x_next,
                           float* row_scale_next, int32_t* seg_next, int32_t* n_halted_next, float* log_mult_next, int32_t* pos_next,
                           int32_t* totals, float* sv, float* ycls, int32_t* src_next, void* stream);

/* pv_avit_pack_step_bwd's contract for the same range: one launch, one workgroup per image (G[b] has one owner), a wave per input row. */
int pv_avit_pack_step_long_bwd(const float* g_next, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, const int32_t* seg_next,
                               const int32_t* src_next, const float* sv, const float* ycls, const float* gR, const float* grho, const float* gacc,
                               const float* gh, float* G, float* dy, uint16_t* dy16, float* dR, int64_t B, int64_t S, int64_t D, int64_t R,
                               int64_t R_next, int64_t n_cls, float gate_scale, int last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_AVIT_LONG_H */
