/* peekvit_hip_pct_train.h - C ABI of the training path of the point-cloud stem's pair stage (ARPE: k-NN -> lin1 -> bn1 -> ELU -> max over the
 * neighbours; points [B, N, 3] -> y [B, N, 6]), forward and backward.
 *
 * Additive to include/peekvit_hip.h and include/peekvit_hip_pct.h (same library, same conventions, ABI v10 unchanged): stateless, never
 * allocates, never synchronises, launches on the caller's stream, validates every argument before touching the GPU (PV_ERR_INVALID_ARG /
 * PV_ERR_UNSUPPORTED).  No entry point uses an atomic: sums over the batch leave the GPU as one partial row per workgroup, which the caller
 * adds in a fixed order, so two runs give identical bits.
 *
 * Notation: pairs p = (b, q, j), j one of the k nearest neighbours of point q of image b (q itself included); f_p = [x_q, x_q - x_j] (6 values);
 * z_p = w1 f_p + b1 (6 channels).  With BatchNorm 1 as y = scale * z + shift (batch or running statistics, the caller's choice),
 *   y[b, q, c] = elu(scale[c] * z*[c] + shift[c]),   z*[c] = the z[c] of the neighbour that maximises sign(scale[c]) * z[c]
 * (ELU is monotone and BatchNorm affine per channel: the maximum over the neighbours moves in front of both).
 *
 *   pv_arpe_knn            the neighbour lists, chosen exactly as pv_arpe_embed chooses them (one shared implementation)
 *   pv_arpe_pair_moments   first and second moments of the pair features f: all that batch statistics of z need, for any w1
 *   pv_arpe_pair_max       y and the winning neighbour of every (query, channel)
 *   pv_arpe_pair_bwd       the three sums over the query points from which every parameter gradient follows
 *
 * Limits of all four: 16 <= N <= 4096 (PV_ERR_UNSUPPORTED outside), 1 <= k <= N, every pointer 4-byte aligned (2-byte for the uint16
 * arrays).  G = B * ceil(N / 64) is the number of partial rows (one per 64 query points of an image). */
#ifndef PEEKVIT_HIP_PCT_TRAIN_H
#define PEEKVIT_HIP_PCT_TRAIN_H

#include "peekvit_hip_pct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Width of a partial row of pv_arpe_pair_moments (6 sums, 21 products, 1 pad) and of pv_arpe_pair_bwd (6 x (A, Z, C[6])). */
#define PV_ARPE_MOMENT_COLS 28
#define PV_ARPE_BWD_COLS 48

/* points fp32 [B, N, 3] -> idx uint16 [B, N, k]: per query point the k points of the same image with the smallest squared distance
 * (dx*dx + dy*dy) + dz*dz, every operation rounded to fp32 on its own, exact ties to the lowest index, the query itself a candidate; in
 * ascending index order.  Equal to pv_arpe_embed's idx_out value for value. */
int pv_arpe_knn(const float* points, uint16_t* idx, int64_t B, int64_t N, int64_t k, void* stream);

/* Moments of f' = [x_q - shift, x_q - x_j] over the pairs of each group of 64 query points.  shift fp32 [3] (any value: it only moves the
 * point about which the sums are taken; the batch mean of the points keeps them small).  partial fp32 [G, 28]:
 *   partial[g, i]      = sum f'[i]                          i = 0..5
 *   partial[g, 6 + t]  = sum f'[i] f'[j]                    t = the position of (i, j), i <= j, in row-major order of the upper triangle
 *   partial[g, 27]     = 0
 * Features are fp32; a thread sums its pairs in index order in fp64 (the products are exact in it), the 256 threads of a group are added in
 * a fixed tree, and the row is rounded to fp32 once. */
int pv_arpe_pair_moments(const float* points, const uint16_t* idx, const float* shift, float* partial, int64_t B, int64_t N, int64_t k, void* stream);

/* y fp32 [B, N, 6] and arg uint16 [B, N, 6] from points, idx (pv_arpe_knn's), w1 fp32 [6, 6], b1 fp32 [6], scale / shift fp32 [6].
 * arg[b, q, c] is the point index of the neighbour whose z[c] is the largest (scale[c] > 0) or the smallest (scale[c] < 0); among equal
 * values, and for scale[c] == 0, the lowest index. */
int pv_arpe_pair_max(const float* points, const uint16_t* idx, const float* w1, const float* b1, const float* scale, const float* shift, float* y,
                     uint16_t* arg, int64_t B, int64_t N, int64_t k, void* stream);

/* Backward sums.  g fp32 [B, N, 6] = dL/dy; g' = g * (1 if y > 0 else y + 1) (ELU's derivative from its output); f* = [x_q, x_q - x_arg],
 * z* = w1 f* + b1 per (query, channel).  partial fp32 [G, 48], per channel c:
 *   partial[g, c]              = A[c]    = sum g'[c]
 *   partial[g, 6 + c]          = Z[c]    = sum g'[c] z*[c]
 *   partial[g, 12 + 6 c + i]   = C[c, i] = sum g'[c] f*[i]
 * over the 64 query points of the group: one lane per query forms its terms in fp32, one fixed tree adds them in fp64, the row is rounded to
 * fp32 once.  arg values must be < N. */
int pv_arpe_pair_bwd(const float* points, const uint16_t* arg, const float* y, const float* g, const float* w1, const float* b1, float* partial,
                     int64_t B, int64_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEEKVIT_HIP_PCT_TRAIN_H */
