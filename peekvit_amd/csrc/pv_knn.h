// Brute-force k nearest neighbours of one query point per wave, the cloud of the image in the LDS as x | y | z planes (12 N bytes): the
// distance and selection part of the ARPE stem.  pv_arpe_kernel (pv_pct.hip, the eval stem in one launch) and pv_arpe_knn_kernel
// (pv_pct_train.hip, the neighbour lists of the training path) CALL these functions, so both choose the same neighbours to the bit.
// A lane keeps the squared distances to the candidates lane, lane + 64, ... in registers (NI = ceil(N / 64) of them, as bit patterns:
// non-negative floats order as unsigned integers).  The k-th smallest is found bit by bit from the top: the number of keys that share the
// prefix found so far and have a 0 in the next bit is a sum of ballot popcounts - scalar work, no cross-lane traffic.  Ties at the threshold
// are taken in index order through a ballot prefix count.
#pragma once
#include "pv_common.h"

#define PV_ARPE_QPB 64          // query points per workgroup (4 waves x 16)

// points fp32 [N, 3] of one image -> planes lds[0:N] = x, lds[N:2N] = y, lds[2N:3N] = z; every thread of the workgroup calls it, the
// caller synchronises
__device__ __forceinline__ void pv_knn_stage_cloud(float* __restrict__ lds, const float* __restrict__ p, int N, int tid, int nthreads) {
    for (int t = tid; t < 3 * N; t += nthreads) {
        const int j = t / 3, c = t - 3 * j;
        lds[c * N + j] = p[t];
    }
}

template <int NI>
__device__ __forceinline__ void pv_knn_keys(uint32_t (&key)[NI], const float* sx, const float* sy, const float* sz, float qx, float qy, float qz,
                                            int N, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma clang fp contract(off)          // (dx*dx + dy*dy) + dz*dz with every operation rounded: what the stock-op k-NN computes
        const int j = lane + 64 * i;
        key[i] = 0xffffffffu;
        if (j < N) {
            const float dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
            key[i] = __builtin_bit_cast(uint32_t, (dx * dx + dy * dy) + dz * dz);
        }
    }
}

// the k-th smallest key, bit by bit from the top; kr = its rank among the keys that share the prefix found so far
template <int NI>
__device__ __forceinline__ void pv_knn_threshold(const uint32_t (&key)[NI], int k, uint32_t& prefix, int& kr) {
    prefix = 0;
    kr = k;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t mask = ~((1u << bit) - 1u);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) cnt += __popcll(__ballot((key[i] & mask) == prefix));
        if (kr > cnt) {
            kr -= cnt;
            prefix |= 1u << bit;
        }
    }
}

// winners: every key below the threshold, and the first kr keys equal to it in index order.  f(j, sel) runs on the whole wave for every
// register of candidates (j = lane + 64 i; sel: candidate j is one of the k winners), so f may use wave-wide operations.
template <int NI, class F>
__device__ __forceinline__ void pv_knn_winners(const uint32_t (&key)[NI], uint32_t prefix, int kr, int N, int lane, F&& f) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int taken = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (64 * i >= N) break;                                 // (wave-uniform)
        const int j = lane + 64 * i;
        const bool in = j < N, eq = in && key[i] == prefix;
        const unsigned long long em = __ballot(eq);
        const bool sel = in && (key[i] < prefix || (eq && taken + __popcll(em & below) < kr));
        taken += __popcll(em);
        f(j, sel);
    }
}

// the winners' indices in ascending order: winner number r of the query goes to out[r] (Out = int32_t or uint16_t); pos is carried
// from one register of candidates to the next
template <class Out>
__device__ __forceinline__ void pv_knn_emit(Out* __restrict__ out, int j, bool sel, int k, int lane, int& pos) {
    const unsigned long long sm = __ballot(sel);
    const int r = pos + __popcll(sm & ((1ull << lane) - 1ull));
    if (sel && r < k) out[r] = (Out)j;
    pos += __popcll(sm);
}
