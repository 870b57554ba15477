// Token ranking by a sort (include/peekvit_hip_rank_infer.h): pv_rank_topk_gap's contract (pv_rowops.hip counts every rank
// against every other key, O(N^2) per image) in O(N log^2 N).
//
// One workgroup of 256 threads per image, the keys of the image in the LDS.  A key is 64 bits: the norm's sortable bit pattern (larger float <=>
// larger integer, NaN above +inf) in the high word, the COMPLEMENTED index in the low word - unique, so any sorting network leaves the stable
// descending order (ties: the lowest index has the largest low word and comes first).  The network is bitonic on P = 256 E >= N keys (E = 1, 2, 4, 8,
// 16), pad keys 0 below every real key (a real key's high word has its top bit set).  Thread t owns the E neighbouring keys t E .. t E + E - 1: the
// exchange distances j < E of a stage run in its registers without a barrier (42 of the 78 steps at P = 4096), the distances j >= E in the LDS, one
// comparator per thread and pass, neighbouring threads on neighbouring keys.  A slot of padding behind every 16 keys keeps the owners' strided reads
// of their E keys off a common bank (E = 16: a stride of 17 slots of 8 bytes).  The rank of a key is its position: no atomics, no second pass.
//
// pv_sort_key / pv_unsort_key / pv_rank_gap are RESTATED from pv_rowops.hip (three small device functions, bit for bit): moving them to a shared
// header would touch every object that includes it, and the entry points here promise the same bits as pv_rank_topk_gap on the same norms
// (tests/test_hip_rank_infer.py compares the two).
#include "pv_common.h"
#include "../../include/peekvit_hip_rank_infer.h"

#define PV_RANK_ORDER_MAX_N 4096
#define PV_RO_SLOT(i) ((i) + ((i) >> 4))

// sortable key: larger float (NaN above +inf, like torch's descending argsort) <=> larger uint32
__device__ __forceinline__ uint32_t pv_sort_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pv_unsort_key(uint32_t u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
// gap_min[b] = min(gap_min[b], (n_{k-1} - n_k) / n_{k-1}) from the keys of rank k - 1 and rank k (pv_rowops.hip: one workgroup per image, no race)
__device__ __forceinline__ void pv_rank_gap(const uint32_t* edge, float* __restrict__ gap_min, int64_t b, int N, int k) {
    if (gap_min && threadIdx.x == 0 && k < N) {
        const float hi = pv_unsort_key(edge[0]), lo = pv_unsort_key(edge[1]);
        const float gap = hi > 0.f ? (hi - lo) / hi : 0.f;
        if (gap < gap_min[b]) gap_min[b] = gap;
    }
}

// one comparator: a sits at the lower position; desc puts the larger key there
__device__ __forceinline__ void pv_ro_exchange(uint64_t& a, uint64_t& b, bool desc) {
    const bool swap = desc ? (a < b) : (a > b);
    const uint64_t x = swap ? b : a, y = swap ? a : b;
    a = x;
    b = y;
}

template <int E>
__global__ __launch_bounds__(256) void pv_rank_order_kernel(const float* __restrict__ norms, int32_t* __restrict__ keep, float* __restrict__ gap_min, int N, int k) {
    constexpr int P = 256 * E;
    __shared__ uint64_t keys[P + P / 16];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = t; i < P; i += 256)
        keys[PV_RO_SLOT(i)] = i < N ? ((uint64_t)pv_sort_key(norms[b * N + i]) << 32) | (uint32_t)~(uint32_t)i : 0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {          // a stage merges runs of kk / 2 keys; a run whose position has bit kk clear descends
        int j = kk >> 1;
        for (; j >= (E > 1 ? E : 1); j >>= 1) {    // distances the owners cannot serve: one comparator per thread and pass, in the LDS
            for (int c = t; c < P / 2; c += 256) {
                const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l = i + j;
                uint64_t lo = keys[PV_RO_SLOT(i)], hi = keys[PV_RO_SLOT(l)];
                pv_ro_exchange(lo, hi, (i & kk) == 0);
                keys[PV_RO_SLOT(i)] = lo;
                keys[PV_RO_SLOT(l)] = hi;
            }
            __syncthreads();
        }
        if constexpr (E > 1) {                     // the remaining distances j, j / 2, ..., 1 (j < E) stay inside one owner's keys
            const int base = t * E;
            uint64_t v[E];
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = keys[PV_RO_SLOT(base + e)];
#pragma unroll
            for (int jj = E / 2; jj >= 1; jj >>= 1) {
                if (jj <= j) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if ((e & jj) == 0) pv_ro_exchange(v[e], v[e | jj], ((base + e) & kk) == 0);
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) keys[PV_RO_SLOT(base + e)] = v[e];
            __syncthreads();
        }
    }
    for (int r = t; r < k; r += 256) keep[b * k + r] = (int32_t)~(uint32_t)keys[PV_RO_SLOT(r)];
    if (gap_min && t == 0 && k < N) {
        const uint32_t edge[2] = {(uint32_t)(keys[PV_RO_SLOT(k - 1)] >> 32), (uint32_t)(keys[PV_RO_SLOT(k)] >> 32)};
        pv_rank_gap(edge, gap_min, b, N, k);
    }
}

extern "C" int pv_rank_order_gap(const float* norms, int32_t* keep, float* gap_min, int64_t B, int64_t N, int64_t k, void* stream) {
    if (!norms || !keep || B <= 0 || N <= 0 || k < 0 || k > N) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)norms | (uintptr_t)keep | (uintptr_t)gap_min) & 3) return PV_ERR_INVALID_ARG;
    if (N > PV_RANK_ORDER_MAX_N || B > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (k == 0) return PV_OK;
#define RO_LAUNCH(E_) PV_LAUNCH(pv_rank_order_kernel<E_>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, norms, keep, gap_min, (int)N, (int)k)
    if (N <= 256) { RO_LAUNCH(1); }
    else if (N <= 512) { RO_LAUNCH(2); }
    else if (N <= 1024) { RO_LAUNCH(4); }
    else if (N <= 2048) { RO_LAUNCH(8); }
    else { RO_LAUNCH(16); }
#undef RO_LAUNCH
    return pv_check_launch();
}
