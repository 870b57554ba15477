// Training path of the point-cloud stem's pair stage (include/peekvit_hip_pct_train.h): the neighbour lists, the moments of the pair
// features that batch statistics need, the max over the neighbours in front of BatchNorm and ELU, and the backward sums over the query points.
//
// All four kernels give one workgroup the same 64 query points of an image (PV_ARPE_QPB), so G = B * ceil(N / 64) is the grid and the number
// of partial rows.  Nothing is accumulated across workgroups on the GPU: a workgroup adds its threads in a fixed tree and stores one row.
// pv_arpe_knn_kernel is pv_arpe_kernel's (pv_pct.hip) distance and selection part: both call pv_knn.h.
#include "pv_knn.h"
#include "../../include/peekvit_hip_pct_train.h"

// dynamic LDS: the cloud (12 N bytes, rounded up to 16) and, behind it, whatever a kernel needs to add its waves - no static LDS, so the
// dynamic base stays 16-byte aligned
static inline size_t pv_cloud_bytes(int64_t N) { return ((size_t)N * 12 + 15) & ~(size_t)15; }

// The sums that leave a workgroup are formed in fp64 (a product of two fp32 values is exact in it) and rounded to fp32 once, as the partial
// row is stored: a row is then as accurate as its format allows, whatever k is.  A fixed butterfly: every lane ends with the same bits.
__device__ __forceinline__ double pv_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------
// neighbour lists: one wave per query at a time
// ------------------------------------------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(256) void pv_arpe_knn_kernel(const float* __restrict__ points, uint16_t* __restrict__ idx, int N, int k, int bpi) {
    extern __shared__ __attribute__((aligned(16))) float pv_knn_lds[];
    const float* const sx = pv_knn_lds;
    const float* const sy = pv_knn_lds + N;
    const float* const sz = pv_knn_lds + 2 * N;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    pv_knn_stage_cloud(pv_knn_lds, points + (int64_t)b * N * 3, N, threadIdx.x, 256);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int qi = 0; qi < PV_ARPE_QPB / 4; ++qi) {
        const int q = blk * PV_ARPE_QPB + qi * 4 + wave;          // (wave-uniform)
        if (q >= N) break;
        uint32_t key[NI];
        pv_knn_keys<NI>(key, sx, sy, sz, sx[q], sy[q], sz[q], N, lane);
        uint32_t prefix;
        int kr;
        pv_knn_threshold<NI>(key, k, prefix, kr);
        uint16_t* const io = idx + ((int64_t)b * N + q) * k;
        int pos = 0;
        pv_knn_winners<NI>(key, prefix, kr, N, lane, [&](int j, bool sel) { pv_knn_emit(io, j, sel, k, lane, pos); });
    }
}

static int pv_arpe_shape(int64_t B, int64_t N, int64_t k) {
    if (B <= 0 || N <= 0 || k <= 0) return PV_ERR_INVALID_ARG;
    if (N < PV_ARPE_MIN_N || N > PV_ARPE_MAX_N) return PV_ERR_UNSUPPORTED;
    if (k > N) return PV_ERR_INVALID_ARG;
    if (B * ((N + PV_ARPE_QPB - 1) / PV_ARPE_QPB) > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

extern "C" int pv_arpe_knn(const float* points, uint16_t* idx, int64_t B, int64_t N, int64_t k, void* stream) {
    if (!points || !idx) return PV_ERR_INVALID_ARG;
    if (const int e = pv_arpe_shape(B, N, k)) return e;
    if (((uintptr_t)points & 3) || ((uintptr_t)idx & 1)) return PV_ERR_INVALID_ARG;
    const int64_t bpi = (N + PV_ARPE_QPB - 1) / PV_ARPE_QPB;
    const int ni = (int)((N + 63) / 64);
    const dim3 grid((unsigned)(B * bpi));
    const size_t lds = pv_cloud_bytes(N);
#define KNN_LAUNCH(NI_) PV_LAUNCH(pv_arpe_knn_kernel<NI_>, grid, dim3(256), lds, (hipStream_t)stream, points, idx, (int)N, (int)k, (int)bpi)
    if (ni <= 1) { KNN_LAUNCH(1); }
    else if (ni <= 2) { KNN_LAUNCH(2); }
    else if (ni <= 4) { KNN_LAUNCH(4); }
    else if (ni <= 8) { KNN_LAUNCH(8); }
    else if (ni <= 16) { KNN_LAUNCH(16); }
    else if (ni <= 32) { KNN_LAUNCH(32); }
    else { KNN_LAUNCH(64); }
#undef KNN_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// moments of the pair features: thread t takes the pairs t, t + 256, ... of the group's 64 k (consecutive in idx)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_arpe_moments_kernel(const float* __restrict__ points, const uint16_t* __restrict__ idx,
                                                              const float* __restrict__ shift, float* __restrict__ partial, int N, int k, int bpi,
                                                              int red_off) {
    extern __shared__ __attribute__((aligned(16))) float pv_mom_lds[];
    const float* const sx = pv_mom_lds;
    const float* const sy = pv_mom_lds + N;
    const float* const sz = pv_mom_lds + 2 * N;
    double* const red = reinterpret_cast<double*>(pv_mom_lds + red_off);          // [4][28], behind the cloud (16-byte aligned)
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    pv_knn_stage_cloud(pv_mom_lds, points + (int64_t)b * N * 3, N, threadIdx.x, 256);
    __syncthreads();
    const int q0 = blk * PV_ARPE_QPB, nq = min(PV_ARPE_QPB, N - q0), total = nq * k;
    const uint16_t* const ip = idx + ((int64_t)b * N + q0) * k;
    const float cx = shift[0], cy = shift[1], cz = shift[2];
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    for (int p = threadIdx.x; p < total; p += 256) {
        const int q = q0 + p / k, j = min((int)ip[p], N - 1);
        const float f[6] = {sx[q] - cx, sy[q] - cy, sz[q] - cz, sx[q] - sx[j], sy[q] - sy[j], sz[q] - sz[j]};
        int t = 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            acc[i] += (double)f[i];
#pragma unroll
            for (int jj = i; jj < 6; ++jj, ++t) acc[t] = fma((double)f[i], (double)f[jj], acc[t]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 27; ++i) {
        const double s = pv_wave_sum_f64(acc[i]);
        if (lane == 0) red[wave * PV_ARPE_MOMENT_COLS + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < PV_ARPE_MOMENT_COLS) {
        const int c = threadIdx.x;
        const double s = c < 27 ? (red[c] + red[PV_ARPE_MOMENT_COLS + c]) + (red[2 * PV_ARPE_MOMENT_COLS + c] + red[3 * PV_ARPE_MOMENT_COLS + c]) : 0.0;
        partial[(int64_t)blockIdx.x * PV_ARPE_MOMENT_COLS + c] = (float)s;
    }
}

extern "C" int pv_arpe_pair_moments(const float* points, const uint16_t* idx, const float* shift, float* partial, int64_t B, int64_t N, int64_t k,
                                    void* stream) {
    if (!points || !idx || !shift || !partial) return PV_ERR_INVALID_ARG;
    if (const int e = pv_arpe_shape(B, N, k)) return e;
    if ((((uintptr_t)points | (uintptr_t)shift | (uintptr_t)partial) & 3) || ((uintptr_t)idx & 1)) return PV_ERR_INVALID_ARG;
    const int64_t bpi = (N + PV_ARPE_QPB - 1) / PV_ARPE_QPB;
    const size_t cloud = pv_cloud_bytes(N);
    PV_LAUNCH(pv_arpe_moments_kernel, dim3((unsigned)(B * bpi)), dim3(256), cloud + 4 * PV_ARPE_MOMENT_COLS * sizeof(double), (hipStream_t)stream, points,
              idx, shift, partial, (int)N, (int)k, (int)bpi, (int)(cloud / 4));
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// max over the neighbours: four lanes per query, each takes every fourth neighbour; (value, index) pairs meet by two exchanges
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_arpe_pair_max_kernel(const float* __restrict__ points, const uint16_t* __restrict__ idx,
                                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y,
                                                               uint16_t* __restrict__ arg, int N, int k, int bpi) {
    extern __shared__ __attribute__((aligned(16))) float pv_max_lds[];
    const float* const sx = pv_max_lds;
    const float* const sy = pv_max_lds + N;
    const float* const sz = pv_max_lds + 2 * N;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    pv_knn_stage_cloud(pv_max_lds, points + (int64_t)b * N * 3, N, threadIdx.x, 256);
    __syncthreads();
    const int q = blk * PV_ARPE_QPB + (threadIdx.x >> 2), part = threadIdx.x & 3;
    const bool live = q < N;
    const int qc = live ? q : N - 1;
    const float qx = sx[qc], qy = sy[qc], qz = sz[qc];
    float W[6][3], a[6], sg[6], best[6];
    int bj[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        a[c] = b1[c] + w1[c * 6] * qx + w1[c * 6 + 1] * qy + w1[c * 6 + 2] * qz;
        W[c][0] = w1[c * 6 + 3]; W[c][1] = w1[c * 6 + 4]; W[c][2] = w1[c * 6 + 5];
        const float s = scale[c];
        sg[c] = s > 0.f ? 1.f : s < 0.f ? -1.f : 0.f;
        best[c] = -__builtin_inff();
        bj[c] = 0xffff;
    }
    const uint16_t* const ip = idx + ((int64_t)b * N + qc) * k;
    for (int n = part; live && n < k; n += 4) {
        const int j = min((int)ip[n], N - 1);
        const float dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float v = sg[c] * (a[c] + W[c][0] * dx + W[c][1] * dy + W[c][2] * dz);
            if (v > best[c] || (v == best[c] && j < bj[c])) { best[c] = v; bj[c] = j; }
        }
    }
#pragma unroll
    for (int off = 1; off <= 2; off <<= 1) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float v = __shfl_xor(best[c], off, 64);
            const int j = __shfl_xor(bj[c], off, 64);
            if (v > best[c] || (v == best[c] && j < bj[c])) { best[c] = v; bj[c] = j; }
        }
    }
    if (live && part == 0) {
        float* const yo = y + ((int64_t)b * N + q) * 6;
        uint16_t* const ao = arg + ((int64_t)b * N + q) * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            yo[c] = pv_elu(scale[c] * (sg[c] * best[c]) + shift[c]);
            ao[c] = (uint16_t)bj[c];
        }
    }
}

extern "C" int pv_arpe_pair_max(const float* points, const uint16_t* idx, const float* w1, const float* b1, const float* scale, const float* shift,
                                float* y, uint16_t* arg, int64_t B, int64_t N, int64_t k, void* stream) {
    if (!points || !idx || !w1 || !b1 || !scale || !shift || !y || !arg) return PV_ERR_INVALID_ARG;
    if (const int e = pv_arpe_shape(B, N, k)) return e;
    if ((((uintptr_t)points | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)y) & 3) ||
        (((uintptr_t)idx | (uintptr_t)arg) & 1))
        return PV_ERR_INVALID_ARG;
    const int64_t bpi = (N + PV_ARPE_QPB - 1) / PV_ARPE_QPB;
    PV_LAUNCH(pv_arpe_pair_max_kernel, dim3((unsigned)(B * bpi)), dim3(256), pv_cloud_bytes(N), (hipStream_t)stream, points, idx, w1, b1, scale, shift,
              y, arg, (int)N, (int)k, (int)bpi);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// backward sums: one wave per group, one lane per query
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pv_arpe_pair_bwd_kernel(const float* __restrict__ points, const uint16_t* __restrict__ arg,
                                                              const float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, float* __restrict__ partial, int N, int bpi) {
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi, lane = threadIdx.x;
    const int q = blk * PV_ARPE_QPB + lane;
    const float* const pb = points + (int64_t)b * N * 3;
    float v[PV_ARPE_BWD_COLS];
#pragma unroll
    for (int i = 0; i < PV_ARPE_BWD_COLS; ++i) v[i] = 0.f;
    if (q < N) {
        const int64_t row = ((int64_t)b * N + q) * 6;
        const float qx = pb[3 * q], qy = pb[3 * q + 1], qz = pb[3 * q + 2];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float yc = y[row + c];
            const float gp = g[row + c] * (yc > 0.f ? 1.f : yc + 1.f);
            const int j = min((int)arg[row + c], N - 1);
            const float f[6] = {qx, qy, qz, qx - pb[3 * j], qy - pb[3 * j + 1], qz - pb[3 * j + 2]};
            float z = b1[c];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                z = fmaf(w1[c * 6 + i], f[i], z);
                v[12 + 6 * c + i] = gp * f[i];
            }
            v[c] = gp;
            v[6 + c] = gp * z;
        }
    }
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < PV_ARPE_BWD_COLS; ++i) {
        const float s = (float)pv_wave_sum_f64((double)v[i]);
        if (lane == i) out = s;
    }
    if (lane < PV_ARPE_BWD_COLS) partial[(int64_t)blockIdx.x * PV_ARPE_BWD_COLS + lane] = out;
}

extern "C" int pv_arpe_pair_bwd(const float* points, const uint16_t* arg, const float* y, const float* g, const float* w1, const float* b1,
                                float* partial, int64_t B, int64_t N, void* stream) {
    if (!points || !arg || !y || !g || !w1 || !b1 || !partial) return PV_ERR_INVALID_ARG;
    if (const int e = pv_arpe_shape(B, N, 1)) return e;
    if ((((uintptr_t)points | (uintptr_t)y | (uintptr_t)g | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)partial) & 3) || ((uintptr_t)arg & 1))
        return PV_ERR_INVALID_ARG;
    const int64_t bpi = (N + PV_ARPE_QPB - 1) / PV_ARPE_QPB;
    PV_LAUNCH(pv_arpe_pair_bwd_kernel, dim3((unsigned)(B * bpi)), dim3(64), 0, (hipStream_t)stream, points, arg, y, g, w1, b1, partial, (int)N, (int)bpi);
    return pv_check_launch();
}
