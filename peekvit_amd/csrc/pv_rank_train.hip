// Row movers of a sorting point-cloud block in train mode (include/peekvit_hip_rank_train.h): the dense rows [B, S, D] <-> the
// compact rows [B, Sc, D] = row 0, the k kept rows in rank order and - when rows are masked - ONE tail row that stands for all of them.
//
//   pack          x, keep -> xc     gather, the tail row zero                 expand   yc -> y    the tail row into every row L .. S - 1
//   unpack_grad   dxc, keep -> dx   scatter, zeros elsewhere (tail dropped)   reduce   g -> gc    copy, the tail row = the sum of rows L .. S - 1
//
// One wave per row with pv_rows.h's row registers, loads and stores (16-byte accesses, grid-stride over rows).  The tail sum has one owner per element
// and a fixed order: a workgroup owns 16 float4 columns of one image, its 16 row groups walk the rows L + rg, L + rg + 16, ... in order, and thread
// group 0 adds the 16 partials in order - no atomics, two runs give identical bits.  Indices read from keep are clamped to the image's rows.
#include "pv_rows.h"
#include "../../include/peekvit_hip_rank_train.h"

#define PV_RANK_MAX_N 4096          // rows 1.. of an image (pv_rank_topk's limit; the inverse map of unpack_grad lives in the LDS)

template <int NCH>
__global__ __launch_bounds__(256) void pv_rank_pack_kernel(const float* __restrict__ x, const int32_t* __restrict__ keep, float* __restrict__ xc, int64_t B, int S,
                                                           int k, int Sc, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t rows = B * Sc;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t b = r / Sc;
        const int j = (int)(r - b * Sc);
        RowRegs<NCH> v;
        if (j <= k) {
            int src = 0;
            if (j > 0) {
                src = keep[b * k + (j - 1)];
                src = 1 + (src < 0 ? 0 : (src > S - 2 ? S - 2 : src));
            }
            pv_load_row<NCH>(v, x + (b * S + src) * (int64_t)D, nvec, lane);
        } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c) v.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        pv_store_row<NCH>(xc + r * (int64_t)D, v, nvec, lane);
    }
}

// y row r <- yc row min(r, L) (EXPAND), or gc row r <- g row r for r < L (the copied rows of reduce: Sd = L + 1 destination rows, the last one skipped)
template <int NCH, bool EXPAND>
__global__ __launch_bounds__(256) void pv_rank_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t B, int S, int L, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int Sd = EXPAND ? S : L, Ss = EXPAND ? L + 1 : S;          // rows per image walked here / rows per image of the source
    const int64_t rows = B * Sd;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t b = r / Sd;
        const int j = (int)(r - b * Sd);
        RowRegs<NCH> v;
        pv_load_row<NCH>(v, src + (b * Ss + (j < L ? j : L)) * (int64_t)D, nvec, lane);
        pv_store_row<NCH>(dst + (b * (EXPAND ? S : L + 1) + j) * (int64_t)D, v, nvec, lane);
    }
}

__device__ __forceinline__ void pv_add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// gc[b, L] = g[b, L] + ... + g[b, S - 1]: grid (ceil(nvec / 16), B), thread = (row group rg = tid >> 4, column c = tid & 15)
__global__ __launch_bounds__(256) void pv_rank_tail_sum_kernel(const float* __restrict__ g, float* __restrict__ gc, int S, int L, int D) {
    __shared__ float4 red[16][16];
    const int c = threadIdx.x & 15, rg = threadIdx.x >> 4, nvec = D >> 2;
    const int col = blockIdx.x * 16 + c;
    const int64_t b = blockIdx.y;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < nvec) {
        const float4* gp = reinterpret_cast<const float4*>(g + b * S * (int64_t)D) + col;
        int r = L + rg;
        for (; r + 48 < S; r += 64) {              // four loads in flight, added in row order
            const float4 v0 = gp[(int64_t)r * nvec], v1 = gp[(int64_t)(r + 16) * nvec], v2 = gp[(int64_t)(r + 32) * nvec], v3 = gp[(int64_t)(r + 48) * nvec];
            pv_add4(acc, v0); pv_add4(acc, v1); pv_add4(acc, v2); pv_add4(acc, v3);
        }
        for (; r < S; r += 16) pv_add4(acc, gp[(int64_t)r * nvec]);
    }
    red[rg][c] = acc;
    __syncthreads();
    if (rg == 0 && col < nvec) {
        float4 s = red[0][c];
#pragma unroll
        for (int i = 1; i < 16; ++i) pv_add4(s, red[i][c]);
        reinterpret_cast<float4*>(gc + (b * (L + 1) + L) * (int64_t)D)[col] = s;
    }
}

// grid (ceil(S / 64), B): every workgroup builds the image's inverse map in the LDS (pv_scatter_tokens_kernel's scheme), then writes its 64 rows of dx once
template <int NCH>
__global__ __launch_bounds__(256) void pv_rank_unpack_grad_kernel(const float* __restrict__ dxc, const int32_t* __restrict__ keep, float* __restrict__ dx, int S, int k,
                                                                  int Sc, int D) {
    extern __shared__ int inv[];                     // inv[n] = position of row 1 + n in the kept list, or -1
    const int64_t b = blockIdx.y;
    const int N = S - 1;
    for (int n = threadIdx.x; n < N; n += 256) inv[n] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += 256) {
        const int n = keep[b * k + i];
        if (n >= 0 && n < N) inv[n] = i;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int r1 = min(S, (int)(blockIdx.x + 1) * 64);
    for (int r = blockIdx.x * 64 + wave; r < r1; r += 4) {
        const int src = r == 0 ? 0 : (inv[r - 1] < 0 ? -1 : 1 + inv[r - 1]);
        RowRegs<NCH> v;
        if (src < 0) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) v.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            pv_load_row<NCH>(v, dxc + (b * Sc + src) * (int64_t)D, nvec, lane);
        }
        pv_store_row<NCH>(dx + (b * S + r) * (int64_t)D, v, nvec, lane);
    }
}

// D <= 1024: at most four float4 chunks per lane
#define PV_RANK_DISPATCH(D, MACRO) do { const int nch_ = (int)(((D) / 4 + 63) / 64); if (nch_ <= 1) { MACRO(1); } else if (nch_ == 2) { MACRO(2); } \
                                        else if (nch_ == 3) { MACRO(3); } else { MACRO(4); } } while (0)

static int pv_rank_check(const void* a, const void* b, int64_t B, int64_t S, int64_t D) {
    if (!a || !b || B <= 0 || S < 2 || D <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024 || S - 1 > PV_RANK_MAX_N || B > 0xffff) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

extern "C" int pv_rank_pack_f32(const float* x, const int32_t* keep, float* xc, int64_t B, int64_t S, int64_t k, int64_t D, void* stream) {
    if (!keep || ((uintptr_t)keep & 3) || k < 1 || (S >= 2 && k > S - 1)) return PV_ERR_INVALID_ARG;
    const int rc = pv_rank_check(x, xc, B, S, D);
    if (rc != PV_OK) return rc;
    const int64_t Sc = k + 1 + (k < S - 1 ? 1 : 0);
#define RP_LAUNCH(N) PV_LAUNCH(pv_rank_pack_kernel<N>, dim3(pv_stream_grid(B * Sc, 4)), dim3(256), 0, (hipStream_t)stream, x, keep, xc, B, (int)S, (int)k, (int)Sc, (int)D)
    PV_RANK_DISPATCH(D, RP_LAUNCH);
#undef RP_LAUNCH
    return pv_check_launch();
}

extern "C" int pv_rank_expand_f32(const float* yc, float* y, int64_t B, int64_t S, int64_t L, int64_t D, void* stream) {
    if (L < 1 || (S >= 2 && L >= S)) return PV_ERR_INVALID_ARG;
    const int rc = pv_rank_check(yc, y, B, S, D);
    if (rc != PV_OK) return rc;
#define RE_LAUNCH(N) PV_LAUNCH((pv_rank_rows_kernel<N, true>), dim3(pv_stream_grid(B * S, 4)), dim3(256), 0, (hipStream_t)stream, yc, y, B, (int)S, (int)L, (int)D)
    PV_RANK_DISPATCH(D, RE_LAUNCH);
#undef RE_LAUNCH
    return pv_check_launch();
}

extern "C" int pv_rank_reduce_f32(const float* g, float* gc, int64_t B, int64_t S, int64_t L, int64_t D, void* stream) {
    if (L < 1 || (S >= 2 && L >= S)) return PV_ERR_INVALID_ARG;
    const int rc = pv_rank_check(g, gc, B, S, D);
    if (rc != PV_OK) return rc;
#define RR_LAUNCH(N) PV_LAUNCH((pv_rank_rows_kernel<N, false>), dim3(pv_stream_grid(B * L, 4)), dim3(256), 0, (hipStream_t)stream, g, gc, B, (int)S, (int)L, (int)D)
    PV_RANK_DISPATCH(D, RR_LAUNCH);
#undef RR_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_rank_tail_sum_kernel, dim3((unsigned)((D / 4 + 15) / 16), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, gc, (int)S, (int)L, (int)D);
    return pv_check_launch();
}

extern "C" int pv_rank_unpack_grad_f32(const float* dxc, const int32_t* keep, float* dx, int64_t B, int64_t S, int64_t k, int64_t D, void* stream) {
    if (!keep || ((uintptr_t)keep & 3) || k < 1 || (S >= 2 && k > S - 1)) return PV_ERR_INVALID_ARG;
    const int rc = pv_rank_check(dxc, dx, B, S, D);
    if (rc != PV_OK) return rc;
    const int64_t Sc = k + 1 + (k < S - 1 ? 1 : 0);
#define RU_LAUNCH(N) PV_LAUNCH(pv_rank_unpack_grad_kernel<N>, dim3((unsigned)((S + 63) / 64), (unsigned)B), dim3(256), (size_t)(S - 1) * sizeof(int), (hipStream_t)stream, dxc, keep, dx, (int)S, (int)k, \
                               (int)Sc, (int)D)
    PV_RANK_DISPATCH(D, RU_LAUNCH);
#undef RU_LAUNCH
    return pv_check_launch();
}
