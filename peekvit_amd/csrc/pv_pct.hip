// Point-cloud transformer (reference models/pct.py, include/peekvit_hip_pct.h): the ARPE stem in one launch, the LayerNorm that keeps its
// fp32 rows (the residual a PCT block adds), the mean pool over all rows and the two-layer classification head.
//
// pv_arpe_embed: one workgroup holds the cloud of its image in the LDS (x | y | z planes, 12 N bytes) and serves 64 query points, one wave
// per query at a time.  The k nearest neighbours are pv_knn.h's (distances as bit patterns in registers, a ballot radix select, ties in index
// order), shared with the training path's pv_arpe_knn (pv_pct_train.hip).  The pass over the winners keeps, per channel, the maximum of
// sign(scale1) * z: ELU is monotone and BatchNorm at eval is affine, so the maximum over the neighbours moves in front of both.
#include "pv_rows.h"
#include "pv_knn.h"
#include "../../include/peekvit_hip_pct.h"
#include "../../include/peekvit_hip_rank_train.h"      // pv_layernorm_f32_bf16_masked: an instantiation of pv_layernorm_f32_bf16_kernel
#include "../../include/peekvit_hip_rank_infer.h"      // pv_layernorm_gather_f32_bf16: another one

template <int NI>
__global__ __launch_bounds__(256) void pv_arpe_kernel(const float* __restrict__ points, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ s1, const float* __restrict__ t1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, const float* __restrict__ s2, const float* __restrict__ t2,
                                                      float* __restrict__ tokens, int32_t* __restrict__ idx_out, int N, int k, int D, int64_t S,
                                                      int64_t row_off, int bpi) {
    extern __shared__ float pv_arpe_lds[];
    float* const sx = pv_arpe_lds;
    float* const sy = pv_arpe_lds + N;
    float* const sz = pv_arpe_lds + 2 * N;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    pv_knn_stage_cloud(pv_arpe_lds, points + (int64_t)b * N * 3, N, threadIdx.x, 256);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    float W[6][6], bias[6], sg[6], sc[6], sh[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int i = 0; i < 6; ++i) W[c][i] = w1[c * 6 + i];
        bias[c] = b1[c];
        sc[c] = s1[c];
        sh[c] = t1[c];
        sg[c] = sc[c] < 0.f ? -1.f : 1.f;
    }
    for (int qi = 0; qi < PV_ARPE_QPB / 4; ++qi) {
        const int q = blk * PV_ARPE_QPB + qi * 4 + wave;          // (wave-uniform)
        if (q >= N) break;
        const float qx = sx[q], qy = sy[q], qz = sz[q];
        uint32_t key[NI];
        pv_knn_keys<NI>(key, sx, sy, sz, qx, qy, qz, N, lane);
        uint32_t prefix;
        int kr;
        pv_knn_threshold<NI>(key, k, prefix, kr);
        float a[6], m[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            a[c] = bias[c] + W[c][0] * qx + W[c][1] * qy + W[c][2] * qz;
            m[c] = -__builtin_inff();
        }
        int32_t* const io = idx_out ? idx_out + ((int64_t)b * N + q) * k : nullptr;
        int pos = 0;
        pv_knn_winners<NI>(key, prefix, kr, N, lane, [&](int j, bool sel) {
            if (io) pv_knn_emit(io, j, sel, k, lane, pos);
            if (sel) {
                const float dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const float z = a[c] + W[c][3] * dx + W[c][4] * dy + W[c][5] * dz;
                    m[c] = fmaxf(m[c], sg[c] * z);
                }
            }
        });
        float h[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) h[c] = pv_elu(sc[c] * (sg[c] * pv_wave_max(m[c])) + sh[c]);
        // 6 -> D, BatchNorm 2, ELU: a lane writes 16-byte chunks of the token row
        float* const orow = tokens + (((int64_t)b * S + row_off + q) * D);
        for (int idx = lane; idx < nvec; idx += 64) {
            const float4* wp = reinterpret_cast<const float4*>(w2 + 24 * (int64_t)idx);
            float wr[24];
#pragma unroll
            for (int v = 0; v < 6; ++v) {
                const float4 t = wp[v];
                wr[4 * v] = t.x; wr[4 * v + 1] = t.y; wr[4 * v + 2] = t.z; wr[4 * v + 3] = t.w;
            }
            const float4 bv = reinterpret_cast<const float4*>(b2)[idx], sv = reinterpret_cast<const float4*>(s2)[idx],
                         tv = reinterpret_cast<const float4*>(t2)[idx];
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w}, ss[4] = {sv.x, sv.y, sv.z, sv.w}, tt[4] = {tv.x, tv.y, tv.z, tv.w};
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float y = bb[r];
#pragma unroll
                for (int c = 0; c < 6; ++c) y = fmaf(wr[6 * r + c], h[c], y);
                o[r] = pv_elu(ss[r] * y + tt[r]);
            }
            reinterpret_cast<float4*>(orow)[idx] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

extern "C" int pv_arpe_embed(const float* points, const float* w1, const float* b1, const float* bn1_scale, const float* bn1_shift, const float* w2,
                             const float* b2, const float* bn2_scale, const float* bn2_shift, float* tokens, int32_t* idx_out, int64_t B, int64_t N,
                             int64_t k, int64_t D, int64_t S, int64_t row_off, void* stream) {
    if (!points || !w1 || !b1 || !bn1_scale || !bn1_shift || !w2 || !b2 || !bn2_scale || !bn2_shift || !tokens) return PV_ERR_INVALID_ARG;
    if (B <= 0 || N <= 0 || k <= 0 || D <= 0 || S <= 0 || row_off < 0) return PV_ERR_INVALID_ARG;
    if (N < PV_ARPE_MIN_N || N > PV_ARPE_MAX_N || D % 4 || D > PV_ARPE_MAX_D) return PV_ERR_UNSUPPORTED;
    if (k > N || row_off > S || N > S - row_off) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)points | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)bn1_scale | (uintptr_t)bn1_shift | (uintptr_t)idx_out) & 3) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)tokens | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)bn2_scale | (uintptr_t)bn2_shift) & 15) return PV_ERR_INVALID_ARG;
    const int64_t bpi = (N + PV_ARPE_QPB - 1) / PV_ARPE_QPB;
    if (B * bpi > 0x7fffffff || S > ((int64_t)1 << 40) / D) return PV_ERR_UNSUPPORTED;
    const int ni = (int)((N + 63) / 64);
    const dim3 grid((unsigned)(B * bpi));
    const size_t lds = (size_t)N * 12;
#define ARPE_LAUNCH(NI_) PV_LAUNCH(pv_arpe_kernel<NI_>, grid, dim3(256), lds, (hipStream_t)stream, points, w1, b1, bn1_scale, bn1_shift, w2, b2, \
                                   bn2_scale, bn2_shift, tokens, idx_out, (int)N, (int)k, (int)D, S, row_off, (int)bpi)
    if (ni <= 1) { ARPE_LAUNCH(1); }
    else if (ni <= 2) { ARPE_LAUNCH(2); }
    else if (ni <= 4) { ARPE_LAUNCH(4); }
    else if (ni <= 8) { ARPE_LAUNCH(8); }
    else if (ni <= 16) { ARPE_LAUNCH(16); }
    else if (ni <= 32) { ARPE_LAUNCH(32); }
    else { ARPE_LAUNCH(64); }
#undef ARPE_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// LayerNorm with both planes: pv_rows.h's row LayerNorm and 16-bit store, as pv_layernorm_kernel (pv_rowops.hip) without a row scale, plus
// the fp32 rows
// ------------------------------------------------------------------------------------------------
// MASKED (pv_layernorm_f32_bf16_masked, include/peekvit_hip_rank_train.h): the row is multiplied by row_scale[row] before BOTH stores (a scale of
// 1 changes no bit, a scale of 0 leaves zeros in both planes)
// GATHER (pv_layernorm_gather_f32_bf16, include/peekvit_hip_rank_infer.h): x is [B, S, ldx] and output row b (1 + k) + j reads row 0 (j == 0) or row
// 1 + keep[b, j - 1] of image b, the index clamped to the image; the outputs stay contiguous
template <int NCH, bool MASKED = false, bool GATHER = false>
__global__ __launch_bounds__(256) void pv_layernorm_f32_bf16_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, uint16_t* __restrict__ out16,
                                                                    float* __restrict__ out32, int64_t ld32, int64_t rows, int D, float eps,
                                                                    const float* __restrict__ row_scale = nullptr,
                                                                    const int32_t* __restrict__ keep = nullptr, int S = 0, int k = 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        RowRegs<NCH> r;
        int64_t src = row;
        if constexpr (GATHER) {
            const int64_t b = row / (k + 1);
            const int j = (int)(row - b * (k + 1));
            int n = 0;
            if (j > 0) {
                n = keep[b * k + (j - 1)];
                n = 1 + (n < 0 ? 0 : (n > S - 2 ? S - 2 : n));
            }
            src = b * S + n;
        }
        pv_load_row<NCH>(r, x + src * ldx, nvec, lane);
        pv_ln_row<NCH>(r, gamma, beta, D, nvec, lane, eps);
        if constexpr (MASKED) {
            const float sc = row_scale[row];
#pragma unroll
            for (int j = 0; j < NCH; ++j) { r.v[j].x *= sc; r.v[j].y *= sc; r.v[j].z *= sc; r.v[j].w *= sc; }
        }
        pv_store_row16<NCH>(out16 + row * (int64_t)D, r, nvec, lane);
        pv_store_row<NCH>(out32 + row * ld32, r, nvec, lane);
    }
}

extern "C" int pv_layernorm_f32_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta, uint16_t* out16, float* out32, int64_t ld32,
                                     int64_t rows, int64_t D, float eps, void* stream) {
    if (!x || !gamma || !beta || !out16 || !out32 || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    if (ldx % 4 || ldx < D || ld32 % 4 || ld32 < D) return PV_ERR_INVALID_ARG;
    if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out32) & 15) || ((uintptr_t)out16 & 7)) return PV_ERR_INVALID_ARG;
    if (rows > ((int64_t)1 << 40) / (ldx > ld32 ? ldx : ld32)) return PV_ERR_UNSUPPORTED;
    {   // the fp32 rows must not land on the rows being read
        const uintptr_t a0 = (uintptr_t)x, a1 = a0 + (uintptr_t)((rows - 1) * ldx + D) * 4;
        const uintptr_t b0 = (uintptr_t)out32, b1 = b0 + (uintptr_t)((rows - 1) * ld32 + D) * 4;
        if (a0 < b1 && b0 < a1) return PV_ERR_INVALID_ARG;
    }
    const dim3 grid(pv_stream_grid(rows, 4));
#define LNF_LAUNCH(N_) PV_LAUNCH(pv_layernorm_f32_bf16_kernel<N_>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta, out16, out32, ld32, rows, \
                                 (int)D, eps)
    PV_DISPATCH_NCH(D, LNF_LAUNCH);
#undef LNF_LAUNCH
    return pv_check_launch();
}

// The same LayerNorm times a per-row scale (include/peekvit_hip_rank_train.h): the MASKED instantiation; contiguous rows.
extern "C" int pv_layernorm_f32_bf16_masked(const float* x, const float* gamma, const float* beta, const float* row_scale, uint16_t* out16, float* out32,
                                            int64_t rows, int64_t D, float eps, void* stream) {
    if (!x || !gamma || !beta || !row_scale || !out16 || !out32 || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out32) & 15) || ((uintptr_t)out16 & 7) || ((uintptr_t)row_scale & 3)) return PV_ERR_INVALID_ARG;
    if (rows > ((int64_t)1 << 40) / D) return PV_ERR_UNSUPPORTED;
    {   // the fp32 rows must not land on the rows being read
        const uintptr_t a0 = (uintptr_t)x, a1 = a0 + (uintptr_t)(rows * D) * 4, b0 = (uintptr_t)out32, b1 = b0 + (uintptr_t)(rows * D) * 4;
        if (a0 < b1 && b0 < a1) return PV_ERR_INVALID_ARG;
    }
    const dim3 grid(pv_stream_grid(rows, 4));
#define LNFM_LAUNCH(N_) PV_LAUNCH((pv_layernorm_f32_bf16_kernel<N_, true>), grid, dim3(256), 0, (hipStream_t)stream, x, D, gamma, beta, out16, out32, D, rows, \
                                  (int)D, eps, row_scale)
    PV_DISPATCH_NCH(D, LNFM_LAUNCH);
#undef LNFM_LAUNCH
    return pv_check_launch();
}

// The same LayerNorm with its rows read through a ranking (include/peekvit_hip_rank_infer.h): the GATHER instantiation; contiguous rows.
extern "C" int pv_layernorm_gather_f32_bf16(const float* x, const int32_t* keep, const float* gamma, const float* beta, uint16_t* out16, float* out32,
                                            int64_t B, int64_t S, int64_t k, int64_t D, float eps, void* stream) {
    if (!x || !gamma || !beta || !out16 || !out32 || B <= 0 || S <= 0 || D <= 0 || k < 0 || k > S - 1 || (k > 0 && !keep)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out32) & 15) || ((uintptr_t)out16 & 7) || ((uintptr_t)keep & 3)) return PV_ERR_INVALID_ARG;
    if (S > 0x7fffffff || B > ((int64_t)1 << 40) / D / S) return PV_ERR_UNSUPPORTED;
    const int64_t rows = B * (k + 1);
    {   // the fp32 rows must not land on the rows being read
        const uintptr_t a0 = (uintptr_t)x, a1 = a0 + (uintptr_t)(B * S * D) * 4, b0 = (uintptr_t)out32, b1 = b0 + (uintptr_t)(rows * D) * 4;
        if (a0 < b1 && b0 < a1) return PV_ERR_INVALID_ARG;
    }
    const dim3 grid(pv_stream_grid(rows, 4));
#define LNFG_LAUNCH(N_) PV_LAUNCH((pv_layernorm_f32_bf16_kernel<N_, false, true>), grid, dim3(256), 0, (hipStream_t)stream, x, D, gamma, beta, out16, out32, D, rows, \
                                  (int)D, eps, (const float*)nullptr, keep, (int)S, (int)k)
    PV_DISPATCH_NCH(D, LNFG_LAUNCH);
#undef LNFG_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// mean over the rows of an image: 16 float4 columns x 16 row groups per workgroup
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pv_kahan_add(float& s, float& c, float v) {
#pragma clang fp contract(off)
    const float y = v - c;
    const float t = s + y;
    c = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(256) void pv_mean_pool_kernel(const float* __restrict__ x, float* __restrict__ pooled, int S, int nvec, int tiles) {
#pragma clang fp contract(off)
    __shared__ float4 part[16][17];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int cv = threadIdx.x & 15, g = threadIdx.x >> 4, col = tile * 16 + cv;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
    if (col < nvec) {
        const float4* xp = reinterpret_cast<const float4*>(x) + (int64_t)b * S * nvec + col;
        for (int r = g; r < S; r += 16) {
            const float4 v = xp[(int64_t)r * nvec];
            pv_kahan_add(s[0], c[0], v.x); pv_kahan_add(s[1], c[1], v.y); pv_kahan_add(s[2], c[2], v.z); pv_kahan_add(s[3], c[3], v.w);
        }
    }
    part[g][cv] = make_float4(s[0], s[1], s[2], s[3]);
    __syncthreads();
    if (g == 0 && col < nvec) {
        float t[16][4];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 v = part[i][cv];
            t[i][0] = v.x; t[i][1] = v.y; t[i][2] = v.z; t[i][3] = v.w;
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int i = 0; i < w; ++i) t[i][e] = t[i][e] + t[i + w][e];
            o[e] = t[0][e] / (float)S;
        }
        reinterpret_cast<float4*>(pooled)[(int64_t)b * nvec + col] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

extern "C" int pv_mean_pool_f32(const float* x, float* pooled, int64_t B, int64_t S, int64_t D, void* stream) {
    if (!x || !pooled || B <= 0 || S <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)pooled) & 15) return PV_ERR_INVALID_ARG;
    const int64_t nvec = D / 4, tiles = (nvec + 15) / 16;
    if (S > 0x7fffffff || nvec > 0x7fffffff || B * tiles > 0x7fffffff || S > ((int64_t)1 << 40) / D / B) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_mean_pool_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, (hipStream_t)stream, x, pooled, (int)S, (int)nvec, (int)tiles);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// classification head: one workgroup per image, one wave per dot product
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_pct_head_kernel(const float* __restrict__ pooled, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ bs, const float* __restrict__ bt, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ logits, int D, int Hd, int C) {
    extern __shared__ float pv_head_lds[];
    float* const sp = pv_head_lds;
    float* const hid = pv_head_lds + D;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < D; d += 256) sp[d] = pooled[(int64_t)b * D + d];
    __syncthreads();
    for (int j = wave; j < Hd; j += 4) {
        const float* wr = w1 + (int64_t)j * D;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(sp[d], wr[d], acc);
        acc = pv_wave_sum(acc);
        if (lane == 0) hid[j] = pv_gelu_erf(bs[j] * (acc + (b1 ? b1[j] : 0.f)) + bt[j]);
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        const float* wr = w2 + (int64_t)c * Hd;
        float acc = 0.f;
        for (int d = lane; d < Hd; d += 64) acc = fmaf(hid[d], wr[d], acc);
        acc = pv_wave_sum(acc);
        if (lane == 0) logits[(int64_t)b * C + c] = acc + (b2 ? b2[c] : 0.f);
    }
}

extern "C" int pv_pct_head_f32(const float* pooled, const float* w1, const float* b1, const float* bn_scale, const float* bn_shift, const float* w2,
                               const float* b2, float* logits, int64_t B, int64_t D, int64_t Hd, int64_t C, void* stream) {
    if (!pooled || !w1 || !bn_scale || !bn_shift || !w2 || !logits || B <= 0 || D <= 0 || Hd <= 0 || C <= 0) return PV_ERR_INVALID_ARG;
    if (D > PV_PCT_HEAD_MAX_D || Hd > PV_PCT_HEAD_MAX_D || B > 0x7fffffff || C > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)pooled | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)bn_scale | (uintptr_t)bn_shift | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)logits) & 3)
        return PV_ERR_INVALID_ARG;
    PV_LAUNCH(pv_pct_head_kernel, dim3((unsigned)B), dim3(256), (size_t)(D + Hd) * 4, (hipStream_t)stream, pooled, w1, b1, bn_scale, bn_shift, w2, b2,
              logits, (int)D, (int)Hd, (int)C);
    return pv_check_launch();
}
