// HBM-bound row kernels of the ViT encoder hot path (gfx950): cast, im2col, token prologue, LayerNorm,
// CLS pooling, fp32 head, token norms, rank/top-k, compaction gather, residual gate.
// One wave (64 lanes) owns one token row; 16-byte vector accesses; grid-stride over rows.
#include "pv_rows.h"
#include "../../include/peekvit_hip_pct_block.h"      // pv_layernorm_bwd_sum: an instantiation of pv_layernorm_bwd_kernel
#include "../../include/peekvit_hip_rank_train.h"     // pv_layernorm_bwd_sum_masked: the same, dy times a per-row scale

// ------------------------------------------------------------------------------------------------
// fp32 -> bf16 cast
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_cast_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    int64_t nvec = n >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const float4* s = reinterpret_cast<const float4*>(src) + i * 2;
        float4 a = s[0], b = s[1];
        u32x4 o = {pv_pack_bf16x2(a.x, a.y), pv_pack_bf16x2(a.z, a.w), pv_pack_bf16x2(b.x, b.y), pv_pack_bf16x2(b.z, b.w)};
        reinterpret_cast<u32x4*>(dst)[i] = o;
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nvec << 3) + threadIdx.x; i < n; i += 256) dst[i] = pv_f2bf(src[i]);
    }
}

extern "C" int pv_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream) {
    if (!src || !dst || n < 0) return PV_ERR_INVALID_ARG;
    if (n == 0) return PV_OK;
    if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return PV_ERR_INVALID_ARG;
    PV_LAUNCH(pv_cast_kernel, dim3(pv_stream_grid((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// split-precision packing (precision mode "bf16x3"): src fp32 [rows, K] -> dst bf16 [rows, 3K]
//   order 0 (activations): [hi | lo | hi]      order 1 (weights): [hi | hi | lo]
// so that dst_act . dst_w^T = a_hi.w_hi + a_lo.w_hi + a_hi.w_lo  - the plain bf16 MFMA GEMM at 3K gives ~fp32 products.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_split3_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t rows, int K, int order) {
    const int K4 = K >> 2;
    const int64_t total = rows * K4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t r = idx / K4;
        const int k = (int)(idx - r * K4) << 2;
        const float4 v = *reinterpret_cast<const float4*>(src + r * K + k);
        u32x2 hi, lo;
        { const PvHiLo t_ = pv_split2(v.x, v.y); hi[0] = t_.hi; lo[0] = t_.lo; }
        { const PvHiLo t_ = pv_split2(v.z, v.w); hi[1] = t_.hi; lo[1] = t_.lo; }
        uint16_t* d = dst + r * 3 * (int64_t)K + k;
        *reinterpret_cast<u32x2*>(d) = hi;
        *reinterpret_cast<u32x2*>(d + K) = order == 0 ? lo : hi;
        *reinterpret_cast<u32x2*>(d + 2 * K) = order == 0 ? hi : lo;
    }
}

extern "C" int pv_split3_f32_bf16(const float* src, uint16_t* dst, int64_t rows, int64_t K, int order, void* stream) {
    if (!src || !dst || rows <= 0 || K <= 0 || (order != 0 && order != 1)) return PV_ERR_INVALID_ARG;
    if (K % 4 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_split3_kernel, dim3(pv_stream_grid(rows * (K / 4), 256)), dim3(256), 0, (hipStream_t)stream, src, dst, rows, (int)K, order);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// im2col for the stride-P / kernel-P patch convolution (models/vit.py:212)
// ------------------------------------------------------------------------------------------------
template <bool VEC, bool SPLIT = false>
__global__ __launch_bounds__(256) void pv_im2col_kernel(const float* __restrict__ x, uint16_t* __restrict__ cols, int64_t B, int C,
                                                        int H, int W, int P, uint32_t* range_flag) {
    const int Hp = H / P, Wp = W / P, Np = Hp * Wp, K = C * P * P;
    float vmax = 0.f;          // operand-range guard (fp16 build; compiled away otherwise)
    if (VEC) {
        const int K8 = K >> 3;
        const int64_t total = B * (int64_t)Np * K8;
        for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
            int64_t m = idx / K8;
            int k = (int)(idx - m * K8) << 3;
            int c = k / (P * P), kh = (k / P) % P, kw = k % P;
            int64_t b = m / Np;
            int pi = (int)(m - b * Np), ph = pi / Wp, pw = pi - ph * Wp;
            const float* s = x + ((b * C + c) * H + (int64_t)ph * P + kh) * W + pw * P + kw;
            float4 a = reinterpret_cast<const float4*>(s)[0], d = reinterpret_cast<const float4*>(s)[1];
            if (SPLIT) {          // [hi | lo | hi] rows of 3K
                u32x4 hi, lo;
                { const PvHiLo t_ = pv_split2(a.x, a.y); hi[0] = t_.hi; lo[0] = t_.lo; } { const PvHiLo t_ = pv_split2(a.z, a.w); hi[1] = t_.hi; lo[1] = t_.lo; }
                { const PvHiLo t_ = pv_split2(d.x, d.y); hi[2] = t_.hi; lo[2] = t_.lo; } { const PvHiLo t_ = pv_split2(d.z, d.w); hi[3] = t_.hi; lo[3] = t_.lo; }
                uint16_t* o = cols + m * 3 * (int64_t)K + k;
                *reinterpret_cast<u32x4*>(o) = hi;
                *reinterpret_cast<u32x4*>(o + K) = lo;
                *reinterpret_cast<u32x4*>(o + 2 * K) = hi;
            } else {
                u32x4 o = {pv_pack_bf16x2_tracked(a.x, a.y, vmax), pv_pack_bf16x2_tracked(a.z, a.w, vmax), pv_pack_bf16x2_tracked(d.x, d.y, vmax),
                           pv_pack_bf16x2_tracked(d.z, d.w, vmax)};
                reinterpret_cast<u32x4*>(cols)[idx] = o;
            }
        }
    } else {
        const int64_t total = B * (int64_t)Np * K;
        for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
            int64_t m = idx / K;
            int k = (int)(idx - m * K);
            int c = k / (P * P), kh = (k / P) % P, kw = k % P;
            int64_t b = m / Np;
            int pi = (int)(m - b * Np), ph = pi / Wp, pw = pi - ph * Wp;
            const float v = x[((b * C + c) * H + (int64_t)ph * P + kh) * W + pw * P + kw];
            pv_range_track(vmax, v, v);
            cols[idx] = pv_f2bf(v);
        }
    }
    if (!SPLIT) pv_range_commit(vmax, range_flag);
}

extern "C" int pv_im2col_split_bf16(const float* x, uint16_t* cols, int64_t B, int64_t C, int64_t H, int64_t W, int64_t P, void* stream) {
    if (!x || !cols || B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || H % P || W % P) return PV_ERR_INVALID_ARG;
    if (P % 8 || W % 4 || ((uintptr_t)x & 15) || ((uintptr_t)cols & 15)) return PV_ERR_UNSUPPORTED;
    const int64_t work = B * (H / P) * (W / P) * (C * P * P / 8);
    PV_LAUNCH((pv_im2col_kernel<true, true>), dim3(pv_stream_grid(work, 256)), dim3(256), 0, (hipStream_t)stream, x, cols, B, (int)C, (int)H, (int)W, (int)P,
              (uint32_t*)nullptr);
    return pv_check_launch();
}

extern "C" int pv_im2col_bf16(const float* x, uint16_t* cols, int64_t B, int64_t C, int64_t H, int64_t W, int64_t P, uint32_t* range_flag,
                              void* stream) {
    if (!x || !cols || B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || ((uintptr_t)range_flag & 3)) return PV_ERR_INVALID_ARG;
    if (H % P || W % P) return PV_ERR_INVALID_ARG;
    const bool vec = (P % 8 == 0) && (W % 4 == 0) && !((uintptr_t)x & 15) && !((uintptr_t)cols & 15);
    const int64_t K = C * P * P, work = B * (H / P) * (W / P) * (vec ? K / 8 : K);
    dim3 grid(pv_stream_grid(work, 256));
    if (vec)
        PV_LAUNCH(pv_im2col_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, cols, B, (int)C, (int)H, (int)W, (int)P, range_flag);
    else
        PV_LAUNCH(pv_im2col_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, cols, B, (int)C, (int)H, (int)W, (int)P, range_flag);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// uint8 NHWC input pipeline fused into the patch gather: the DataLoader's ToTensor + Normalize
// (reference data/imagenette.py:73: x/255, then (x - mean)/std, fp32) happen here, per element, in the same op order, so the
// bf16 patch matrix is bit-identical to im2col of the normalised fp32 NCHW tensor - at 1/4 of the input bytes.
// ------------------------------------------------------------------------------------------------
struct PvNorm3 { float mean[3], std[3]; };

__global__ __launch_bounds__(256) void pv_im2col_u8_kernel(const uint8_t* __restrict__ x, uint16_t* __restrict__ cols, int64_t B, int H, int W,
                                                           int P, PvNorm3 nm) {
    const int Hp = H / P, Wp = W / P, Np = Hp * Wp, K = 3 * P * P, K8 = K >> 3;
    const int64_t total = B * (int64_t)Np * K8;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t m = idx / K8;
        const int k = (int)(idx - m * K8) << 3;
        const int c = k / (P * P), kh = (k / P) % P, kw = k % P;
        const int64_t b = m / Np;
        const int pi = (int)(m - b * Np), ph = pi / Wp, pw = pi - ph * Wp;
        const uint8_t* s = x + ((b * H + (int64_t)ph * P + kh) * W + pw * P + kw) * 3 + c;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ((float)s[3 * j] / 255.0f - nm.mean[c]) / nm.std[c];
        u32x4 o = {pv_pack_bf16x2(v[0], v[1]), pv_pack_bf16x2(v[2], v[3]), pv_pack_bf16x2(v[4], v[5]), pv_pack_bf16x2(v[6], v[7])};
        reinterpret_cast<u32x4*>(cols)[idx] = o;
    }
}

extern "C" int pv_im2col_u8_bf16(const uint8_t* x, uint16_t* cols, int64_t B, int64_t H, int64_t W, int64_t P, float mean0, float mean1,
                                 float mean2, float std0, float std1, float std2, void* stream) {
    if (!x || !cols || B <= 0 || H <= 0 || W <= 0 || P <= 0 || H % P || W % P) return PV_ERR_INVALID_ARG;
    if (std0 == 0.f || std1 == 0.f || std2 == 0.f) return PV_ERR_INVALID_ARG;
    if (P % 8 || ((uintptr_t)cols & 15)) return PV_ERR_UNSUPPORTED;
    const int64_t work = B * (H / P) * (W / P) * (3 * P * P / 8);
    PvNorm3 nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    PV_LAUNCH(pv_im2col_u8_kernel, dim3(pv_stream_grid(work, 256)), dim3(256), 0, (hipStream_t)stream, x, cols, B, (int)H, (int)W, (int)P, nm);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// backward helpers: split-K slice reduction, bf16 transpose, column sums
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_sum_slices_kernel(const float* __restrict__ part, const float* base, float* out, int64_t n, int slices) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = base ? reinterpret_cast<const float4*>(base)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < slices; ++t) {
            const float4 v = reinterpret_cast<const float4*>(part + (int64_t)t * n)[i];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        reinterpret_cast<float4*>(out)[i] = s;
    }
}

extern "C" int pv_sum_slices_f32(const float* partials, float* out, int64_t n_elems, int64_t slices, int accumulate, void* stream) {
    if (!partials || !out || n_elems <= 0 || slices <= 0) return PV_ERR_INVALID_ARG;
    if (n_elems % 4 || ((uintptr_t)partials & 15) || ((uintptr_t)out & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_sum_slices_kernel, dim3(pv_stream_grid(n_elems / 4, 256)), dim3(256), 0, (hipStream_t)stream, partials, accumulate ? (const float*)out : (const float*)nullptr, out,
              n_elems, (int)slices);
    return pv_check_launch();
}

// out = base + sum of the slices (base may be out): the second half of a split-K GEMM with a residual - the small-batch form of
// PV_EPI_BIAS_RES_F32 (slice 0 carries the bias), where M rows alone would put a dozen workgroups on 256 CUs.
extern "C" int pv_sum_slices_add_f32(const float* partials, const float* base, float* out, int64_t n_elems, int64_t slices, void* stream) {
    if (!partials || !base || !out || n_elems <= 0 || slices <= 0) return PV_ERR_INVALID_ARG;
    if (n_elems % 4 || ((uintptr_t)partials & 15) || ((uintptr_t)out & 15) || ((uintptr_t)base & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_sum_slices_kernel, dim3(pv_stream_grid(n_elems / 4, 256)), dim3(256), 0, (hipStream_t)stream, partials, base, out, n_elems, (int)slices);
    return pv_check_launch();
}

// Elementwise finish of a split-K GEMM with a 16-bit output (small batches): out16 = f(sum of slices), f = exact GELU (fc1, models/blocks.py:82) or
// the q pre-scale of the in-projection (columns < qcols times qscale); slice 0 carries the bias.  Tracks the operand range like the GEMM epilogues.
__global__ __launch_bounds__(256) void pv_sum_slices_act_kernel(const float* __restrict__ part, uint16_t* __restrict__ out, int64_t M, int N, int slices, int gelu,
                                                                int qcols, float qscale, uint32_t* range_flag) {
    const int64_t n = M * N, n4 = n >> 2;
    float vmax = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = reinterpret_cast<const float4*>(part)[i];
        for (int t = 1; t < slices; ++t) {
            const float4 v = reinterpret_cast<const float4*>(part + (int64_t)t * n)[i];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (gelu) {
            s.x = pv_gelu_fast(s.x); s.y = pv_gelu_fast(s.y); s.z = pv_gelu_fast(s.z); s.w = pv_gelu_fast(s.w);
        } else if ((int)((i * 4) % N) < qcols) {          // N % 4 == 0 and qcols % 4 == 0: the four columns are on one side
            s.x *= qscale; s.y *= qscale; s.z *= qscale; s.w *= qscale;
        }
        reinterpret_cast<u32x2*>(out)[i] = (u32x2){pv_pack_bf16x2_tracked(s.x, s.y, vmax), pv_pack_bf16x2_tracked(s.z, s.w, vmax)};
    }
    pv_range_commit(vmax, range_flag);
}

extern "C" int pv_sum_slices_act_bf16(const float* partials, uint16_t* out, int64_t M, int64_t N, int64_t slices, int gelu, int64_t qcols, float qscale,
                                      uint32_t* range_flag, void* stream) {
    if (!partials || !out || M <= 0 || N <= 0 || slices <= 0) return PV_ERR_INVALID_ARG;
    if (N % 4 || qcols % 4 || N > 0x7fffffff || ((uintptr_t)partials & 15) || ((uintptr_t)out & 7)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_sum_slices_act_kernel, dim3(pv_stream_grid(M * N / 4, 256)), dim3(256), 0, (hipStream_t)stream, partials, out, M, (int)N, (int)slices, gelu,
              (int)qcols, qscale, range_flag);
    return pv_check_launch();
}

// Row-wise finish of a split-K residual GEMM that ALSO emits the LayerNorm the consumer applies to the finished rows (small batches, where a
// LayerNorm launch is latency, not bandwidth): one wave per row keeps it in registers - out = base + sum of slices, ln_out = 16-bit LN(out).
// Same row arithmetic as pv_layernorm_bf16 (pv_ln_row, pv_rows.h).
template <int NCH>
__global__ __launch_bounds__(256) void pv_sum_slices_ln_kernel(const float* __restrict__ part, const float* base, float* out, int64_t rows, int D, int slices,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               uint16_t* __restrict__ ln_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t n = rows * D;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, base + row * D, nvec, lane);
        for (int t = 0; t < slices; ++t) {
            RowRegs<NCH> v;
            pv_load_row<NCH>(v, part + (int64_t)t * n + row * D, nvec, lane);
#pragma unroll
            for (int j = 0; j < NCH; ++j) { r.v[j].x += v.v[j].x; r.v[j].y += v.v[j].y; r.v[j].z += v.v[j].z; r.v[j].w += v.v[j].w; }
        }
        pv_store_row<NCH>(out + row * D, r, nvec, lane);
        pv_ln_row<NCH>(r, gamma, beta, D, nvec, lane, eps);
        pv_store_row16<NCH>(ln_out + row * (int64_t)D, r, nvec, lane);
    }
}

// 64 x 64 tiles through LDS; a workgroup walks a 64-column strip over 1024 source rows (16 tiles).  Fast path (C, lds, ldd
// multiples of 8, 16-byte aligned): 16-byte global loads and stores, the transposition happens in the LDS read (8 two-byte
// reads down a tile column).  CSUM: the strip's column sums over those 1024 rows fall out of the loaded registers and go
// to ws[chunk][C] (bias gradient = column sums of the dY being transposed for the weight gradient; pv_colsum stage 2 ends it).
template <bool VEC, bool CSUM>
__global__ __launch_bounds__(256) void pv_transpose_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t R, int64_t C,
                                                           int64_t lds, int64_t ldd, float* __restrict__ ws, int crows) {
    __shared__ uint16_t tile[64][72];          // 144-byte rows: 16-byte aligned chunks, 36-bank pitch
    __shared__ float red[32][65];
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    const int64_t rbeg = (int64_t)blockIdx.y * crows, rend = rbeg + crows < ldd ? rbeg + crows : ldd;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int rr = threadIdx.x >> 3, ch = threadIdx.x & 7;
    for (int64_t r0 = rbeg; r0 < rend; r0 += 64) {
        if (VEC) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t r = r0 + rr + 32 * h, c = c0 + ch * 8;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (r < R && c < C) v = *reinterpret_cast<const u32x4*>(src + r * lds + c);
                *reinterpret_cast<u32x4*>(&tile[rr + 32 * h][ch * 8]) = v;
                if (CSUM) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        cs[2 * k] += pv_unpack_lo(v[k]);
                        cs[2 * k + 1] += pv_unpack_hi(v[k]);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int oc = rr + 32 * h;                                  // output row = source column
                const int64_t orow = c0 + oc, ocol = r0 + ch * 8;
                if (orow < C && ocol < ldd) {
                    uint32_t w[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)tile[ch * 8 + 2 * k][oc] | ((uint32_t)tile[ch * 8 + 2 * k + 1][oc] << 16);
                    *reinterpret_cast<u32x4*>(dst + orow * ldd + ocol) = (u32x4){w[0], w[1], w[2], w[3]};
                }
            }
        } else {
            const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
            for (int i = ty; i < 64; i += 4) {
                const uint16_t v = (r0 + i < R && c0 + tx < C) ? src[(r0 + i) * lds + c0 + tx] : (uint16_t)0;
                tile[i][tx] = v;
                if (CSUM) cs[0] += pv_bf2f(v);
            }
            __syncthreads();
            for (int i = ty; i < 64; i += 4)
                if (c0 + i < C && r0 + tx < ldd) dst[(c0 + i) * ldd + r0 + tx] = tile[tx][i];      // columns R..ldd-1 are zero padding
        }
        __syncthreads();
    }
    if (CSUM) {
        if (VEC) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[rr][ch * 8 + k] = cs[k];
        } else if (threadIdx.x < 64 * 4) {
            red[threadIdx.x >> 6][threadIdx.x & 63] = cs[0];
        }
        __syncthreads();
        if (threadIdx.x < 64 && c0 + threadIdx.x < C) {
            float t = 0.f;
            for (int k = 0; k < (VEC ? 32 : 4); ++k) t += red[k][threadIdx.x];
            ws[(int64_t)blockIdx.y * C + c0 + threadIdx.x] = t;
        }
    }
}

__global__ __launch_bounds__(256) void pv_colsum_stage2_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t chunks, int C, int accumulate);

extern "C" int pv_transpose_bf16(const uint16_t* src, int64_t lds, uint16_t* dst, int64_t R, int64_t C, int64_t ldd, float* colsum_out,
                                 float* colsum_ws, void* stream) {
    if (!src || !dst || R <= 0 || C <= 0 || ldd < R || lds < C) return PV_ERR_INVALID_ARG;
    if (colsum_out && !colsum_ws) return PV_ERR_INVALID_ARG;
    const int crows = ldd <= 65536 ? 64 : 1024;          // source rows per workgroup: a weight matrix (<= 4096 rows) would otherwise be 12-48 workgroups
    const int64_t chunks = (ldd + crows - 1) / crows;
    dim3 grid((unsigned)((C + 63) / 64), (unsigned)chunks);
    if (chunks > 65535 || C > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    const bool vec = C % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0 && !((uintptr_t)src & 15) && !((uintptr_t)dst & 15);
    hipStream_t s = (hipStream_t)stream;
    if (colsum_out) {
        if (vec) PV_LAUNCH((pv_transpose_kernel<true, true>), grid, dim3(256), 0, s, src, dst, R, C, lds, ldd, colsum_ws, crows);
        else PV_LAUNCH((pv_transpose_kernel<false, true>), grid, dim3(256), 0, s, src, dst, R, C, lds, ldd, colsum_ws, crows);
        if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
        PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, s, (const float*)colsum_ws, colsum_out, chunks, (int)C, 0);
    } else {
        if (vec) PV_LAUNCH((pv_transpose_kernel<true, false>), grid, dim3(256), 0, s, src, dst, R, C, lds, ldd, (float*)nullptr, crows);
        else PV_LAUNCH((pv_transpose_kernel<false, false>), grid, dim3(256), 0, s, src, dst, R, C, lds, ldd, (float*)nullptr, crows);
    }
    return pv_check_launch();
}

// Column sums, stage 1: a workgroup owns a chunk of `crows` rows (1024; 64 for short matrices, which would otherwise fill a tenth of the
// chip) x 512-column (bf16: 8 per lane) / 256-column (fp32: 4 per lane) strip; its 4 waves interleave the rows with 16-byte loads and
// combine through LDS into ws[chunk][C].  Stage 2 sums the chunks: a workgroup per 64 columns, 4 waves striding the chunk list.
static inline int64_t pv_colsum_chunk_rows(int64_t R) { return R <= 65536 ? 64 : 1024; }

template <bool BF16>
__global__ __launch_bounds__(256) void pv_colsum_kernel(const void* __restrict__ src, float* __restrict__ ws, int64_t R, int C, int crows) {
    constexpr int VW = BF16 ? 8 : 4;
    __shared__ float red[4][64 * VW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * VW;
    const int64_t r0 = (int64_t)blockIdx.y * crows, r1 = r0 + crows < R ? r0 + crows : R;
    float acc[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) acc[k] = 0.f;
    if (c < C) {
#pragma unroll 4
        for (int64_t r = r0 + wave; r < r1; r += 4) {
            if (BF16) {
                const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(src) + r * C + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc[2 * k] += pv_unpack_lo(w[k]);
                    acc[2 * k + 1] += pv_unpack_hi(w[k]);
                }
            } else {
                const float4 w = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src) + r * C + c);
                acc[0] += w.x; acc[1] += w.y; acc[2] += w.z; acc[3] += w.w;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VW; ++k) red[wave][lane * VW + k] = acc[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * VW; e += 256) {
        const int cc = blockIdx.x * 64 * VW + e;
        if (cc < C) ws[(int64_t)blockIdx.y * C + cc] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    }
}

__global__ __launch_bounds__(256) void pv_colsum_stage2_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t chunks, int C, int accumulate) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (c < C) {
        // eight independent loads in flight per lane: the chunk list is up to ~400 long and a dependent chain of L2 round trips paced this
        // kernel (43 us for 19 MB at r2's first profile)
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int64_t t = wave;
        for (; t + 28 < chunks; t += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += ws[(t + 4 * u) * C + c];
        }
        for (; t < chunks; t += 4) a[0] += ws[t * C + c];
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C) {
        const float v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        out[c] = accumulate ? out[c] + v : v;
    }
}

extern "C" int pv_colsum_f32(const void* src, int src_is_bf16, float* out, float* ws, int64_t R, int64_t C, int accumulate, void* stream) {
    if (!src || !out || !ws || R <= 0 || C <= 0) return PV_ERR_INVALID_ARG;
    const int vw = src_is_bf16 ? 8 : 4;
    if (C % vw || ((uintptr_t)src & 15) || C > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    const int64_t crows = pv_colsum_chunk_rows(R);
    const int64_t chunks = (R + crows - 1) / crows;
    if (chunks > 65535) return PV_ERR_UNSUPPORTED;
    dim3 grid((unsigned)((C / vw + 63) / 64), (unsigned)chunks);
    if (src_is_bf16) PV_LAUNCH(pv_colsum_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, ws, R, (int)C, (int)crows);
    else PV_LAUNCH(pv_colsum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, ws, R, (int)C, (int)crows);
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, (hipStream_t)stream, ws, out, chunks, (int)C, accumulate);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// token prologue: special rows (+pos) and the optional budget token row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_token_prologue_kernel(float* __restrict__ tokens, const float* __restrict__ special,
                                                                const float* __restrict__ pos, const float* __restrict__ btok, float budget,
                                                                int64_t B, int64_t S, int D, int n_special) {
    const int rows_per_img = n_special + (btok ? 1 : 0);
    const int64_t total = B * rows_per_img * (int64_t)D;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        int d = (int)(idx % D);
        int64_t r = idx / D;
        int64_t b = r / rows_per_img;
        int j = (int)(r - b * rows_per_img);
        if (j < n_special)
            tokens[(b * S + j) * D + d] = special[(int64_t)j * D + d] + pos[(int64_t)j * D + d];
        else
            tokens[(b * S + (S - 1)) * D + d] = btok[d] * budget;
    }
}

extern "C" int pv_token_prologue(float* tokens, const float* special, const float* pos, const float* budget_token, float budget,
                                 int64_t B, int64_t S_total, int64_t D, int64_t n_special, void* stream) {
    if (!tokens || !special || !pos || B <= 0 || S_total <= 0 || D <= 0 || n_special < 0 || n_special > S_total) return PV_ERR_INVALID_ARG;
    const int64_t work = B * (n_special + (budget_token ? 1 : 0)) * D;
    if (work == 0) return PV_OK;
    PV_LAUNCH(pv_token_prologue_kernel, dim3(pv_stream_grid(work, 256)), dim3(256), 0, (hipStream_t)stream, tokens, special, pos,
                       budget_token, budget, B, S_total, (int)D, (int)n_special);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// LayerNorm (one wave per row; the row stays in registers: two-pass mean / variance in fp32)
// ------------------------------------------------------------------------------------------------
template <int NCH, bool SPLIT = false>
__global__ __launch_bounds__(256) void pv_layernorm_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ row_scale,
                                                           uint16_t* __restrict__ out, int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + row * ldx, nvec, lane);
        pv_ln_row<NCH>(r, gamma, beta, D, nvec, lane, eps);
        const float sc = row_scale ? row_scale[row] : 1.0f;
        if constexpr (!SPLIT) {
            pv_store_row16_scaled<NCH>(out + row * (int64_t)D, r, sc, nvec, lane);
        } else {          // [hi | lo | hi] rows of 3D
            u32x2* o = reinterpret_cast<u32x2*>(out + row * (int64_t)D * 3);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                int idx = lane + 64 * j;
                if (idx < nvec) {
                    u32x2 hi, lo;
                    { const PvHiLo t_ = pv_split2(r.v[j].x * sc, r.v[j].y * sc); hi[0] = t_.hi; lo[0] = t_.lo; }
                    { const PvHiLo t_ = pv_split2(r.v[j].z * sc, r.v[j].w * sc); hi[1] = t_.hi; lo[1] = t_.lo; }
                    o[idx] = hi;
                    o[idx + nvec] = lo;
                    o[idx + 2 * nvec] = hi;
                }
            }
        }
    }
}

extern "C" int pv_layernorm_split_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* row_scale, uint16_t* out,
                                       int64_t rows, int64_t D, float eps, void* stream) {
    if (!x || !gamma || !beta || !out || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    if (ldx % 4 || ldx < D || ((uintptr_t)x & 15) || ((uintptr_t)out & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return PV_ERR_INVALID_ARG;
    dim3 grid(pv_stream_grid(rows, 4));
#define LNS_LAUNCH(N) PV_LAUNCH((pv_layernorm_kernel<N, true>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta, row_scale, out, rows, (int)D, eps)
    PV_DISPATCH_NCH(D, LNS_LAUNCH);
#undef LNS_LAUNCH
    return pv_check_launch();
}

extern "C" int pv_layernorm_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* row_scale, uint16_t* out,
                                 int64_t rows, int64_t D, float eps, void* stream) {
    if (!x || !gamma || !beta || !out || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    if (ldx % 4 || ldx < D || ((uintptr_t)x & 15) || ((uintptr_t)out & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return PV_ERR_INVALID_ARG;
    dim3 grid(pv_stream_grid(rows, 4));
#define LN_LAUNCH(N) PV_LAUNCH(pv_layernorm_kernel<N>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta, row_scale, out, rows, (int)D, eps)
    PV_DISPATCH_NCH(D, LN_LAUNCH);
#undef LN_LAUNCH
    return pv_check_launch();
}

extern "C" int pv_sum_slices_add_ln_f32(const float* partials, const float* base, float* out, int64_t rows, int64_t D, int64_t slices, const float* gamma,
                                        const float* beta, float eps, uint16_t* ln_out, void* stream) {
    if (!partials || !base || !out || !gamma || !beta || !ln_out || rows <= 0 || D <= 0 || slices <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)partials | (uintptr_t)base | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) & 15 || ((uintptr_t)ln_out & 7)) return PV_ERR_INVALID_ARG;
    dim3 grid(pv_stream_grid(rows, 4));
#define SSL_LAUNCH(N) PV_LAUNCH(pv_sum_slices_ln_kernel<N>, grid, dim3(256), 0, (hipStream_t)stream, partials, base, out, rows, (int)D, (int)slices, gamma, beta, eps, ln_out)
    PV_DISPATCH_NCH(D, SSL_LAUNCH);
#undef SSL_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward (models/blocks.py:60,77 under loss.backward()): y = xhat * gamma + beta, xhat = (x - mean) * rstd
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma;   dres_out = dres_in + dx   (x also feeds the skip)
//   dgamma = sum_rows dy * xhat, dbeta = sum_rows dy:  per-lane column accumulators over the rows a wave walks, combined per
//   block through LDS into ws[block][2][D]; pv_sum_slices_f32 finishes the reduction.  Statistics are recomputed from x.
// ------------------------------------------------------------------------------------------------
// MASKED (ResidualViT, models/residualvit.py:249-260 under loss.backward()): the forward was y = m[row] * (xhat * gamma + beta).
//   dmask[row] (+)= sum_d dy * (xhat * gamma + beta)  [+ sum_d dx_out * u  when the branch output u is given: x1 = x + m * u]
//   then dy <- m * dy and everything proceeds as in the plain case; the 16-bit copy of dx_out can be written scaled by m (the
//   gradient of the branch output u), and the third column-sum plane is taken of exactly that copy.
// SUM (pv_layernorm_bwd_sum, include/peekvit_hip_pct_block.h: a block whose residual is the LayerNorm OUTPUT): the incoming gradient is
//   dy = float(dy) + dy32, formed in fp32 and never rounded; either term may be null.  Nothing else changes.
// SUM with SCALED (pv_layernorm_bwd_sum_masked, include/peekvit_hip_rank_train.h): the forward was y = m[row] * LN(x) with a constant m, so that sum is
//   multiplied by row_scale[row]; a row with m = 0 gives dx = 0 and adds nothing to dgamma / dbeta, m = 1 changes no bit.
template <int NCH, bool MASKED, bool SUM = false, bool SCALED = false>
__global__ __launch_bounds__(256) void pv_layernorm_bwd_kernel(const float* __restrict__ x, const uint16_t* __restrict__ dy,
                                                               const float* __restrict__ gamma, const float* __restrict__ dres_in,
                                                               float* __restrict__ dx_out, uint16_t* __restrict__ dx_bf16, float* __restrict__ ws,
                                                               int64_t rows, int D, float eps, const float* __restrict__ beta,
                                                               const float* __restrict__ row_scale, float* __restrict__ dmask,
                                                               const uint16_t* __restrict__ u, int scale_copy, int dmask_accumulate,
                                                               const uint16_t* __restrict__ dres16 = nullptr, const float* __restrict__ dy32 = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    float4 ag[NCH], ab[NCH], ac[NCH], gm[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        ag[j] = make_float4(0.f, 0.f, 0.f, 0.f); ab[j] = ag[j]; ac[j] = ag[j];
        const int idx = lane + 64 * j;
        gm[j] = idx < nvec ? reinterpret_cast<const float4*>(gamma)[idx] : ag[j];
    }
    const float invD = 1.0f / (float)D;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + row * D, nvec, lane);
        float4 d[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            u32x2 w = {0u, 0u};
            if (idx < nvec && (!SUM || dy)) w = reinterpret_cast<const u32x2*>(dy + row * D)[idx];
            d[j] = make_float4(pv_unpack_lo(w[0]), pv_unpack_hi(w[0]),
                               pv_unpack_lo(w[1]), pv_unpack_hi(w[1]));
            if constexpr (SUM) {
                if (dy32 && idx < nvec) {
                    const float4 t = reinterpret_cast<const float4*>(dy32 + row * D)[idx];
                    d[j].x += t.x; d[j].y += t.y; d[j].z += t.z; d[j].w += t.w;
                }
                if constexpr (SCALED) {
                    const float sc = row_scale[row];
                    d[j].x *= sc; d[j].y *= sc; d[j].z *= sc; d[j].w *= sc;
                }
            }
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) s += (r.v[j].x + r.v[j].y) + (r.v[j].z + r.v[j].w);
        const float mean = pv_wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (lane + 64 * j < nvec) {
                const float a = r.v[j].x - mean, b = r.v[j].y - mean, c = r.v[j].z - mean, e = r.v[j].w - mean;
                q += (a * a + b * b) + (c * c + e * e);
            }
        const float rstd = 1.0f / sqrtf(pv_wave_sum(q) * invD + eps);
        float s1 = 0.f, s2 = 0.f, mdot = 0.f;
        const float msk = MASKED ? row_scale[row] : 1.0f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (lane + 64 * j < nvec) {
                float4& v = r.v[j];                                          // v <- xhat
                v.x = (v.x - mean) * rstd; v.y = (v.y - mean) * rstd; v.z = (v.z - mean) * rstd; v.w = (v.w - mean) * rstd;
                if (MASKED) {
                    const float4 bt = reinterpret_cast<const float4*>(beta)[lane + 64 * j];
                    mdot += (d[j].x * fmaf(v.x, gm[j].x, bt.x) + d[j].y * fmaf(v.y, gm[j].y, bt.y)) +
                            (d[j].z * fmaf(v.z, gm[j].z, bt.z) + d[j].w * fmaf(v.w, gm[j].w, bt.w));
                    d[j].x *= msk; d[j].y *= msk; d[j].z *= msk; d[j].w *= msk;
                }
                ag[j].x += d[j].x * v.x; ag[j].y += d[j].y * v.y; ag[j].z += d[j].z * v.z; ag[j].w += d[j].w * v.w;
                ab[j].x += d[j].x; ab[j].y += d[j].y; ab[j].z += d[j].z; ab[j].w += d[j].w;
                d[j].x *= gm[j].x; d[j].y *= gm[j].y; d[j].z *= gm[j].z; d[j].w *= gm[j].w;     // d <- g
                s1 += (d[j].x + d[j].y) + (d[j].z + d[j].w);
                s2 += (d[j].x * v.x + d[j].y * v.y) + (d[j].z * v.z + d[j].w * v.w);
            }
        s1 = pv_wave_sum(s1) * invD;
        s2 = pv_wave_sum(s2) * invD;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) {
                float4 o = dres_in ? reinterpret_cast<const float4*>(dres_in + row * D)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
                if (!MASKED && dres16) {           // the residual gradient handed over in 16 bits (pv_layernorm_bwd16)
                    const u32x2 rw = reinterpret_cast<const u32x2*>(dres16 + row * D)[idx];
                    o = make_float4(pv_unpack_lo(rw[0]), pv_unpack_hi(rw[0]), pv_unpack_lo(rw[1]), pv_unpack_hi(rw[1]));
                }
                o.x += rstd * (d[j].x - s1 - r.v[j].x * s2);
                o.y += rstd * (d[j].y - s1 - r.v[j].y * s2);
                o.z += rstd * (d[j].z - s1 - r.v[j].z * s2);
                o.w += rstd * (d[j].w - s1 - r.v[j].w * s2);
                if (MASKED || dx_out) reinterpret_cast<float4*>(dx_out + row * D)[idx] = o;
                if (MASKED && u) {
                    const u32x2 uw = reinterpret_cast<const u32x2*>(u + row * D)[idx];
                    mdot += (o.x * pv_unpack_lo(uw[0]) + o.y * pv_unpack_hi(uw[0])) + (o.z * pv_unpack_lo(uw[1]) + o.w * pv_unpack_hi(uw[1]));
                }
                if (dx_bf16) {
                    const float cs_ = (MASKED && scale_copy) ? msk : 1.0f;
                    const u32x2 pk = {pv_pack_bf16x2(o.x * cs_, o.y * cs_), pv_pack_bf16x2(o.z * cs_, o.w * cs_)};
                    reinterpret_cast<u32x2*>(dx_bf16 + row * D)[idx] = pk;
                    // column sums of the bf16 values the downstream GEMMs consume (their bias gradient)
                    ac[j].x += pv_unpack_lo(pk[0]); ac[j].y += pv_unpack_hi(pk[0]);
                    ac[j].z += pv_unpack_lo(pk[1]); ac[j].w += pv_unpack_hi(pk[1]);
                } else {
                    ac[j].x += o.x; ac[j].y += o.y; ac[j].z += o.z; ac[j].w += o.w;
                }
            }
        }
        if (MASKED) {
            mdot = pv_wave_sum(mdot);
            if (lane == 0) dmask[row] = dmask_accumulate ? dmask[row] + mdot : mdot;
        }
    }
    // per-block partial sums through LDS: ws[block][3][D] (dgamma, dbeta, colsum dx); pv_colsum stage 2 adds the blocks up
    __shared__ float red[4][3][NCH * 256];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        reinterpret_cast<float4*>(red[wave][0])[lane + 64 * j] = ag[j];
        reinterpret_cast<float4*>(red[wave][1])[lane + 64 * j] = ab[j];
        reinterpret_cast<float4*>(red[wave][2])[lane + 64 * j] = ac[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * D; e += 256) {
        const int which = e / D, c = e - which * D;
        ws[(int64_t)blockIdx.x * 3 * D + e] = (red[0][which][c] + red[1][which][c]) + (red[2][which][c] + red[3][which][c]);
    }
}

__global__ __launch_bounds__(256) void pv_colsum_stage2_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t chunks, int C, int accumulate);

extern "C" int pv_layernorm_bwd(const float* x, const uint16_t* dy, const float* gamma, const float* dres_in, float* dx_out,
                                uint16_t* dx_bf16, float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate, void* stream) {
    if (!x || !dy || !gamma || !dx_out || !dgb || !ws || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)dx_out & 15) || ((uintptr_t)dgb & 15) ||
        ((uintptr_t)ws & 15) || (dres_in && ((uintptr_t)dres_in & 15)) || (dx_bf16 && ((uintptr_t)dx_bf16 & 7))) return PV_ERR_INVALID_ARG;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (ws_floats < blocks * 3 * D) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)blocks);
#define LNB_LAUNCH(N) PV_LAUNCH((pv_layernorm_bwd_kernel<N, false>), grid, dim3(256), 0, (hipStream_t)stream, x, dy, gamma, dres_in, dx_out, dx_bf16, ws, rows, (int)D, eps, \
                                (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (const uint16_t*)nullptr, 0, 0)
    { int nch_ = (int)((D / 4 + 63) / 64); if (nch_ <= 1) { LNB_LAUNCH(1); } else if (nch_ == 2) { LNB_LAUNCH(2); } else if (nch_ == 3) { LNB_LAUNCH(3); } else { LNB_LAUNCH(4); } }
#undef LNB_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((3 * D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dgb, blocks, (int)(3 * D), accumulate);
    return pv_check_launch();
}

// The same backward with the residual gradient travelling in 16 bits between the two LayerNorms of a block (round 5, an OPTION of the training
// path): dres16 (optional) replaces the fp32 dres_in, and dx_out may be NULL when only the 16-bit copy dx_bf16 is wanted.
extern "C" int pv_layernorm_bwd16(const float* x, const uint16_t* dy, const float* gamma, const float* dres_in, const uint16_t* dres16, float* dx_out,
                                  uint16_t* dx_bf16, float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate, void* stream) {
    if (!x || !dy || !gamma || (!dx_out && !dx_bf16) || !dgb || !ws || rows <= 0 || D <= 0 || (dres_in && dres16)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 7) || ((uintptr_t)gamma & 15) || (dx_out && ((uintptr_t)dx_out & 15)) || ((uintptr_t)dgb & 15) ||
        ((uintptr_t)ws & 15) || (dres_in && ((uintptr_t)dres_in & 15)) || (dres16 && ((uintptr_t)dres16 & 7)) || (dx_bf16 && ((uintptr_t)dx_bf16 & 7))) return PV_ERR_INVALID_ARG;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (ws_floats < blocks * 3 * D) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)blocks);
#define LNB_LAUNCH(N) PV_LAUNCH((pv_layernorm_bwd_kernel<N, false>), grid, dim3(256), 0, (hipStream_t)stream, x, dy, gamma, dres_in, dx_out, dx_bf16, ws, rows, (int)D, eps, \
                                (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (const uint16_t*)nullptr, 0, 0, dres16)
    { int nch_ = (int)((D / 4 + 63) / 64); if (nch_ <= 1) { LNB_LAUNCH(1); } else if (nch_ == 2) { LNB_LAUNCH(2); } else if (nch_ == 3) { LNB_LAUNCH(3); } else { LNB_LAUNCH(4); } }
#undef LNB_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((3 * D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dgb, blocks, (int)(3 * D), accumulate);
    return pv_check_launch();
}

// The same backward for a gradient that arrives as a sum of a 16-bit and an fp32 term (include/peekvit_hip_pct_block.h): the SUM instantiation.
extern "C" int pv_layernorm_bwd_sum(const float* x, const uint16_t* dy16, const float* dy32, const float* gamma, float* dx_out, uint16_t* dx16,
                                    float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate, void* stream) {
    if (!x || (!dy16 && !dy32) || !gamma || (!dx_out && !dx16) || !dgb || !ws || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy16 & 7) || ((uintptr_t)dy32 & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)dx_out & 15) ||
        ((uintptr_t)dx16 & 7) || ((uintptr_t)dgb & 15) || ((uintptr_t)ws & 15)) return PV_ERR_INVALID_ARG;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (ws_floats < blocks * 3 * D) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)blocks);
#define LNS_LAUNCH(N) PV_LAUNCH((pv_layernorm_bwd_kernel<N, false, true>), grid, dim3(256), 0, (hipStream_t)stream, x, dy16, gamma, (const float*)nullptr, dx_out, dx16, ws, rows, \
                                (int)D, eps, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (const uint16_t*)nullptr, 0, 0, (const uint16_t*)nullptr, dy32)
    { int nch_ = (int)((D / 4 + 63) / 64); if (nch_ <= 1) { LNS_LAUNCH(1); } else if (nch_ == 2) { LNS_LAUNCH(2); } else if (nch_ == 3) { LNS_LAUNCH(3); } else { LNS_LAUNCH(4); } }
#undef LNS_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((3 * D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dgb, blocks, (int)(3 * D), accumulate);
    return pv_check_launch();
}

// pv_layernorm_bwd_sum for y = row_scale[row] * LN(x) (include/peekvit_hip_rank_train.h): the SUM + SCALED instantiation.
extern "C" int pv_layernorm_bwd_sum_masked(const float* x, const uint16_t* dy16, const float* dy32, const float* gamma, const float* row_scale, float* dx_out,
                                           uint16_t* dx16, float* dgb, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps, int accumulate,
                                           void* stream) {
    if (!x || (!dy16 && !dy32) || !gamma || !row_scale || (!dx_out && !dx16) || !dgb || !ws || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy16 & 7) || ((uintptr_t)dy32 & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)row_scale & 3) || ((uintptr_t)dx_out & 15) ||
        ((uintptr_t)dx16 & 7) || ((uintptr_t)dgb & 15) || ((uintptr_t)ws & 15)) return PV_ERR_INVALID_ARG;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (ws_floats < blocks * 3 * D) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)blocks);
#define LNSM_LAUNCH(N) PV_LAUNCH((pv_layernorm_bwd_kernel<N, false, true, true>), grid, dim3(256), 0, (hipStream_t)stream, x, dy16, gamma, (const float*)nullptr, dx_out, dx16, ws, \
                                 rows, (int)D, eps, (const float*)nullptr, row_scale, (float*)nullptr, (const uint16_t*)nullptr, 0, 0, (const uint16_t*)nullptr, dy32)
    { int nch_ = (int)((D / 4 + 63) / 64); if (nch_ <= 1) { LNSM_LAUNCH(1); } else if (nch_ == 2) { LNSM_LAUNCH(2); } else if (nch_ == 3) { LNSM_LAUNCH(3); } else { LNSM_LAUNCH(4); } }
#undef LNSM_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((3 * D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dgb, blocks, (int)(3 * D), accumulate);
    return pv_check_launch();
}

extern "C" int pv_layernorm_bwd_masked(const float* x, const uint16_t* dy, const float* gamma, const float* beta, const float* row_scale,
                                       const float* dres_in, const uint16_t* u, float* dx_out, uint16_t* dx_bf16, int scale_copy, float* dgb,
                                       float* dmask, int dmask_accumulate, float* ws, int64_t ws_floats, int64_t rows, int64_t D, float eps,
                                       void* stream) {
    if (!x || !dy || !gamma || !beta || !row_scale || !dx_out || !dgb || !dmask || !ws || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 1024) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) || ((uintptr_t)dx_out & 15) ||
        ((uintptr_t)dgb & 15) || ((uintptr_t)ws & 15) || (dres_in && ((uintptr_t)dres_in & 15)) || (dx_bf16 && ((uintptr_t)dx_bf16 & 7)) ||
        (u && ((uintptr_t)u & 7))) return PV_ERR_INVALID_ARG;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (ws_floats < blocks * 3 * D) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)blocks);
#define LNM_LAUNCH(N) PV_LAUNCH((pv_layernorm_bwd_kernel<N, true>), grid, dim3(256), 0, (hipStream_t)stream, x, dy, gamma, dres_in, dx_out, dx_bf16, ws, rows, (int)D, eps, \
                                beta, row_scale, dmask, u, scale_copy, dmask_accumulate)
    { int nch_ = (int)((D / 4 + 63) / 64); if (nch_ <= 1) { LNM_LAUNCH(1); } else if (nch_ == 2) { LNM_LAUNCH(2); } else if (nch_ == 3) { LNM_LAUNCH(3); } else { LNM_LAUNCH(4); } }
#undef LNM_LAUNCH
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_colsum_stage2_kernel, dim3((unsigned)((3 * D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dgb, blocks, (int)(3 * D), 0);
    return pv_check_launch();
}

// x1 = x + m[row] * u  (fp32 residual stream, 16-bit branch output): the masked residual add of the ResidualViT training forward
__global__ __launch_bounds__(256) void pv_masked_residual_kernel(const float* __restrict__ x, const uint16_t* __restrict__ u, const float* __restrict__ m,
                                                                 float* __restrict__ out, int64_t rows, int D) {
    const int nvec = D >> 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * nvec; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / nvec;
        const float s = m[row];
        const float4 xv = reinterpret_cast<const float4*>(x)[e];
        const u32x2 uw = reinterpret_cast<const u32x2*>(u)[e];
        reinterpret_cast<float4*>(out)[e] = make_float4(fmaf(s, pv_unpack_lo(uw[0]), xv.x), fmaf(s, pv_unpack_hi(uw[0]), xv.y),
                                                        fmaf(s, pv_unpack_lo(uw[1]), xv.z), fmaf(s, pv_unpack_hi(uw[1]), xv.w));
    }
}

extern "C" int pv_masked_residual(const float* x, const uint16_t* u, const float* row_scale, float* out, int64_t rows, int64_t D, void* stream) {
    if (!x || !u || !row_scale || !out || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || ((uintptr_t)x & 15) || ((uintptr_t)u & 7) || ((uintptr_t)out & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_masked_residual_kernel, dim3(pv_stream_grid(rows * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, x, u, row_scale, out, rows, (int)D);
    return pv_check_launch();
}

// LayerNorm folding: per-row (mean, rstd) from the (sum, sum of squares) partials the producer GEMM wrote per column tile.
// Guard (ABI v7, bit 2 of the operand-range flag): folding rounds the RAW row to 16 bits instead of the normalised one, so a row whose
// mean is large against its spread loses the spread - the operand noise of the consumer GEMM grows by sqrt(1 + (mean / std)^2), and
// E[x^2] - mean^2 itself cancels in fp32 beyond mean / std ~ 1e3.  Rows with |mean| * rstd > PV_FOLD_MEAN_LIMIT raise the flag and the
// caller repeats the forward with the LayerNorm applied before the rounding (engine.run_guarded).
#define PV_FOLD_MEAN_LIMIT 1.0f
__global__ __launch_bounds__(256) void pv_rowstat_finalize_kernel(const float* __restrict__ part, float* __restrict__ stat, int tiles, int64_t rows,
                                                                  float invD, float eps, uint32_t* flag) {
    bool risky = false;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
        float s = 0.f, q = 0.f;
        for (int t = 0; t < tiles; ++t) {
            const float2 v = *reinterpret_cast<const float2*>(part + ((int64_t)t * rows + r) * 2);
            s += v.x; q += v.y;
        }
        const float mean = s * invD;
        const float var = fmaxf(q * invD - mean * mean, 0.f);
        const float rstd = 1.0f / sqrtf(var + eps);
        *reinterpret_cast<float2*>(stat + 2 * r) = make_float2(mean, rstd);
        risky |= !(fabsf(mean) * rstd <= PV_FOLD_MEAN_LIMIT);
    }
    if (flag != nullptr && risky) atomicOr(flag, 2u);
}

extern "C" int pv_rowstat_finalize(const float* partials, float* stat, int64_t tiles, int64_t rows, int64_t D, float eps, uint32_t* range_flag, void* stream) {
    if (!partials || !stat || tiles <= 0 || rows <= 0 || D <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)partials & 7) || ((uintptr_t)stat & 7) || ((uintptr_t)range_flag & 3)) return PV_ERR_INVALID_ARG;
    PV_LAUNCH(pv_rowstat_finalize_kernel, dim3(pv_stream_grid(rows, 256)), dim3(256), 0, (hipStream_t)stream, partials, stat, (int)tiles, rows,
              1.0f / (float)D, eps, range_flag);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// GELU forward / backward on bf16 streams for the training path (models/blocks.py:82): g = gelu(pre);
// dpre = dg * (Phi(pre) + pre * phi(pre)), exact erf form.
// ------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void pv_gelu_kernel(const uint16_t* __restrict__ pre, const uint16_t* __restrict__ dg, uint16_t* __restrict__ out, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const u32x4 pw = reinterpret_cast<const u32x4*>(pre)[i];
        u32x4 gw = {0u, 0u, 0u, 0u};
        if (BWD) gw = reinterpret_cast<const u32x4*>(dg)[i];
        u32x4 ow;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x0 = pv_unpack_lo(pw[k]), x1 = pv_unpack_hi(pw[k]);
            float y0, y1;
            if (BWD) {
                const float g0 = pv_unpack_lo(gw[k]), g1 = pv_unpack_hi(gw[k]);
                y0 = g0 * (0.5f * (1.0f + erff(x0 * 0.70710678118654752440f)) + x0 * 0.3989422804014327f * __expf(-0.5f * x0 * x0));
                y1 = g1 * (0.5f * (1.0f + erff(x1 * 0.70710678118654752440f)) + x1 * 0.3989422804014327f * __expf(-0.5f * x1 * x1));
            } else {
                y0 = pv_gelu_erf(x0); y1 = pv_gelu_erf(x1);
            }
            ow[k] = pv_pack_bf16x2(y0, y1);
        }
        reinterpret_cast<u32x4*>(out)[i] = ow;
    }
}

extern "C" int pv_gelu_bf16(const uint16_t* pre, uint16_t* out, int64_t n, void* stream) {
    if (!pre || !out || n <= 0) return PV_ERR_INVALID_ARG;
    if (n % 8 || ((uintptr_t)pre & 15) || ((uintptr_t)out & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_gelu_kernel<false>, dim3(pv_stream_grid(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, pre, (const uint16_t*)nullptr, out, n / 8);
    return pv_check_launch();
}

extern "C" int pv_gelu_bwd_bf16(const uint16_t* pre, const uint16_t* dg, uint16_t* dpre, int64_t n, void* stream) {
    if (!pre || !dg || !dpre || n <= 0) return PV_ERR_INVALID_ARG;
    if (n % 8 || ((uintptr_t)pre & 15) || ((uintptr_t)dg & 15) || ((uintptr_t)dpre & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_gelu_kernel<true>, dim3(pv_stream_grid(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, pre, dg, dpre, n / 8);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// final LayerNorm on class-token rows + sum over class tokens (models/vit.py:95,242-243)
// ------------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void pv_cls_pool_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ pooled, int64_t B, int64_t S, int D, int num_cls, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        RowRegs<NCH> acc;
#pragma unroll
        for (int j = 0; j < NCH; ++j) acc.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < num_cls; ++c) {
            RowRegs<NCH> r;
            pv_load_row<NCH>(r, x + (b * S + c) * (int64_t)D, nvec, lane);
            pv_ln_row<NCH>(r, gamma, beta, D, nvec, lane, eps);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                acc.v[j].x += r.v[j].x; acc.v[j].y += r.v[j].y; acc.v[j].z += r.v[j].z; acc.v[j].w += r.v[j].w;
            }
        }
        pv_store_row<NCH>(pooled + b * (int64_t)D, acc, nvec, lane);
    }
}

extern "C" int pv_cls_pool(const float* x, const float* gamma, const float* beta, float* pooled, int64_t B, int64_t S, int64_t D,
                           int64_t num_cls, float eps, void* stream) {
    if (!x || !gamma || !beta || !pooled || B <= 0 || S <= 0 || D <= 0 || num_cls <= 0 || num_cls > S) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    dim3 grid(pv_stream_grid(B, 4));
#define CP_LAUNCH(N) PV_LAUNCH(pv_cls_pool_kernel<N>, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, pooled, B, S, (int)D, (int)num_cls, eps)
    PV_DISPATCH_NCH(D, CP_LAUNCH);
#undef CP_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// fp32 classification head: logits[B,C] = pooled[B,D] . w[C,D]^T + bias   (LDS-tiled, 64x64 tile)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_head_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int B, int D, int C) {
    // Round 6: 32 x 64 tiles (rounds 1-5: 64 x 64 - 128 workgroups for 512 x 1000 logits, half of the CUs idle and the others bound by their fp32
    // FMAs: 44 us at vit_small's batch), 32-column K steps with the NEXT step's rows already in registers while this one is multiplied.
    // Per logit: a fused multiply-add chain over each 32-column K step (k ascending), the step sums added in order - a single fp32 chain over
    // D = 768 lost ~1e-6 of a logit (tests/test_hip_entry_points.py::test_head_both_kernels).
    const int m = blockIdx.y * PV_HEAD_TM + pv_head_a_row(threadIdx.x);
    const float* ap = a + (int64_t)(m < B ? m : 0) * D + pv_head_a_col(threadIdx.x);
    pv_head_tile([&](int k0) { return *reinterpret_cast<const float4*>(ap + k0); }, w, bias, out, B, D, C);
}

// Small batches (serving): the tiled kernel above is ceil(C/64) workgroups walking D in 16-column steps (60 us at batch 1, 6 % of a 1 ms forward).
// One THREAD per logit instead, with exactly the tiled kernel's arithmetic (a fused multiply-add chain per 32-column K step, the step sums added
// in order; the tiled kernel's zero padding of a ragged last step adds exact zeros), so an image's logits do not depend on which of the two
// kernels its batch size selects (tests/test_hip_entry_points.py::test_head_both_kernels, tests/test_hip_models.py::test_full_batch_properties_vit_b_16).
__global__ __launch_bounds__(64) void pv_head_small_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int B, int D, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    const float acc = pv_head_dot(reinterpret_cast<const float4*>(a + (int64_t)b * D), reinterpret_cast<const float4*>(w + (int64_t)c * D), D >> 2);
    out[(int64_t)b * C + c] = acc + (bias ? bias[c] : 0.f);
}

extern "C" int pv_head_f32(const float* pooled, const float* w, const float* b, float* logits, int64_t B, int64_t D, int64_t C, void* stream) {
    if (!pooled || !w || !logits || B <= 0 || D <= 0 || C <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || ((uintptr_t)pooled & 15) || ((uintptr_t)w & 15)) return PV_ERR_UNSUPPORTED;
    if (B <= 16) {
        PV_LAUNCH(pv_head_small_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(64), 0, (hipStream_t)stream, pooled, w, b, logits, (int)B, (int)D, (int)C);
        return pv_check_launch();
    }
    dim3 grid((unsigned)((C + 63) / 64), (unsigned)((B + 31) / 32));
    PV_LAUNCH(pv_head_kernel, grid, dim3(256), 0, (hipStream_t)stream, pooled, w, b, logits, (int)B, (int)D, (int)C);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// RankViT: token norms, rank / top-k, compaction gather  (models/rankvit.py:55-77)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_token_norm_kernel(const float* __restrict__ x, float* __restrict__ norms, int64_t B, int64_t S, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t N = S - 1, rows = B * N;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        int64_t b = r / N, i = r - b * N;
        const float4* xr = reinterpret_cast<const float4*>(x + (b * S + 1 + i) * (int64_t)D);
        float s = 0.f;
        for (int idx = lane; idx < nvec; idx += 64) {
            float4 v = xr[idx];
            s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
        s = pv_wave_sum(s);
        if (lane == 0) norms[r] = sqrtf(s);
    }
}

extern "C" int pv_token_norm(const float* x, float* norms, int64_t B, int64_t S, int64_t D, void* stream) {
    if (!x || !norms || B <= 0 || S < 1 || D <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || ((uintptr_t)x & 15)) return PV_ERR_UNSUPPORTED;
    if (S == 1) return PV_OK;
    PV_LAUNCH(pv_token_norm_kernel, dim3(pv_stream_grid(B * (S - 1), 4)), dim3(256), 0, (hipStream_t)stream, x, norms, B, S, (int)D);
    return pv_check_launch();
}

// sortable key: larger float (NaN above +inf, like torch's descending argsort) <=> larger uint32
__device__ __forceinline__ uint32_t pv_sort_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The keep BOUNDARY of an image (round 6): the relative gap between its last kept norm (rank k - 1) and its first dropped one (rank k),
// (n_{k-1} - n_k) / n_{k-1}.  The ranking is a discrete decision on norms that carry the 16-bit layers' noise (~1e-4 relative): an image whose gap is
// of that size may keep another token than the reference's fp32 arithmetic does.  gap_min[b] = min(gap_min[b], gap): the caller fills it with +inf and
// hands the same array to every ranked layer of a forward - what is left is each image's narrowest boundary (peekvit_amd.models.rankvit repairs those
// images in split precision when asked to).  The two threads that own ranks k - 1 and k leave their norms in LDS; thread 0 folds them in.
__device__ __forceinline__ float pv_unsort_key(uint32_t u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ void pv_rank_gap(const uint32_t* edge, float* __restrict__ gap_min, int64_t b, int N, int k) {
    if (gap_min && threadIdx.x == 0 && k < N) {
        const float hi = pv_unsort_key(edge[0]), lo = pv_unsort_key(edge[1]);
        const float gap = hi > 0.f ? (hi - lo) / hi : 0.f;
        if (gap < gap_min[b]) gap_min[b] = gap;          // (one workgroup per image, launches of a forward in stream order: no race)
    }
}

// one workgroup per image: keys in LDS, rank_i = #{j : key_j > key_i or (key_j == key_i and j < i)} (stable descending)
__global__ __launch_bounds__(256) void pv_rank_topk_kernel(const float* __restrict__ norms, int32_t* __restrict__ keep, float* __restrict__ gap_min, int N, int k) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);
    uint32_t* edge = keys + N;                           // [2]: the keys of rank k - 1 and rank k
    const int64_t b = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += 256) keys[i] = pv_sort_key(norms[b * N + i]);
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {
        const uint32_t ki = keys[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            uint32_t kj = keys[j];
            rank += (kj > ki) || (kj == ki && j < i);
        }
        if (rank < k) keep[b * k + rank] = i;
        if (rank == k - 1) edge[0] = ki;
        if (rank == k) edge[1] = ki;
    }
    if (gap_min) { __syncthreads(); pv_rank_gap(edge, gap_min, b, N, k); }
}

extern "C" int pv_rank_topk_gap(const float* norms, int32_t* keep, float* gap_min, int64_t B, int64_t N, int64_t k, void* stream) {
    if (!norms || !keep || B <= 0 || N <= 0 || k < 0 || k > N) return PV_ERR_INVALID_ARG;
    if (N > 4096) return PV_ERR_UNSUPPORTED;
    if (k == 0) return PV_OK;
    PV_LAUNCH(pv_rank_topk_kernel, dim3((unsigned)B), dim3(256), (size_t)(N + 2) * 4, (hipStream_t)stream, norms, keep, gap_min, (int)N, (int)k);
    return pv_check_launch();
}
extern "C" int pv_rank_topk(const float* norms, int32_t* keep, int64_t B, int64_t N, int64_t k, void* stream) {
    return pv_rank_topk_gap(norms, keep, nullptr, B, N, k, stream);
}

// the same ranking with the norms assembled from a producer GEMM's per-column-tile sums of squares (no pass over the tokens)
__global__ __launch_bounds__(256) void pv_rank_topk_partials_kernel(const float* __restrict__ rowsq, int tiles, int64_t rows, int32_t* __restrict__ keep,
                                                                    float* __restrict__ gap_min, int S, int k) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);
    const int64_t b = blockIdx.x;
    const int N = S - 1;
    uint32_t* edge = keys + N;
    for (int i = threadIdx.x; i < N; i += 256) {
        float s = 0.f;
        for (int t = 0; t < tiles; ++t) s += rowsq[(int64_t)t * rows + b * S + 1 + i];
        keys[i] = pv_sort_key(sqrtf(s));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {
        const uint32_t ki = keys[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            uint32_t kj = keys[j];
            rank += (kj > ki) || (kj == ki && j < i);
        }
        if (rank < k) keep[b * k + rank] = i;
        if (rank == k - 1) edge[0] = ki;
        if (rank == k) edge[1] = ki;
    }
    if (gap_min) { __syncthreads(); pv_rank_gap(edge, gap_min, b, N, k); }
}

extern "C" int pv_rank_topk_partials_gap(const float* rowsq, int64_t tiles, int32_t* keep, float* gap_min, int64_t B, int64_t S, int64_t k, void* stream) {
    if (!rowsq || !keep || B <= 0 || S < 2 || tiles <= 0 || k < 0 || k > S - 1) return PV_ERR_INVALID_ARG;
    if (S - 1 > 4096 || tiles > 64) return PV_ERR_UNSUPPORTED;
    if (k == 0) return PV_OK;
    PV_LAUNCH(pv_rank_topk_partials_kernel, dim3((unsigned)B), dim3(256), (size_t)(S + 1) * 4, (hipStream_t)stream, rowsq, (int)tiles, B * S, keep, gap_min,
              (int)S, (int)k);
    return pv_check_launch();
}
extern "C" int pv_rank_topk_partials(const float* rowsq, int64_t tiles, int32_t* keep, int64_t B, int64_t S, int64_t k, void* stream) {
    return pv_rank_topk_partials_gap(rowsq, tiles, keep, nullptr, B, S, k, stream);
}

__global__ __launch_bounds__(256) void pv_gather_tokens_kernel(const float* __restrict__ x, const int32_t* __restrict__ keep, float* __restrict__ out,
                                                               int64_t B, int64_t S_in, int64_t k, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t So = k + 1, rows = B * So;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        int64_t b = r / So, j = r - b * So;
        int64_t srow = j == 0 ? 0 : 1 + (int64_t)keep[b * k + (j - 1)];
        const float4* s = reinterpret_cast<const float4*>(x + (b * S_in + srow) * (int64_t)D);
        float4* d = reinterpret_cast<float4*>(out + r * (int64_t)D);
        for (int idx = lane; idx < nvec; idx += 64) d[idx] = s[idx];
    }
}

extern "C" int pv_gather_tokens(const float* x, const int32_t* keep, float* out, int64_t B, int64_t S_in, int64_t k, int64_t D, void* stream) {
    if (!x || !out || B <= 0 || S_in < 1 || k < 0 || k > S_in - 1 || D <= 0 || (k > 0 && !keep)) return PV_ERR_INVALID_ARG;
    if (D % 4 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_gather_tokens_kernel, dim3(pv_stream_grid(B * (k + 1), 4)), dim3(256), 0, (hipStream_t)stream, x, keep, out, B, S_in, k, (int)D);
    return pv_check_launch();
}

// Backward of the compaction (models/rankvit.py:55-77 under loss.backward()): dx[b, 0] = dy[b, 0], dx[b, 1 + keep[b,i]] = dy[b, 1 + i],
// every dropped row = 0.  One workgroup per image: the inverse map is built in LDS, then every output row is written once.
__global__ __launch_bounds__(256) void pv_scatter_tokens_kernel(const float* __restrict__ dy, const int32_t* __restrict__ keep, float* __restrict__ dx,
                                                                int64_t S_in, int64_t k, int D) {
    extern __shared__ int inv[];                     // inv[n] = position of token n in the kept list, or -1
    const int64_t b = blockIdx.x, N = S_in - 1;
    for (int n = threadIdx.x; n < N; n += 256) inv[n] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += 256) inv[keep[b * k + i]] = i;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    for (int64_t r = wave; r < S_in; r += 4) {
        const int src = r == 0 ? 0 : (inv[r - 1] < 0 ? -1 : 1 + inv[r - 1]);
        float4* d = reinterpret_cast<float4*>(dx + (b * S_in + r) * (int64_t)D);
        if (src < 0) {
            for (int idx = lane; idx < nvec; idx += 64) d[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const float4* sp = reinterpret_cast<const float4*>(dy + (b * (k + 1) + src) * (int64_t)D);
            for (int idx = lane; idx < nvec; idx += 64) d[idx] = sp[idx];
        }
    }
}

extern "C" int pv_scatter_tokens(const float* dy, const int32_t* keep, float* dx, int64_t B, int64_t S_in, int64_t k, int64_t D, void* stream) {
    if (!dy || !dx || B <= 0 || S_in < 1 || k < 0 || k > S_in - 1 || D <= 0 || (k > 0 && !keep)) return PV_ERR_INVALID_ARG;
    if (D % 4 || ((uintptr_t)dy & 15) || ((uintptr_t)dx & 15) || S_in > 16384 || B > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_scatter_tokens_kernel, dim3((unsigned)B), dim3(256), (size_t)S_in * sizeof(int), (hipStream_t)stream, dy, keep, dx, S_in, k, (int)D);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// ResidualViT gate + in-place masking (models/residualvit.py:197-235, eval, sigmoid gate, learnable budget token)
// ------------------------------------------------------------------------------------------------
template <int NCH, bool LN>
__global__ __launch_bounds__(256) void pv_residual_gate_kernel(const float* x, float* xo, const float* __restrict__ wg, const float* __restrict__ bg,
                                                               const float* __restrict__ wb, const float* __restrict__ bb, float temp, float sbias,
                                                               float* __restrict__ mask_out, float* __restrict__ row_scale, float* __restrict__ thr_out,
                                                               const float* __restrict__ ln_gamma, const float* __restrict__ ln_beta, float ln_eps,
                                                               uint16_t* __restrict__ ln_out, int64_t S, int D) {
    __shared__ float thr_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t b = blockIdx.x;
    if (wave == 0) {   // threshold from the budget token (last row), models/residualvit.py:212
        const float s = pv_gate_budget_dot(x + (b * S + S - 1) * (int64_t)D, wb, bb, nvec, lane);
        if (lane == 0) {
            thr_s = pv_sigmoid(s);
            if (thr_out) thr_out[b] = thr_s;
        }
    }
    __syncthreads();
    const float thr = thr_s;
    float4 gm[LN ? NCH : 1], bt[LN ? NCH : 1];
    if constexpr (LN) pv_ln_load_affine<NCH>(gm, bt, ln_gamma, ln_beta, nvec, lane);
    for (int64_t i = wave; i < S; i += 4) {
        const bool special = i == 0 || i == S - 1;          // class token, budget token: pass through, scale 1
        const float* xr = x + (b * S + i) * (int64_t)D;
        float* xw = xo + (b * S + i) * (int64_t)D;
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, xr, nvec, lane);
        float m = 1.0f;
        if (!special) {
            m = pv_gate_mask<NCH>(r, wg, bg, temp, sbias, thr, nvec, lane);
#pragma unroll
            for (int j = 0; j < NCH; ++j) { r.v[j].x *= m; r.v[j].y *= m; r.v[j].z *= m; r.v[j].w *= m; }
        }
        // xo == nullptr: the caller never reads the masked tokens (res_scaled residual + ln_out)
        if (xo != nullptr && (!special || xo != x)) pv_store_row<NCH>(xw, r, nvec, lane);
        if (lane == 0) {
            if (!special) mask_out[b * (S - 2) + i - 1] = m;
            row_scale[b * S + i] = m;
        }
        if constexpr (LN) {      // the block's first LayerNorm on the row just written, times its scale: m * LN1(masked row) (residualvit.py:251)
            pv_ln_row_regs<NCH>(r, gm, bt, D, nvec, lane, ln_eps);
            pv_store_row16_scaled<NCH>(ln_out + (b * S + i) * (int64_t)D, r, m, nvec, lane);
        }
    }
}

extern "C" int pv_residual_gate(const float* x, float* xo, const float* wg, const float* bg, const float* wb, const float* bb, float temp,
                                float sigmoid_bias, float* mask_out, float* row_scale, float* thr_out, const float* ln_gamma, const float* ln_beta,
                                float ln_eps, uint16_t* ln_out, int64_t B, int64_t S, int64_t D, void* stream) {
    if (!x || !wg || !bg || !wb || !bb || !mask_out || !row_scale || B <= 0 || S < 3 || D <= 0 || temp == 0.f) return PV_ERR_INVALID_ARG;
    if (!xo && !ln_out) return PV_ERR_INVALID_ARG;          // without the masked tokens the block needs at least its first LayerNorm from here
    if (D % 4 || D > 4096 || ((uintptr_t)x & 15) || ((uintptr_t)xo & 15) || ((uintptr_t)wg & 15) || ((uintptr_t)wb & 15)) return PV_ERR_UNSUPPORTED;
    if (ln_out && (!ln_gamma || !ln_beta || ((uintptr_t)ln_gamma & 15) || ((uintptr_t)ln_beta & 15) || ((uintptr_t)ln_out & 7))) return PV_ERR_INVALID_ARG;
    dim3 grid((unsigned)B);
#define RG_LAUNCH(N) do { if (ln_out) PV_LAUNCH((pv_residual_gate_kernel<N, true>), grid, dim3(256), 0, (hipStream_t)stream, x, xo, wg, bg, wb, bb, temp, sigmoid_bias, mask_out, row_scale, thr_out, ln_gamma, ln_beta, ln_eps, ln_out, S, (int)D); \
                          else PV_LAUNCH((pv_residual_gate_kernel<N, false>), grid, dim3(256), 0, (hipStream_t)stream, x, xo, wg, bg, wb, bb, temp, sigmoid_bias, mask_out, row_scale, thr_out, ln_gamma, ln_beta, ln_eps, ln_out, S, (int)D); } while (0)
    PV_DISPATCH_NCH(D, RG_LAUNCH);
#undef RG_LAUNCH
    return pv_check_launch();
}

// Backward of pv_residual_gate (loss.backward() through models/residualvit.py:197-235 in training).  G = dL/d(x_out) [B,S,D], dr = dL/d(row_scale)
// [B,S] (the mask gradient of the masked block and of any auxiliary loss on block.mask; entries of the two special rows are ignored):
//   patch row:  dm = dr + G . x;  active = sigmoid(..) > thr;  dz = active ? dm * sg (1 - sg) / temp : 0;  dthr -= active ? dm : 0
//               dx = m G + dz wg;   dwg += dz x;   dbg += dz
//   budget row: du = dthr * thr (1 - thr);  dx = G + du wb;  dwb = du x;  dbb = du        class row: dx = G
// One workgroup per image; a wave keeps x and G of its row in registers, so each is read once.  Parameter gradients leave as per-image
// partials (dwg_part, dwb_part [B,D]; scal_part [B,4] = dbg, dbb, 0, 0) for pv_colsum_f32.
template <int NCH>
__global__ __launch_bounds__(256) void pv_residual_gate_bwd_kernel(const float* __restrict__ x, const float* __restrict__ G, const float* __restrict__ dr,
                                                                   const float* __restrict__ wg, const float* __restrict__ bg, const float* __restrict__ wb,
                                                                   const float* __restrict__ bb, float temp, float sbias, float* __restrict__ dx,
                                                                   float* __restrict__ dwg_part, float* __restrict__ dwb_part, float* __restrict__ scal_part,
                                                                   int64_t S, int D) {
    __shared__ float thr_s, red_s[4][2];
    __shared__ float4 red_w[3][NCH * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t b = blockIdx.x, N = S - 2;
    const float* xb = x + (b * S + S - 1) * (int64_t)D;          // the budget row
    const float4* xb4 = reinterpret_cast<const float4*>(xb);
    if (wave == 0) {
        const float s = pv_gate_budget_dot(xb, wb, bb, nvec, lane);
        if (lane == 0) thr_s = pv_sigmoid(s);
    }
    if (wave == 1) {      // class row: passes through
        const float4* s4 = reinterpret_cast<const float4*>(G + (b * S) * (int64_t)D);
        float4* d4 = reinterpret_cast<float4*>(dx + (b * S) * (int64_t)D);
        for (int idx = lane; idx < nvec; idx += 64) d4[idx] = s4[idx];
    }
    __syncthreads();
    const float thr = thr_s;
    float4 wv[NCH], acc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int idx = lane + 64 * j;
        wv[j] = idx < nvec ? reinterpret_cast<const float4*>(wg)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float dbg = 0.f, dthr = 0.f;
    for (int64_t i = wave; i < N; i += 4) {
        const int64_t row = b * S + 1 + i;
        RowRegs<NCH> r, g;
        pv_load_row<NCH>(r, x + row * (int64_t)D, nvec, lane);
        pv_load_row<NCH>(g, G + row * (int64_t)D, nvec, lane);
        float s = 0.f, a = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            s += (r.v[j].x * wv[j].x + r.v[j].y * wv[j].y) + (r.v[j].z * wv[j].z + r.v[j].w * wv[j].w);
            a += (r.v[j].x * g.v[j].x + r.v[j].y * g.v[j].y) + (r.v[j].z * g.v[j].z + r.v[j].w * g.v[j].w);
        }
        s = pv_wave_sum(s) + bg[0];
        a = pv_wave_sum(a);
        const float t = s / temp + sbias;
        const float sg = pv_sigmoid(t);
        const float m = fmaxf(sg - thr, 0.f);
        const float dm = a + dr[row];
        const bool active = sg - thr > 0.f;
        // sigmoid'(t) = sigmoid(t) sigmoid(-t): with the reference's sigmoid bias of 10 the gate sits at 1 - 5e-5 and "1 - sg" in fp32
        // would carry three digits
        const float dz = active ? dm * sg * pv_sigmoid(-t) / temp : 0.f;
        if (active) dthr -= dm;
        dbg += dz;
        float* dxr = dx + row * (int64_t)D;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) {
                reinterpret_cast<float4*>(dxr)[idx] = make_float4(m * g.v[j].x + dz * wv[j].x, m * g.v[j].y + dz * wv[j].y,
                                                                  m * g.v[j].z + dz * wv[j].z, m * g.v[j].w + dz * wv[j].w);
                acc[j].x += dz * r.v[j].x; acc[j].y += dz * r.v[j].y; acc[j].z += dz * r.v[j].z; acc[j].w += dz * r.v[j].w;
            }
        }
    }
    // combine the four waves: dwg partial of the image, dbg, dthr
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) red_w[wave - 1][lane + 64 * j] = acc[j];
    }
    if (lane == 0) { red_s[wave][0] = dbg; red_s[wave][1] = dthr; }      // every lane of a wave holds the same dbg / dthr
    __syncthreads();
    if (wave == 0) {
        const float dbg_t = (red_s[0][0] + red_s[1][0]) + (red_s[2][0] + red_s[3][0]);
        const float dthr_t = (red_s[0][1] + red_s[1][1]) + (red_s[2][1] + red_s[3][1]);
        const float du = dthr_t * thr * (1.0f - thr);      // the threshold is a mid-range sigmoid (budget ~ 0.1 .. 0.9): no cancellation here
        const float4* g4 = reinterpret_cast<const float4*>(G + (b * S + S - 1) * (int64_t)D);
        float4* d4 = reinterpret_cast<float4*>(dx + (b * S + S - 1) * (int64_t)D);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) {
                const float4 t0 = red_w[0][idx], t1 = red_w[1][idx], t2 = red_w[2][idx];
                reinterpret_cast<float4*>(dwg_part + b * (int64_t)D)[idx] =
                    make_float4(acc[j].x + t0.x + t1.x + t2.x, acc[j].y + t0.y + t1.y + t2.y, acc[j].z + t0.z + t1.z + t2.z, acc[j].w + t0.w + t1.w + t2.w);
                const float4 xv = xb4[idx], gv = g4[idx], w = reinterpret_cast<const float4*>(wb)[idx];
                d4[idx] = make_float4(gv.x + du * w.x, gv.y + du * w.y, gv.z + du * w.z, gv.w + du * w.w);
                reinterpret_cast<float4*>(dwb_part + b * (int64_t)D)[idx] = make_float4(du * xv.x, du * xv.y, du * xv.z, du * xv.w);
            }
        }
        if (lane == 0) { scal_part[b * 4] = dbg_t; scal_part[b * 4 + 1] = du; scal_part[b * 4 + 2] = 0.f; scal_part[b * 4 + 3] = 0.f; }
    }
}

extern "C" int pv_residual_gate_bwd(const float* x, const float* dxo, const float* drow, const float* wg, const float* bg, const float* wb, const float* bb,
                                    float temp, float sigmoid_bias, float* dx, float* dwg_part, float* dwb_part, float* scal_part, int64_t B, int64_t S,
                                    int64_t D, void* stream) {
    if (!x || !dxo || !drow || !wg || !bg || !wb || !bb || !dx || !dwg_part || !dwb_part || !scal_part || B <= 0 || S < 3 || D <= 0 || temp == 0.f)
        return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)dxo | (uintptr_t)dx | (uintptr_t)wg | (uintptr_t)wb | (uintptr_t)dwg_part | (uintptr_t)dwb_part) & 15) return PV_ERR_UNSUPPORTED;
    dim3 grid((unsigned)B);
#define RGB_LAUNCH(N) PV_LAUNCH(pv_residual_gate_bwd_kernel<N>, grid, dim3(256), 0, (hipStream_t)stream, x, dxo, drow, wg, bg, wb, bb, temp, sigmoid_bias, dx, dwg_part, dwb_part, scal_part, S, (int)D)
    PV_DISPATCH_NCH(D, RGB_LAUNCH);
#undef RGB_LAUNCH
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// A-ViT token halting (reference models/adavit.py:158-219) on the PACKED row matrix of the HIP forward: image b is the row segment
// [seg[b], seg[b+1]) of y, its live tokens in original order (pos = token index) and, when nh[b] > 0, one representative row of its
// nh[b] halted tokens last (pos = -1; every halted token of an image has the same block output, so its h counts nh[b] times).
// Three launches: (1) one workgroup per image updates c / R / rho / counter / mask of its live tokens, accumulates the class rows of
// `output`, writes its h sum and the next segment length; (2) one workgroup scans the lengths into the next segment table and the
// totals word; (3) one workgroup per image writes the next packed rows (survivors in order, then a zero representative row).
// ------------------------------------------------------------------------------------------------
#define PV_ACT_MAX_CLS 16

__global__ __launch_bounds__(256) void pv_act_update_kernel(const float* __restrict__ y, int D, const int32_t* __restrict__ seg,
                                                            const int32_t* __restrict__ nh, const int32_t* __restrict__ pos, int S,
                                                            float* __restrict__ c, float* __restrict__ rr, float* __restrict__ rho,
                                                            float* __restrict__ counter, float* __restrict__ mask, float* __restrict__ acc, int nc,
                                                            float* __restrict__ hpart, float gate_scale, float gate_center, float thr, int last,
                                                            int32_t* __restrict__ nh_next, int32_t* __restrict__ len_next) {
    __shared__ float red_h[4];
    __shared__ int red_n[4];
    __shared__ int cls_row[PV_ACT_MAX_CLS];
    __shared__ float cls_w[PV_ACT_MAX_CLS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = seg[b], L = seg[b + 1] - s0, n_h = nh[b];
    if (tid < nc) cls_row[tid] = -1;
    __syncthreads();
    float hsum = 0.f;
    int live = 0;
    for (int i = tid; i < L; i += 256) {
        const int64_t row = s0 + i;
        const int p = pos[row];
        // h = sigmoid(x[:,:,0] * gate_scale - gate_center): two roundings, as the reference's two tensor ops (no contraction)
        const float z = __fsub_rn(__fmul_rn(y[row * D], gate_scale), gate_center);
        const float h = 1.0f / (1.0f + expf(-z));
        if (p < 0) {
            hsum += h * (float)n_h;
            continue;
        }
        hsum += h;
        const int64_t t = (int64_t)b * S + p;
        const float he = last ? 1.0f : h;             // the last layer halts everything (:187), after the real h was recorded
        const float cn = __fadd_rn(c[t], he);
        const float R = rr[t];
        const bool reached = cn > thr, notr = cn < thr;
        c[t] = cn;
        float rh = __fadd_rn(rho[t], 1.0f);
        if (reached) rh = __fadd_rn(rh, R);
        rho[t] = rh;
        if (notr) {
            rr[t] = __fsub_rn(R, he);
            counter[t] = __fadd_rn(counter[t], 1.0f);
            ++live;
        }
        mask[t] = notr ? 1.0f : 0.0f;
        if (p < nc) {
            cls_row[p] = (int)i;
            cls_w[p] = reached ? R : (notr ? he : 0.0f);
        }
    }
    // halting_score_layer partial and the number of tokens still running
    for (int o = 32; o > 0; o >>= 1) {
        hsum += __shfl_xor(hsum, o, 64);
        live += __shfl_xor(live, o, 64);
    }
    if (lane == 0) { red_h[wave] = hsum; red_n[wave] = live; }
    __syncthreads();
    if (tid == 0) {
        hpart[b] = (red_h[0] + red_h[1]) + (red_h[2] + red_h[3]);
        const int n_live = red_n[0] + red_n[1] + red_n[2] + red_n[3];
        if (nh_next) nh_next[b] = S - n_live;
        if (len_next) len_next[b] = n_live + (S - n_live > 0 ? 1 : 0);
    }
    // output += block_out * (R * reached + h * not_reached) on the class rows (the only rows of `output` the logits read)
    for (int e = tid; e < nc * D; e += 256) {
        const int p = e / D, d = e - p * D;
        const int i = cls_row[p];
        if (i < 0) continue;
        float* a = acc + ((int64_t)b * nc + p) * D + d;
        *a = __fadd_rn(*a, __fmul_rn(y[(int64_t)(s0 + i) * D + d], cls_w[p]));
    }
}

__global__ __launch_bounds__(256) void pv_act_compact_kernel(const float* __restrict__ y, int D, const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ pos, int S, const float* __restrict__ mask,
                                                             const int32_t* __restrict__ seg_next, const int32_t* __restrict__ nh_next,
                                                             float* __restrict__ x_next, float* __restrict__ rs_next, int32_t* __restrict__ pos_next) {
    __shared__ int wcount[4];
    __shared__ int src[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = seg[b], L = seg[b + 1] - s0, d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    int p = -1;
    bool keep = false;
    if (tid < L) {
        p = pos[s0 + tid];
        keep = p >= 0 && mask[(int64_t)b * S + p] != 0.0f;
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wcount[w];
    const int nkeep = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    if (keep) {
        const int j = base + before;                  // stable: survivors keep their order
        src[j] = s0 + tid;
        pos_next[d0 + j] = p;
        rs_next[d0 + j] = 1.0f;
    }
    const bool rep = nh_next[b] > 0 && Ln == nkeep + 1;
    if (rep && tid == 0) {
        pos_next[d0 + nkeep] = -1;
        rs_next[d0 + nkeep] = 0.0f;
    }
    __syncthreads();
    const int nvec = D >> 2;
    for (int j = wave; j < nkeep; j += 4) {
        const float4* s = reinterpret_cast<const float4*>(y + (int64_t)src[j] * D);
        float4* d = reinterpret_cast<float4*>(x_next + (int64_t)(d0 + j) * D);
        for (int v = lane; v < nvec; v += 64) d[v] = s[v];
    }
    if (rep && wave == 0) {
        float4* d = reinterpret_cast<float4*>(x_next + (int64_t)(d0 + nkeep) * D);
        for (int v = lane; v < nvec; v += 64) d[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

extern "C" int pv_act_step(const float* y, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, int64_t B, int64_t S, int64_t D,
                           float* c, float* r, float* rho, float* counter, float* mask, float* acc, int64_t num_cls, float* h_part,
                           float gate_scale, float gate_center, float threshold, int last, float* x_next, float* row_scale_next,
                           int32_t* seg_next, int32_t* n_halted_next, int32_t* pos_next, int32_t* totals, void* stream) {
    if (!y || !seg_start || !n_halted || !pos || !c || !r || !rho || !counter || !mask || !acc || !h_part || B <= 0 || S <= 0 || D <= 0)
        return PV_ERR_INVALID_ARG;
    if (!last && (!x_next || !row_scale_next || !seg_next || !n_halted_next || !pos_next || !totals)) return PV_ERR_INVALID_ARG;
    if (num_cls < 1 || num_cls > S) return PV_ERR_INVALID_ARG;
    if (num_cls > PV_ACT_MAX_CLS || S > 256 || D % 4 || B > 0x7fffffff || ((uintptr_t)y & 15) || (x_next && ((uintptr_t)x_next & 15)))
        return PV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    PV_LAUNCH(pv_act_update_kernel, dim3((unsigned)B), dim3(256), 0, s, y, (int)D, seg_start, n_halted, pos, (int)S, c, r, rho, counter, mask, acc,
              (int)num_cls, h_part, gate_scale, gate_center, threshold, last, last ? nullptr : n_halted_next, last ? nullptr : seg_next + 1);
    int rc = pv_check_launch();
    if (rc != PV_OK || last) return rc;
    if ((rc = pv_seg_scan(seg_next, (int)B, totals, s)) != PV_OK) return rc;
    PV_LAUNCH(pv_act_compact_kernel, dim3((unsigned)B), dim3(256), 0, s, y, (int)D, seg_start, pos, (int)S, mask, seg_next, n_halted_next, x_next,
              row_scale_next, pos_next);
    return pv_check_launch();
}
