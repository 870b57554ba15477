// The tile pieces of the streaming attention kernels, shared by the forward body of pv_attention.hip and the backward kernels of
// pv_attention_stream.hip (uniform sequences) and pv_sparse_train.hip (ragged segments with weighted keys): the 64-row staging into a swizzled LDS
// image, the operand fragments straight from global memory and by transposed LDS reads, the packing of two accumulator tiles into one operand, the
// backward's S | dP tile product, and the 16-bit store with the bias partial sums.  Everything is inlined into the including file and compiles under
// that file's flags.
#pragma once
#include "pv_common.h"
#include "pv_attn.h"

constexpr float PV_LOG2E = 1.44269504088896340736f;
constexpr int PV_SB = 64;              // rows per block that passes through the LDS, and per workgroup

// rows [r0, r0 + 64) x the head's DH columns of a 16-bit matrix with row stride ld -> one swizzled LDS image (rows past S - 1 repeat row S - 1, the
// columns DH .. DHP - 1 are zero): the forward's staging
template <int DH>
__device__ __forceinline__ void pv_stage_rows(const uint16_t* __restrict__ src, int64_t ld, int r0, int S, char* img, int tid) {
    constexpr int DHP = (DH + 31) / 32 * 32, CPR = DHP / 8;
    for (int e = tid; e < PV_SB * CPR; e += 256) {
        const int row = e / CPR, c = e - row * CPR;
        int r = r0 + row; r = r < S ? r : S - 1;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (c * 8 < DH) v = *reinterpret_cast<const u32x4*>(src + (int64_t)r * ld + c * 8);
        *reinterpret_cast<u32x4*>(img + pv_swz<CPR>(row, c)) = v;
    }
}

// B-operand fragments of row `r` (one row per lane i16, lane group g the columns ks * 32 + 8 g ..): straight from global memory
template <int DH>
__device__ __forceinline__ void pv_row_frag(const uint16_t* __restrict__ src, int64_t ld, int r, int g, bf16x8 (&f)[(DH + 31) / 32]) {
#pragma unroll
    for (int ks = 0; ks < (DH + 31) / 32; ++ks) {
        const int dcol = ks * 32 + 8 * g;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (dcol < DH) v = *reinterpret_cast<const u32x4*>(src + (int64_t)r * ld + dcol);
        f[ks] = __builtin_bit_cast(bf16x8, v);
    }
}

__device__ __forceinline__ float pv_dot8(bf16x8 a, bf16x8 b) {
    const u32x4 x = __builtin_bit_cast(u32x4, a), y = __builtin_bit_cast(u32x4, b);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s = fmaf(pv_unpack_lo(x[i]), pv_unpack_lo(y[i]), s);
        s = fmaf(pv_unpack_hi(x[i]), pv_unpack_hi(y[i]), s);
    }
    return s;
}

// the A operand M^T (16 columns dt * 16 .. of the rows of one 32-row step) from a row-major swizzled image: two transposed reads sixteen rows apart
template <int DHP>
__device__ __forceinline__ bf16x8 pv_tr_frag(const char* img, int off, int tt) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + off + tt * (32 * DHP * 2)));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + off + tt * (32 * DHP * 2) + 16 * DHP * 2));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the two products the backward kernels recompute for one 16-row tile `t` of two LDS images: s += A[t] x^T (the scores) and c += B[t] y^T (dP), the
// rows of both images read at the lane's offsets off[ks], x and y the lane's own fragments
template <int DH>
__device__ __forceinline__ void pv_sdp_tile(const char* A, const char* B, const int (&off)[(DH + 31) / 32], int t, const bf16x8 (&x)[(DH + 31) / 32],
                                            const bf16x8 (&y)[(DH + 31) / 32], f32x4& s, f32x4& c) {
    constexpr int DHP = (DH + 31) / 32 * 32;
#pragma unroll
    for (int ks = 0; ks < DHP / 32; ++ks) {
        s = PV_MFMA_16x16x32(*reinterpret_cast<const bf16x8*>(A + off[ks] + t * (16 * DHP * 2)), x[ks], s, 0, 0, 0);
        c = PV_MFMA_16x16x32(*reinterpret_cast<const bf16x8*>(B + off[ks] + t * (16 * DHP * 2)), y[ks], c, 0, 0, 0);
    }
}

__device__ __forceinline__ bf16x8 pv_pack_step(const f32x4& a, const f32x4& b) {
    const u32x4 w = {pv_pack_bf16x2(a[0], a[1]), pv_pack_bf16x2(a[2], a[3]), pv_pack_bf16x2(b[0], b[1]), pv_pack_bf16x2(b[2], b[3])};
    return __builtin_bit_cast(bf16x8, w);
}

// O16 (pv_attention_stream_bwd16_bf16, include/peekvit_hip_pct_block.h): the lane's NDT x 4 accumulators of one row, times sc, are rounded once to the
// operand type and stored at op16 (columns 16 dt + 4 g + r of the head) when the row exists.  dbp (optional): the column sums of the STORED values over
// the workgroup's 64 rows (a missing row adds nothing) - the sixteen rows of a wave by xor-shuffles within its lane groups, the four waves through
// `red` (>= 4 DH floats of an LDS image the sweep has finished with), added in a fixed order by the one thread that owns the column.
template <int DH>
__device__ __forceinline__ void pv_store16_colsum(const f32x4 (&acc)[DH / 16], float sc, bool valid, uint16_t* op16, float* dbp, float* red, int tid) {
    const int lane = tid & 63, wid = tid >> 6, g = lane >> 4, i16 = lane & 15;
    if (dbp) __syncthreads();                      // every wave is done with the image (and with the previous sums)
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
        const u32x2 pk = {pv_pack_bf16x2(acc[dt][0] * sc, acc[dt][1] * sc), pv_pack_bf16x2(acc[dt][2] * sc, acc[dt][3] * sc)};
        if (valid) *reinterpret_cast<u32x2*>(op16 + dt * 16) = pk;
        if (dbp) {
            float c[4] = {pv_unpack_lo(pk[0]), pv_unpack_hi(pk[0]), pv_unpack_lo(pk[1]), pv_unpack_hi(pk[1])};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                c[r] = valid ? c[r] : 0.f;
                c[r] += __shfl_xor(c[r], 1, 64);
                c[r] += __shfl_xor(c[r], 2, 64);
                c[r] += __shfl_xor(c[r], 4, 64);
                c[r] += __shfl_xor(c[r], 8, 64);
                if (i16 == 0) red[wid * DH + dt * 16 + 4 * g + r] = c[r];
            }
        }
    }
    if (dbp) {
        __syncthreads();
        if (tid < DH) dbp[tid] = (red[tid] + red[DH + tid]) + (red[2 * DH + tid] + red[3 * DH + tid]);
    }
}
