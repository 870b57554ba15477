// ResidualViT training on the packed live rows (include/peekvit_hip_sparse_train.h): the attention backward over ragged row
// segments with a weight per key, and the backward of the pack step.  (The two forwards are further instantiations of existing kernel bodies and sit
// with them: pv_attention_varlen_w_lse_bf16's kernel in pv_attention.hip, pv_residual_pack_step_train in pv_sparse.hip.)  Past PV_SPARSE_MAX_LEN rows
// (include/peekvit_hip_sparse_long_train.h, section 35) the attention pair is the streaming forward with statistics (pv_attention.hip) and the LONG
// instantiation of the dQ body below; the pack step's backward for those rows is pv_sparse_long_train.hip.
//
// Attention backward: pv_attention_stream.hip's two-launch structure - each kernel walks the dimension its result is summed over and recomputes S and
// dP, so every sum has one owner and a fixed order and two runs give identical bits - on ragged segments:
//   * image b is the row segment [seg[b], seg[b+1]) of the packed matrices; the grid is the worst case, nb = ceil(max_len / 64) blocks per (image,
//     head), and a workgroup whose block starts beyond its segment leaves before its first barrier (after zeroing its slice of the bias partials);
//   * every key r has its own fp32 log-multiplicity lmul[r], added to its score wherever p is recomputed.  In the dQ kernel the key sits in the
//     accumulator rows, so the block's 64 weights are staged next to K and V and read as one 16-byte LDS read per key tile; in the dK | dV kernel the
//     key is the lane's own and its weight a register;
//   * a weighted key can hold nearly all of a row's probability, where dS = p (dP - delta) is a difference of nearly equal numbers and a delta formed
//     from the STORED 16-bit output carries that output's rounding, as large as the difference.  In a segment with any
//     non-zero weight the rows' delta is therefore sum_k p dP in fp32, by one more sweep over the keys; a segment without weights keeps
//     delta = sum_d dO O, bit for bit the uniform kernel's arithmetic.
// Statistics and delta are [R, H].  Lane maps, slot order and the fp16 build's probability scale are pv_attention_stream.hip's.
#include "pv_rows.h"
#include "pv_attn_tiles.h"
#include "../../include/peekvit_hip_sparse_long_train.h"

// ONE body for pv_attention_varlen_w_bwd16_bf16's dQ kernel and pv_attention_varlen_w_stream_bwd16_bf16's (include/peekvit_hip_sparse_long_train.h,
// DESIGN.md section 35).  LONG: segments of up to PV_SPARSE_LONG_MAX_LEN rows - the one line that knew a segment fits 256 threads, the test for a
// weighted key, walks the whole segment; everything else streams already.  Two __global__ functions wrap it, so the first keeps its name and its code.
template <int DH, bool LONG>
__device__ __forceinline__ void pv_attn_ragged_dq_body(const uint16_t* qkv, const uint16_t* dout, const uint16_t* att,
                                                       const float* lse, const int32_t* seg, const float* lmul,
                                                       float* delta_ws, uint16_t* dqkv16, float* dbias_partial,
                                                       int H, int nqb, float qscale) {
    constexpr int DHP = (DH + 31) / 32 * 32, CPR = DHP / 8, KS = DHP / 32, NDT = DH / 16;
    __shared__ __attribute__((aligned(16))) char Ks[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) char Vs[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) float Lm[PV_SB];          // the weights of the block's keys (0 past the segment's end)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15;
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh / H, h = bh - b * H;
    const int D = H * DH;
    const int64_t ld = 3 * (int64_t)D;
    const int s0 = seg[b], S = seg[b + 1] - s0;
    float* const dbp = dbias_partial ? dbias_partial + ((int64_t)b * nqb + qb) * ld + h * DH : nullptr;
    if (qb * PV_SB >= S || S > nqb * PV_SB) {          // (workgroup-uniform, before any barrier: a block beyond the segment, or a segment beyond the stated bound)
        if (dbp && tid < DH) dbp[tid] = 0.f;
        return;
    }
    const uint16_t* base = qkv + (int64_t)s0 * ld + h * DH;
    const int q = qb * PV_SB + wid * 16 + i16;         // this lane's query (every accumulator below holds it)
    const int qr = q < S ? q : S - 1;
    bf16x8 qf[KS], dof[KS];
    float delta = 0.f;
    {
        bf16x8 of[KS];
        pv_row_frag<DH>(base, ld, qr, g, qf);
        pv_row_frag<DH>(dout + (int64_t)s0 * D + h * DH, D, qr, g, dof);
        pv_row_frag<DH>(att + (int64_t)s0 * D + h * DH, D, qr, g, of);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) delta += pv_dot8(dof[ks], of[ks]);
        delta += __shfl_xor(delta, 16, 64);
        delta += __shfl_xor(delta, 32, 64);
    }
    const int64_t srow = (int64_t)(s0 + qr) * H + h;
    const float nl = -lse[srow];
    // does any key of the segment carry a weight?  (S <= nqb * 64 <= 256: one key per thread; LONG: every 256th key per thread, a key beyond row 255
    // that went unseen would leave its segment with the unweighted delta)
    bool anyw;
    if constexpr (LONG) {
        anyw = false;
        for (int k = tid; k < S; k += 256) anyw |= lmul[s0 + k] != 0.f;
    } else {
        anyw = tid < S && lmul[s0 + tid] != 0.f;
    }
    const bool weighted = __syncthreads_or(anyw) != 0;
    const int tq_ = i16 >> 2, tp_ = i16 & 3;
    int koff[KS], toff[NDT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = pv_swz<CPR>(i16, ks * 4 + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) toff[dt] = pv_swz<CPR>(4 * g + tq_, dt * 2 + (tp_ >> 1)) + ((tp_ & 1) << 3);
    if (weighted) {            // (uniform) delta = sum_k p dP in fp32, with the sweep's own s and dP
        float acc = 0.f;
        for (int k0 = 0; k0 < S; k0 += PV_SB) {
            __syncthreads();
            pv_stage_rows<DH>(base + D, ld, k0, S, Ks, tid);
            pv_stage_rows<DH>(base + 2 * D, ld, k0, S, Vs, tid);
            if (tid < PV_SB) Lm[tid] = k0 + tid < S ? lmul[s0 + k0 + tid] : 0.f;
            __syncthreads();
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
                pv_sdp_tile<DH>(Ks, Vs, koff, kt, qf, dof, s, c);
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(Lm + kt * 16 + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = k0 + kt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r] + w4[r], PV_LOG2E, nl)) : 0.f;
                    acc = fmaf(p, c[r], acc);
                }
            }
        }
        acc += __shfl_xor(acc, 16, 64);            // the four lane groups hold the keys 4 g + r of every 16-key tile
        acc += __shfl_xor(acc, 32, 64);
        delta = acc;
    }
    if (g == 0 && q < S) delta_ws[srow] = delta;
    f32x4 dq[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < S; k0 += PV_SB) {
        __syncthreads();                           // the previous block has been consumed
        pv_stage_rows<DH>(base + D, ld, k0, S, Ks, tid);
        pv_stage_rows<DH>(base + 2 * D, ld, k0, S, Vs, tid);
        if (tid < PV_SB) Lm[tid] = k0 + tid < S ? lmul[s0 + k0 + tid] : 0.f;
        __syncthreads();
        f32x4 ds[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
            pv_sdp_tile<DH>(Ks, Vs, koff, kt, qf, dof, s, c);
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(Lm + kt * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {          // key k0 + 16 kt + 4 g + r of query q
                const float p = k0 + kt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r] + w4[r], PV_LOG2E, nl)) : 0.f;
                ds[kt][r] = p * (c[r] - delta);
            }
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const bf16x8 dsf = pv_pack_step(ds[2 * tt], ds[2 * tt + 1]);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) dq[dt] = PV_MFMA_16x16x32(pv_tr_frag<DHP>(Ks, toff[dt], tt), dsf, dq[dt], 0, 0, 0);
        }
    }
    // (a lane without a row stores nothing: its pointer is never formed from q)
    pv_store16_colsum<DH>(dq, qscale, q < S, dqkv16 + (int64_t)(s0 + qr) * ld + h * DH + 4 * g, dbp, reinterpret_cast<float*>(Ks), tid);
}

template <int DH>
__global__ __launch_bounds__(256) void pv_attn_ragged_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const uint16_t* __restrict__ att,
                                                                const float* __restrict__ lse, const int32_t* __restrict__ seg, const float* __restrict__ lmul,
                                                                float* __restrict__ delta_ws, uint16_t* __restrict__ dqkv16, float* __restrict__ dbias_partial,
                                                                int H, int nqb, float qscale) {
    pv_attn_ragged_dq_body<DH, false>(qkv, dout, att, lse, seg, lmul, delta_ws, dqkv16, dbias_partial, H, nqb, qscale);
}

template <int DH>
__global__ __launch_bounds__(256) void pv_attn_ragged_dq_long_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
                                                                     const uint16_t* __restrict__ att, const float* __restrict__ lse,
                                                                     const int32_t* __restrict__ seg, const float* __restrict__ lmul,
                                                                     float* __restrict__ delta_ws, uint16_t* __restrict__ dqkv16,
                                                                     float* __restrict__ dbias_partial, int H, int nqb, float qscale) {
    pv_attn_ragged_dq_body<DH, true>(qkv, dout, att, lse, seg, lmul, delta_ws, dqkv16, dbias_partial, H, nqb, qscale);
}

template <int DH>
__global__ __launch_bounds__(256) void pv_attn_ragged_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                 const int32_t* __restrict__ seg, const float* __restrict__ lmul, const float* __restrict__ delta_ws,
                                                                 uint16_t* __restrict__ dqkv16, float* __restrict__ dbias_partial, int H, int nkb) {
    constexpr int DHP = (DH + 31) / 32 * 32, CPR = DHP / 8, KS = DHP / 32, NDT = DH / 16;
    __shared__ __attribute__((aligned(16))) char Qs[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) char Os[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) float Ls[PV_SB];          // - lse (+ PV_P_SHIFT) of the block's queries
    __shared__ __attribute__((aligned(16))) float Dl[PV_SB];          // delta (* 2^-PV_P_SHIFT)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15;
    const int kb = blockIdx.x % nkb, bh = blockIdx.x / nkb;
    const int b = bh / H, h = bh - b * H;
    const int D = H * DH;
    const int64_t ld = 3 * (int64_t)D;
    const int s0 = seg[b], S = seg[b + 1] - s0;
    float* const dbp = dbias_partial ? dbias_partial + ((int64_t)b * nkb + kb) * ld + h * DH : nullptr;
    if (kb * PV_SB >= S || S > nkb * PV_SB) {          // (workgroup-uniform, before any barrier)
        if (dbp && tid < DH) { dbp[D + tid] = 0.f; dbp[2 * D + tid] = 0.f; }
        return;
    }
    const uint16_t* base = qkv + (int64_t)s0 * ld + h * DH;
    const uint16_t* dob = dout + (int64_t)s0 * D + h * DH;
    const int key = kb * PV_SB + wid * 16 + i16;       // this lane's key (every accumulator below holds it)
    const int kr = key < S ? key : S - 1;
    const float tb = lmul[s0 + kr];                    // the weight of this lane's key
    bf16x8 kf[KS], vf[KS];
    pv_row_frag<DH>(base + D, ld, kr, g, kf);
    pv_row_frag<DH>(base + 2 * D, ld, kr, g, vf);
    const int tq_ = i16 >> 2, tp_ = i16 & 3;
    int roff[KS], toff[NDT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) roff[ks] = pv_swz<CPR>(i16, ks * 4 + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) toff[dt] = pv_swz<CPR>(4 * g + tq_, dt * 2 + (tp_ >> 1)) + ((tp_ & 1) << 3);
    f32x4 dk[NDT], dv[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
    for (int q0 = 0; q0 < S; q0 += PV_SB) {
        __syncthreads();                           // the previous block has been consumed
        pv_stage_rows<DH>(base, ld, q0, S, Qs, tid);
        pv_stage_rows<DH>(dob, D, q0, S, Os, tid);
        if (tid < PV_SB) {
            int r = q0 + tid; r = r < S ? r : S - 1;
            Ls[tid] = PV_P_SHIFT - lse[(int64_t)(s0 + r) * H + h];
            Dl[tid] = delta_ws[(int64_t)(s0 + r) * H + h] * PV_P_UNSHIFT;
        }
        __syncthreads();
        f32x4 p[4], ds[4];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
            pv_sdp_tile<DH>(Qs, Os, roff, qt, kf, vf, s, c);
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qt * 16 + 4 * g);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(Dl + qt * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {          // query q0 + 16 qt + 4 g + r against this lane's key; a query past S - 1 contributes nothing
                p[qt][r] = q0 + qt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r] + tb, PV_LOG2E, l4[r])) : 0.f;
                ds[qt][r] = p[qt][r] * fmaf(c[r], PV_P_UNSHIFT, -d4[r]);       // (PV_P_SHIFT = 0: c - delta, exactly)
            }
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const bf16x8 pf = pv_pack_step(p[2 * tt], p[2 * tt + 1]), dsf = pv_pack_step(ds[2 * tt], ds[2 * tt + 1]);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                dv[dt] = PV_MFMA_16x16x32(pv_tr_frag<DHP>(Os, toff[dt], tt), pf, dv[dt], 0, 0, 0);
                dk[dt] = PV_MFMA_16x16x32(pv_tr_frag<DHP>(Qs, toff[dt], tt), dsf, dk[dt], 0, 0, 0);
            }
        }
    }
    uint16_t* op16 = dqkv16 + (int64_t)(s0 + kr) * ld + h * DH + 4 * g;
    pv_store16_colsum<DH>(dk, 1.0f, key < S, op16 + D, dbp ? dbp + D : nullptr, reinterpret_cast<float*>(Qs), tid);
    pv_store16_colsum<DH>(dv, PV_P_UNSHIFT, key < S, op16 + 2 * D, dbp ? dbp + 2 * D : nullptr, reinterpret_cast<float*>(Qs), tid);
}

extern "C" int pv_attention_varlen_w_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg_start, const float* log_mult, int64_t B,
                                              int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream) {
    if (!qkv || !out || !lse || !seg_start || !log_mult || B <= 0 || H <= 0 || max_len <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)log_mult & 3) || ((uintptr_t)seg_start & 3) ||
        ((uintptr_t)range_flag & 3))
        return PV_ERR_INVALID_ARG;
    if (dh != 64 || max_len > PV_SPARSE_MAX_LEN || B > 0x7fffffff || H > 0x7fffffff || B * H > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    return pv_launch_attn_varlen_w_lse(qkv, out, lse, seg_start, log_mult, B, (int)max_len, (int)H, range_flag, (hipStream_t)stream);
}

extern "C" int pv_attention_varlen_w_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, const int32_t* seg_start,
                                                const float* log_mult, uint16_t* dqkv16, float* dbias_partial, float* delta_ws, int64_t B, int64_t max_len,
                                                int64_t H, int64_t dh, float qscale, void* stream) {
    if (!qkv || !dout || !out || !lse || !seg_start || !log_mult || !dqkv16 || !delta_ws || B <= 0 || H <= 0 || max_len <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)out & 15) || ((uintptr_t)dqkv16 & 15) || ((uintptr_t)lse & 3) ||
        ((uintptr_t)delta_ws & 3) || ((uintptr_t)dbias_partial & 3) || ((uintptr_t)log_mult & 3) || ((uintptr_t)seg_start & 3))
        return PV_ERR_INVALID_ARG;
    if (dh != 64 || max_len > PV_SPARSE_MAX_LEN || B > 0x7fffffff || H > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    const int nb = (int)((max_len + PV_SB - 1) / PV_SB);        // query blocks of the first kernel = key blocks of the second
    if (B * H * nb > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * H * nb));
    PV_LAUNCH(pv_attn_ragged_dq_kernel<64>, grid, dim3(256), 0, s, qkv, dout, out, lse, seg_start, log_mult, delta_ws, dqkv16, dbias_partial, (int)H, nb, qscale);
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_attn_ragged_dkv_kernel<64>, grid, dim3(256), 0, s, qkv, dout, lse, seg_start, log_mult, (const float*)delta_ws, dqkv16, dbias_partial, (int)H, nb);
    return pv_check_launch();
}

// ---- the same pair past PV_SPARSE_MAX_LEN rows (include/peekvit_hip_sparse_long_train.h) ------------------------------------------------------------
extern "C" int pv_attention_varlen_w_stream_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg_start, const float* log_mult, int64_t B,
                                                     int64_t max_len, int64_t H, int64_t dh, uint32_t* range_flag, void* stream) {
    if (!qkv || !out || !lse || !seg_start || !log_mult || B <= 0 || H <= 0 || max_len <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 7) || ((uintptr_t)lse & 3) || ((uintptr_t)log_mult & 3) || ((uintptr_t)seg_start & 3) ||
        ((uintptr_t)range_flag & 3))
        return PV_ERR_INVALID_ARG;
    if (dh != 64 || max_len > PV_SPARSE_LONG_MAX_LEN || B > 0x7fffffff || H > 0x7fffffff || B * H > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    return pv_launch_attn_stream_var_lse(qkv, out, lse, seg_start, log_mult, B, (int)max_len, (int)H, range_flag, (hipStream_t)stream);
}

// The dQ launch is the LONG instantiation; the dK | dV launch is the kernel above as it stands (its one length assumption is the S > nkb * 64 guard).
extern "C" int pv_attention_varlen_w_stream_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, const int32_t* seg_start,
                                                       const float* log_mult, uint16_t* dqkv16, float* dbias_partial, float* delta_ws, int64_t B,
                                                       int64_t max_len, int64_t H, int64_t dh, float qscale, void* stream) {
    if (!qkv || !dout || !out || !lse || !seg_start || !log_mult || !dqkv16 || !delta_ws || B <= 0 || H <= 0 || max_len <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)out & 15) || ((uintptr_t)dqkv16 & 15) || ((uintptr_t)lse & 3) ||
        ((uintptr_t)delta_ws & 3) || ((uintptr_t)dbias_partial & 3) || ((uintptr_t)log_mult & 3) || ((uintptr_t)seg_start & 3))
        return PV_ERR_INVALID_ARG;
    if (dh != 64 || max_len > PV_SPARSE_LONG_MAX_LEN || B > 0x7fffffff || H > 0x7fffffff || B * H > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    const int nb = (int)((max_len + PV_SB - 1) / PV_SB);        // query blocks of the first kernel = key blocks of the second
    if (B * H * nb > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * H * nb));
    PV_LAUNCH(pv_attn_ragged_dq_long_kernel<64>, grid, dim3(256), 0, s, qkv, dout, out, lse, seg_start, log_mult, delta_ws, dqkv16, dbias_partial, (int)H, nb, qscale);
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH(pv_attn_ragged_dkv_kernel<64>, grid, dim3(256), 0, s, qkv, dout, lse, seg_start, log_mult, (const float*)delta_ws, dqkv16, dbias_partial, (int)H, nb);
    return pv_check_launch();
}

// ---- backward of the pack step: pv_residual_gate_bwd_kernel's arithmetic (pv_rowops.hip) on packed rows --------------------------------------------
// One workgroup per image, a wave per input row, x and G of the row in registers.  The gather's transpose needs no search: src_next names the input
// row of every written row, so the image's inverse table (input row -> written row, -1 for a row that merged into the zero row) is built in LDS.  The
// dense mask's gradient comes back per input row as the sum over the row's tokens, in token order, by the one thread that owns the row.
#define PV_SPT_MAXL 256         // rows of one segment the kernel can hold (one thread per row); the entry point admits PV_SPARSE_MAX_LEN

template <int NCH>
__global__ __launch_bounds__(256) void pv_sp_pack_bwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ tok_row,
                                                             int N, int D, const float* __restrict__ mask_row, const float* __restrict__ gate_arg,
                                                             const float* __restrict__ thr_in, const int32_t* __restrict__ seg_next,
                                                             const int32_t* __restrict__ src_next, const float* __restrict__ G, const float* __restrict__ drs,
                                                             const float* __restrict__ dmask, const float* __restrict__ wg, const float* __restrict__ wb,
                                                             float temp, float* __restrict__ dx, float* __restrict__ dm_row, float* __restrict__ dwg_part,
                                                             float* __restrict__ dwb_part, float* __restrict__ scal_part) {
    __shared__ int inv[PV_SPT_MAXL], stok[PV_SPT_MAXL];
    __shared__ float dms[PV_SPT_MAXL], sdm[PV_SPT_MAXL];
    __shared__ float red_s[4][2];
    __shared__ float4 red_w[3][NCH * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0, d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    if (L < 2 || L > N + 2 || N + 2 > PV_SPT_MAXL || Ln < 2 || Ln > L) {          // (workgroup-uniform: tables this library did not write - the image adds nothing)
        for (int idx = tid; idx < nvec; idx += 256) {
            reinterpret_cast<float4*>(dwg_part + (int64_t)b * D)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(dwb_part + (int64_t)b * D)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 4) scal_part[b * 4 + tid] = 0.f;
        return;
    }
    if (tid < L) inv[tid] = -1;
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        stok[t] = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        sdm[t] = dmask ? dmask[(int64_t)b * N + t] : 0.f;
    }
    __syncthreads();
    if (tid < Ln) {
        const int i = src_next[d0 + tid];
        if (i >= 0 && i < L) inv[i] = tid;
    }
    if (tid < L) {
        float s = 0.f;
        for (int t = 0; t < N; ++t) s += stok[t] == tid ? sdm[t] : 0.f;
        dms[tid] = s;
        if (tid == 0 || tid == L - 1) dm_row[s0 + tid] = 0.f;
    }
    __syncthreads();
    const float thr = thr_in[b];
    if (wave == 1) {      // class row: passes through
        const float4* s4 = reinterpret_cast<const float4*>(G + (int64_t)d0 * D);
        float4* d4 = reinterpret_cast<float4*>(dx + (int64_t)s0 * D);
        for (int idx = lane; idx < nvec; idx += 64) d4[idx] = s4[idx];
    }
    float4 wv[NCH], acc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int idx = lane + 64 * j;
        wv[j] = idx < nvec ? reinterpret_cast<const float4*>(wg)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float dbg = 0.f, dthr = 0.f;
    for (int i = 1 + wave; i < L - 1; i += 4) {
        const int jn = inv[i];                     // (wave-uniform)
        float* dxr = dx + (int64_t)(s0 + i) * D;
        if (jn < 1 || jn >= Ln - 1) {              // merged into the zero row: multiplied by 0 in the forward, relu's slope is 0
            for (int idx = lane; idx < nvec; idx += 64) reinterpret_cast<float4*>(dxr)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane == 0) dm_row[s0 + i] = 0.f;
            continue;
        }
        RowRegs<NCH> r, gr;
        pv_load_row<NCH>(r, x + (int64_t)(s0 + i) * D, nvec, lane);
        pv_load_row<NCH>(gr, G + (int64_t)(d0 + jn) * D, nvec, lane);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) a += (r.v[j].x * gr.v[j].x + r.v[j].y * gr.v[j].y) + (r.v[j].z * gr.v[j].z + r.v[j].w * gr.v[j].w);
        a = pv_wave_sum(a);
        const float t = gate_arg[s0 + i], m = mask_row[s0 + i];
        const float dm = (a + drs[d0 + jn]) + dms[i];
        // sigmoid'(t) = sigmoid(t) sigmoid(-t): "1 - sg" would lose digits where the gate sits near 1 (pv_residual_gate_bwd_kernel)
        const float dz = dm * pv_sigmoid(t) * pv_sigmoid(-t) / temp;
        dthr -= dm;
        dbg += dz;
        if (lane == 0) dm_row[s0 + i] = dm;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) {
                reinterpret_cast<float4*>(dxr)[idx] = make_float4(m * gr.v[j].x + dz * wv[j].x, m * gr.v[j].y + dz * wv[j].y,
                                                                  m * gr.v[j].z + dz * wv[j].z, m * gr.v[j].w + dz * wv[j].w);
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
        const float du = dthr_t * thr * (1.0f - thr);      // the threshold is a mid-range sigmoid: no cancellation here
        const float4* xb4 = reinterpret_cast<const float4*>(x + (int64_t)(s0 + L - 1) * D);
        const float4* g4 = reinterpret_cast<const float4*>(G + (int64_t)(d0 + Ln - 1) * D);
        float4* d4 = reinterpret_cast<float4*>(dx + (int64_t)(s0 + L - 1) * D);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) {
                const float4 t0 = red_w[0][idx], t1 = red_w[1][idx], t2 = red_w[2][idx];
                reinterpret_cast<float4*>(dwg_part + (int64_t)b * D)[idx] =
                    make_float4(acc[j].x + t0.x + t1.x + t2.x, acc[j].y + t0.y + t1.y + t2.y, acc[j].z + t0.z + t1.z + t2.z, acc[j].w + t0.w + t1.w + t2.w);
                const float4 xv = xb4[idx], gv = g4[idx], w = reinterpret_cast<const float4*>(wb)[idx];
                d4[idx] = make_float4(gv.x + du * w.x, gv.y + du * w.y, gv.z + du * w.z, gv.w + du * w.w);
                reinterpret_cast<float4*>(dwb_part + (int64_t)b * D)[idx] = make_float4(du * xv.x, du * xv.y, du * xv.z, du * xv.w);
            }
        }
        if (lane == 0) { scal_part[b * 4] = dbg_t; scal_part[b * 4 + 1] = du; scal_part[b * 4 + 2] = 0.f; scal_part[b * 4 + 3] = 0.f; }
    }
}

extern "C" int pv_residual_pack_step_bwd(const float* x, const int32_t* seg_start, const int32_t* tok_row, const float* mask_row, const float* gate_arg,
                                         const float* thr, const int32_t* seg_next, const int32_t* src_next, const float* g_next, const float* drow_scale,
                                         const float* dmask, int64_t B, int64_t N, int64_t D, const float* wg, const float* wb, float temp, float* dx,
                                         float* dm_row, float* dwg_part, float* dwb_part, float* scal_part, void* stream) {
    if (!x || !seg_start || !tok_row || !mask_row || !gate_arg || !thr || !seg_next || !src_next || !g_next || !drow_scale || !wg || !wb || !dx || !dm_row ||
        !dwg_part || !dwb_part || !scal_part || B <= 0 || N < 0 || D <= 0 || temp == 0.f)
        return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x | (uintptr_t)g_next | (uintptr_t)dx | (uintptr_t)wg | (uintptr_t)wb | (uintptr_t)dwg_part | (uintptr_t)dwb_part | (uintptr_t)scal_part) & 15)
        return PV_ERR_INVALID_ARG;
    if (x == dx || g_next == dx) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096 || N + 2 > PV_SPARSE_MAX_LEN || B > 0x7fffffff) return PV_ERR_UNSUPPORTED;
#define SPB_LAUNCH(NC) PV_LAUNCH(pv_sp_pack_bwd_kernel<NC>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, x, seg_start, tok_row, (int)N, (int)D, mask_row, \
                                 gate_arg, thr, seg_next, src_next, g_next, drow_scale, dmask, wg, wb, temp, dx, dm_row, dwg_part, dwb_part, scal_part)
    PV_DISPATCH_NCH(D, SPB_LAUNCH);
#undef SPB_LAUNCH
    return pv_check_launch();
}
