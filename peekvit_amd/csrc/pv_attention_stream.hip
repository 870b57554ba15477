// Streaming attention for training on gfx950: the entry points of include/peekvit_hip_attn_stream.h and the two backward kernels.  Any S >= 1:
// nothing here holds a whole head in the LDS (the resident backward kernels of pv_attention.hip stop at S = 208, 416 at dh = 32).
//
//   forward    pv_attn_stream_kernel<dh, LSE = true> (pv_attention.hip): out and lse[b, h, q] = log2 sum_k exp(s[q, k])
//   backward   with p = exp2(s log2(e) - lse), dP = dO V^T, delta[q] = sum_d dO[q, d] O[q, d], dS = p o (dP - delta):
//                dQ = dS K        dK = dS^T Q        dV = P^T dO
//
// TWO launches, no atomics, no hand-off between workgroups.  dQ is a sum over the keys and dK, dV are sums over the queries: a single kernel that
// walks one of the two has to add the other across workgroups (float atomics: the bits depend on the order of arrival; an ordered hand-off: a
// spin between workgroups).  Here each kernel walks the dimension its result is summed over and recomputes S and dP - 7 MFMA products per
// (64 x 64) tile pair instead of 5 - so every sum has one owner and a fixed order: two runs give identical bits.
//
//   pv_attn_stream_dq_kernel    one workgroup = 64 queries of one (image, head), a 16-query tile per wave: the forward's grid and staging.  K and V
//                               blocks of 64 keys pass through the LDS; S^T = K Q^T and dP^T = V dO^T with the QUERY on the lane (lse and delta are
//                               per-lane scalars), and the packed dS^T accumulators are the B operand of dQ^T += K^T dS^T, K^T by transposed LDS reads:
//                               exactly how the forward feeds P to V^T P^T.  Its prologue forms delta and leaves it in delta_ws.
//   pv_attn_stream_dkv_kernel   one workgroup = 64 keys, a 16-key tile per wave whose K and V fragments stay in registers.  Blocks of 64 queries pass
//                               through the LDS (Q rows, dO rows, lse, delta); S = Q K^T and dP = dO V^T with the KEY on the lane, so the packed
//                               P and dS accumulators are the B operands of dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T by transposed reads of the
//                               same images).  dK^T and dV^T live in accumulators for the whole sweep and are stored once.
//
// Slot order of the packed operands (both kernels, as in the forward): k slot j of lane group g in the 32-row step tt is row 32 tt + 4 g + j (j < 4) or
// 32 tt + 16 + 4 g + j - 4 (j >= 4) on BOTH operands - two ds_read_b64_tr_b16 sixteen rows apart on the A side.
//
// fp16 build: P is packed as p * 2^PV_P_SHIFT for dV (the fp16 MFMA flushes subnormal operands), dS keeps its own magnitude - the factor leaves inside
// the bracket, (dP - delta) * 2^-PV_P_SHIFT as one FMA - and dV is multiplied by the exact 2^-PV_P_SHIFT where it is stored: pv_attn_bwd_kernel's
// arithmetic.  The dQ kernel packs no P and needs no factor.  PV_P_SHIFT = 0 (bf16 build) changes nothing.
//
// Results are fp32 [B, S, 3 D] (the caller normalises dO by a power of two and undoes it afterwards: an fp32 result has the range for that).
#include "pv_common.h"
#include "pv_attn_tiles.h"       // staging, fragments, packing and the 16-bit store of the two backward kernels (shared with pv_sparse_train.hip)
#include "pv_attn.h"
#include "../../include/peekvit_hip_attn_stream.h"
#include "../../include/peekvit_hip_pct_block.h"       // pv_attention_stream_bwd16_bf16: the O16 instantiations of the two backward kernels
#include "../../include/peekvit_hip_rank_train.h"      // pv_attention_stream_{lse, bwd16}_w_bf16: the W instantiations (a last key that stands for several)
#include "../../include/peekvit_hip_dropout.h"         // pv_attention_stream_{lse, bwd16}_drop_bf16: the DROP instantiations (dropout on the probabilities)

// W (pv_attention_stream_bwd16_w_bf16, include/peekvit_hip_rank_train.h): the forward added tail_log_mult to the score of key S - 1 (a key that stands for
// several identical ones); both kernels add it again, in fp32, where they recompute p.  With a weight the dQ kernel also forms the rows' delta itself,
// from p and dP (see there); with tail_log_mult = 0 nothing else changes.
//
// DROP (pv_attention_stream_bwd16_drop_bf16, include/peekvit_hip_dropout.h): the forward dropped probabilities with the mask M of pv_dropout.h and scaled the
// survivors by 1 / (1 - p).  delta = rowsum(dO o O) of the STORED output stays what it is (sum_k P_k M_k dP_k / (1 - p) = sum_d dO_d O_d), dS becomes
// P o (M o dP / (1 - p) - delta) in fp32 with the unrounded P, and dV uses P o M with 1 / (1 - p) applied where dV is stored.  Both kernels evaluate
// the mask again: the dQ kernel holds one query per lane (one row key per lane), the dK | dV kernel stages the 64 row keys of a query block in the
// LDS next to Ls / Dl.  Every added line sits under `if constexpr (DROP)`.
template <int DH, bool O16 = false, bool W = false, bool DROP = false>
__global__ __launch_bounds__(256) void pv_attn_stream_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const uint16_t* __restrict__ att,
                                                                const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ delta_ws, int S, int H,
                                                                int nqb, float qscale, uint16_t* __restrict__ dqkv16 = nullptr,
                                                                float* __restrict__ dbias_partial = nullptr, float tail_log_mult = 0.f, PvDrop dr = PvDrop{}) {
    constexpr int DHP = (DH + 31) / 32 * 32, CPR = DHP / 8, KS = DHP / 32, NDT = DH / 16;
    __shared__ __attribute__((aligned(16))) char Ks[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) char Vs[PV_SB * DHP * 2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15;
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh / H, h = bh - b * H;
    const int D = H * DH;
    const int64_t ld = 3 * (int64_t)D;
    const uint16_t* base = qkv + (int64_t)b * S * ld + h * DH;
    const int q = qb * 64 + wid * 16 + i16;            // this lane's query (every accumulator below holds it)
    const int qr = q < S ? q : S - 1;
    bf16x8 qf[KS], dof[KS];
    float delta = 0.f;
    {
        bf16x8 of[KS];
        pv_row_frag<DH>(base, ld, qr, g, qf);
        pv_row_frag<DH>(dout + (int64_t)b * S * D + h * DH, D, qr, g, dof);
        pv_row_frag<DH>(att + (int64_t)b * S * D + h * DH, D, qr, g, of);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) delta += pv_dot8(dof[ks], of[ks]);
        delta += __shfl_xor(delta, 16, 64);
        delta += __shfl_xor(delta, 32, 64);
    }
    const int64_t srow = ((int64_t)b * H + h) * S;
    if (g == 0 && q < S) delta_ws[srow + q] = delta;
    const float nl = -lse[srow + qr];
    uint32_t rk_lo = 0u, rk_hi = 0u;               // (DROP) the two halves of this lane's row key
    if constexpr (DROP) {
        const uint64_t rk = pv_drop_row_key(dr.base, (uint64_t)(srow + qr));
        rk_lo = (uint32_t)rk;
        rk_hi = (uint32_t)(rk >> 32);
    }
    const int tq_ = i16 >> 2, tp_ = i16 & 3;
    int koff[KS], toff[NDT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = pv_swz<CPR>(i16, ks * 4 + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) toff[dt] = pv_swz<CPR>(4 * g + tq_, dt * 2 + (tp_ >> 1)) + ((tp_ & 1) << 3);
    if constexpr (W) {
        // A weighted key can hold nearly all of a row's probability; dS = p (dP - delta) of that key is then a difference of nearly equal numbers, and a
        // delta formed from the STORED 16-bit output carries that output's rounding (2^-9 / 2^-12 relative), which is as large as the difference (one
        // other key against a key weighted 500 times: dq, dk 8 - 30 % off in bf16).  With a weight the row's delta is therefore formed from what it is
        // the sum of - delta = sum_k p_k dP_k, in fp32, by one more sweep over the keys with the sweep's own s and dP - and that value goes to delta_ws
        // for the dK | dV launch.  tail_log_mult = 0 is the unweighted kernel by definition and keeps its delta, bit for bit.
        if (tail_log_mult != 0.f) {
            float acc = 0.f;
            for (int k0 = 0; k0 < S; k0 += PV_SB) {
                __syncthreads();
                pv_stage_rows<DH>(base + D, ld, k0, S, Ks, tid);
                pv_stage_rows<DH>(base + 2 * D, ld, k0, S, Vs, tid);
                __syncthreads();
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
                    pv_sdp_tile<DH>(Ks, Vs, koff, kt, qf, dof, s, c);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (k0 + kt * 16 + 4 * g + r == S - 1) s[r] += tail_log_mult;
                        const float p = k0 + kt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r], PV_LOG2E, nl)) : 0.f;
                        acc = fmaf(p, c[r], acc);
                    }
                }
            }
            acc += __shfl_xor(acc, 16, 64);        // the four lane groups hold the keys 4 g + r of every 16-key tile
            acc += __shfl_xor(acc, 32, 64);
            delta = acc;
            if (g == 0 && q < S) delta_ws[srow + q] = delta;
        }
    }
    f32x4 dq[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < S; k0 += PV_SB) {
        __syncthreads();                           // the previous block has been consumed
        pv_stage_rows<DH>(base + D, ld, k0, S, Ks, tid);
        pv_stage_rows<DH>(base + 2 * D, ld, k0, S, Vs, tid);
        __syncthreads();
        f32x4 ds[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
            pv_sdp_tile<DH>(Ks, Vs, koff, kt, qf, dof, s, c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {          // key k0 + 16 kt + 4 g + r of query q
                if constexpr (W)
                    if (k0 + kt * 16 + 4 * g + r == S - 1) s[r] += tail_log_mult;
                const float p = k0 + kt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r], PV_LOG2E, nl)) : 0.f;
                if constexpr (DROP) c[r] = pv_drop_keep(rk_lo, rk_hi, (uint32_t)(k0 + kt * 16 + 4 * g + r), dr.thr) ? c[r] * dr.scale : 0.f;
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
    if constexpr (O16) {                           // the same values in 16 bits, and this (image, query block, head)'s slice of the bias partial row
        pv_store16_colsum<DH>(dq, qscale, q < S, dqkv16 + ((int64_t)b * S + q) * ld + h * DH + 4 * g,
                              dbias_partial ? dbias_partial + ((int64_t)b * nqb + qb) * ld + h * DH : nullptr, reinterpret_cast<float*>(Ks), tid);
    } else if (q < S) {                            // dq[dt][r] = dL/dq'[q][16 dt + 4 g + r]
        float* op = dqkv + ((int64_t)b * S + q) * ld + h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) *reinterpret_cast<f32x4*>(op + dt * 16) = dq[dt] * qscale;
    }
}

template <int DH, bool O16 = false, bool W = false, bool DROP = false>
__global__ __launch_bounds__(256) void pv_attn_stream_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                 const float* __restrict__ delta_ws, float* __restrict__ dqkv, int S, int H, int nkb,
                                                                 uint16_t* __restrict__ dqkv16 = nullptr, float* __restrict__ dbias_partial = nullptr,
                                                                 float tail_log_mult = 0.f, PvDrop dr = PvDrop{}) {
    constexpr int DHP = (DH + 31) / 32 * 32, CPR = DHP / 8, KS = DHP / 32, NDT = DH / 16;
    __shared__ __attribute__((aligned(16))) char Qs[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) char Os[PV_SB * DHP * 2];
    __shared__ __attribute__((aligned(16))) float Ls[PV_SB];          // - lse (+ PV_P_SHIFT) of the block's queries
    __shared__ __attribute__((aligned(16))) float Dl[PV_SB];          // delta (* 2^-PV_P_SHIFT)
    __shared__ __attribute__((aligned(16))) uint32_t Rk[DROP ? 2 * PV_SB : 4];      // (DROP) the block's row keys: the low halves, then the high halves
    const float su = DROP ? dr.scale * PV_P_UNSHIFT : PV_P_UNSHIFT;    // (DROP) 1 / (1 - p) rides with the exact power of two
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15;
    const int kb = blockIdx.x % nkb, bh = blockIdx.x / nkb;
    const int b = bh / H, h = bh - b * H;
    const int D = H * DH;
    const int64_t ld = 3 * (int64_t)D;
    const uint16_t* base = qkv + (int64_t)b * S * ld + h * DH;
    const uint16_t* dob = dout + (int64_t)b * S * D + h * DH;
    const int64_t srow = ((int64_t)b * H + h) * S;
    const int key = kb * 64 + wid * 16 + i16;          // this lane's key (every accumulator below holds it)
    const int kr = key < S ? key : S - 1;
    const float tb = (W && key == S - 1) ? tail_log_mult : 0.f;          // (W) the bias of this lane's key
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
            Ls[tid] = PV_P_SHIFT - lse[srow + r];
            Dl[tid] = delta_ws[srow + r] * PV_P_UNSHIFT;
            if constexpr (DROP) {
                const uint64_t rk = pv_drop_row_key(dr.base, (uint64_t)(srow + r));
                Rk[tid] = (uint32_t)rk;
                Rk[PV_SB + tid] = (uint32_t)(rk >> 32);
            }
        }
        __syncthreads();
        f32x4 p[4], ds[4];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = s;
            pv_sdp_tile<DH>(Qs, Os, roff, qt, kf, vf, s, c);
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qt * 16 + 4 * g);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(Dl + qt * 16 + 4 * g);
            u32x4 rl = {0u, 0u, 0u, 0u}, rh = rl;
            if constexpr (DROP) {
                rl = *reinterpret_cast<const u32x4*>(Rk + qt * 16 + 4 * g);
                rh = *reinterpret_cast<const u32x4*>(Rk + PV_SB + qt * 16 + 4 * g);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {          // query q0 + 16 qt + 4 g + r against this lane's key; a query past S - 1 contributes nothing
                if constexpr (W) s[r] += tb;
                p[qt][r] = q0 + qt * 16 + 4 * g + r < S ? __builtin_amdgcn_exp2f(fmaf(s[r], PV_LOG2E, l4[r])) : 0.f;
                if constexpr (DROP) {              // dS from the unrounded P, dV from P o M
                    const bool keep = pv_drop_keep(rl[r], rh[r], (uint32_t)key, dr.thr);
                    ds[qt][r] = p[qt][r] * fmaf(keep ? c[r] : 0.f, su, -d4[r]);
                    p[qt][r] = keep ? p[qt][r] : 0.f;
                } else {
                    ds[qt][r] = p[qt][r] * fmaf(c[r], PV_P_UNSHIFT, -d4[r]);   // (PV_P_SHIFT = 0: c - delta, exactly)
                }
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
    if constexpr (O16) {                           // the same values in 16 bits, and the k | v slices of the bias partial row
        uint16_t* op16 = dqkv16 + ((int64_t)b * S + key) * ld + h * DH + 4 * g;
        float* dbp = dbias_partial ? dbias_partial + ((int64_t)b * nkb + kb) * ld + h * DH : nullptr;
        pv_store16_colsum<DH>(dk, 1.0f, key < S, op16 + D, dbp ? dbp + D : nullptr, reinterpret_cast<float*>(Qs), tid);
        pv_store16_colsum<DH>(dv, su, key < S, op16 + 2 * D, dbp ? dbp + 2 * D : nullptr, reinterpret_cast<float*>(Qs), tid);
    } else if (key < S) {                          // d*[dt][r] = dL/d{k, v}[key][16 dt + 4 g + r]
        float* op = dqkv + ((int64_t)b * S + key) * ld + h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            *reinterpret_cast<f32x4*>(op + D + dt * 16) = dk[dt];
            *reinterpret_cast<f32x4*>(op + 2 * D + dt * 16) = dv[dt] * PV_P_UNSHIFT;
        }
    }
}

// The two launches of one instantiation: dQ (which leaves the rows' delta in delta_ws), then dK | dV.  The result is dqkv (fp32) or, O16, dqkv16 with
// the optional bias partial rows; tail_log_mult and dr are read by the W and DROP instantiations only.
template <int DH, bool O16, bool W, bool DROP>
static int pv_launch_attn_stream_bwd(const uint16_t* qkv, const uint16_t* dout, const uint16_t* att, const float* lse, float* dqkv, uint16_t* dqkv16,
                                     float* dbias_partial, float* delta_ws, int64_t B, int S, int H, float qscale, float tail_log_mult, const PvDrop& dr,
                                     hipStream_t stream) {
    const int nb = (S + PV_SB - 1) / PV_SB;        // query blocks of the first kernel = key blocks of the second
    if (B * H * nb > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(B * H * nb));
    PV_LAUNCH((pv_attn_stream_dq_kernel<DH, O16, W, DROP>), grid, dim3(256), 0, stream, qkv, dout, att, lse, dqkv, delta_ws, S, H, nb, qscale, dqkv16,
              dbias_partial, tail_log_mult, dr);
    if (pv_check_launch() != PV_OK) return PV_ERR_LAUNCH;
    PV_LAUNCH((pv_attn_stream_dkv_kernel<DH, O16, W, DROP>), grid, dim3(256), 0, stream, qkv, dout, lse, (const float*)delta_ws, dqkv, S, H, nb, dqkv16,
              dbias_partial, tail_log_mult, dr);
    return pv_check_launch();
}

template <bool O16, bool W, bool DROP>
static int pv_dispatch_attn_stream_bwd(int64_t dh, const uint16_t* qkv, const uint16_t* dout, const uint16_t* att, const float* lse, float* dqkv, uint16_t* dqkv16,
                                       float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, float qscale, float tail_log_mult,
                                       const PvDrop& dr, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    switch (dh) {
        case 32: return pv_launch_attn_stream_bwd<32, O16, W, DROP>(qkv, dout, att, lse, dqkv, dqkv16, dbias_partial, delta_ws, B, (int)S, (int)H, qscale, tail_log_mult, dr, s);
        case 48: return pv_launch_attn_stream_bwd<48, O16, W, DROP>(qkv, dout, att, lse, dqkv, dqkv16, dbias_partial, delta_ws, B, (int)S, (int)H, qscale, tail_log_mult, dr, s);
        case 64: return pv_launch_attn_stream_bwd<64, O16, W, DROP>(qkv, dout, att, lse, dqkv, dqkv16, dbias_partial, delta_ws, B, (int)S, (int)H, qscale, tail_log_mult, dr, s);
        default: return PV_ERR_UNSUPPORTED;
    }
}

// ---- the argument checks, one per shape of entry point: a null pointer or a non-positive size, then a misaligned pointer (both PV_ERR_INVALID_ARG), then
// the size limits (PV_ERR_UNSUPPORTED).  A variant's own argument (tail_log_mult, p) is tested by its entry point first and is an invalid argument. ----
static inline int pv_stream_fwd_args(const void* qkv, const void* out, const void* lse, const void* range_flag, int64_t B, int64_t S, int64_t H, int64_t dh) {
    if (!qkv || !out || !lse || B <= 0 || S <= 0 || H <= 0 || dh <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)range_flag & 3)) return PV_ERR_INVALID_ARG;
    if (B > 0x7fffffff || H > 0x7fffffff || B * H > 0x7fffffff || S > 0x3fffffff) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

// result: dqkv (fp32) or dqkv16, 16-byte aligned either way; dbias_partial is optional (the fp32 entry point has none)
static inline int pv_stream_bwd_args(const void* qkv, const void* dout, const void* out, const void* lse, const void* result, const void* delta_ws,
                                     const void* dbias_partial, int64_t B, int64_t S, int64_t H, int64_t dh) {
    if (!qkv || !dout || !out || !lse || !result || !delta_ws || B <= 0 || S <= 0 || H <= 0 || dh <= 0) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)out & 15) || ((uintptr_t)result & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)delta_ws & 3) ||
        ((uintptr_t)dbias_partial & 3))
        return PV_ERR_INVALID_ARG;
    if (B > 0x7fffffff || H > 0x7fffffff || B * H > 0x7fffffff || S > 0x3fffffff) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

extern "C" int pv_attention_stream_lse_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh, uint32_t* range_flag,
                                            void* stream) {
    if (const int rc = pv_stream_fwd_args(qkv, out, lse, range_flag, B, S, H, dh)) return rc;
    return pv_launch_attn_stream_lse(qkv, out, lse, B, (int)S, (int)H, (int)dh, range_flag, (hipStream_t)stream);
}

extern "C" int pv_attention_stream_bwd_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, float* dqkv, float* delta_ws, int64_t B,
                                            int64_t S, int64_t H, int64_t dh, float qscale, void* stream) {
    if (const int rc = pv_stream_bwd_args(qkv, dout, out, lse, dqkv, delta_ws, nullptr, B, S, H, dh)) return rc;
    return pv_dispatch_attn_stream_bwd<false, false, false>(dh, qkv, dout, out, lse, dqkv, nullptr, nullptr, delta_ws, B, S, H, qscale, 0.f, PvDrop{}, stream);
}

// The same backward with a 16-bit result and the bias partial rows (include/peekvit_hip_pct_block.h): the O16 instantiations of the two kernels.
extern "C" int pv_attention_stream_bwd16_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16, float* dbias_partial,
                                              float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale, void* stream) {
    if (const int rc = pv_stream_bwd_args(qkv, dout, out, lse, dqkv16, delta_ws, dbias_partial, B, S, H, dh)) return rc;
    return pv_dispatch_attn_stream_bwd<true, false, false>(dh, qkv, dout, out, lse, nullptr, dqkv16, dbias_partial, delta_ws, B, S, H, qscale, 0.f, PvDrop{}, stream);
}

// ---- a last key that stands for m identical ones (include/peekvit_hip_rank_train.h): tail_log_mult = ln m on its score, forward and backward ----
static inline bool pv_tail_log_mult_ok(float t) { return t >= 0.f && t <= 3.0e38f; }       // (false for a NaN, a negative value and +inf)

extern "C" int pv_attention_stream_lse_w_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh, float tail_log_mult,
                                              uint32_t* range_flag, void* stream) {
    if (!pv_tail_log_mult_ok(tail_log_mult)) return PV_ERR_INVALID_ARG;
    if (const int rc = pv_stream_fwd_args(qkv, out, lse, range_flag, B, S, H, dh)) return rc;
    return pv_launch_attn_stream_lse_w(qkv, out, lse, B, (int)S, (int)H, (int)dh, range_flag, tail_log_mult, (hipStream_t)stream);
}

extern "C" int pv_attention_stream_bwd16_w_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16,
                                                float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale,
                                                float tail_log_mult, void* stream) {
    if (!pv_tail_log_mult_ok(tail_log_mult)) return PV_ERR_INVALID_ARG;
    if (const int rc = pv_stream_bwd_args(qkv, dout, out, lse, dqkv16, delta_ws, dbias_partial, B, S, H, dh)) return rc;
    return pv_dispatch_attn_stream_bwd<true, true, false>(dh, qkv, dout, out, lse, nullptr, dqkv16, dbias_partial, delta_ws, B, S, H, qscale, tail_log_mult, PvDrop{},
                                                          stream);
}

// ---- dropout on the probabilities (include/peekvit_hip_dropout.h): the mask is evaluated again by every launch, nothing is stored ----
extern "C" int pv_attention_stream_lse_drop_bf16(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int64_t S, int64_t H, int64_t dh, float p, uint64_t key,
                                                 uint64_t site, uint32_t* range_flag, void* stream) {
    if (!pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (const int rc = pv_stream_fwd_args(qkv, out, lse, range_flag, B, S, H, dh)) return rc;
    return pv_launch_attn_stream_lse_drop(qkv, out, lse, B, (int)S, (int)H, (int)dh, range_flag, pv_drop_make(key, site, p), (hipStream_t)stream);
}

extern "C" int pv_attention_stream_bwd16_drop_bf16(const uint16_t* qkv, const uint16_t* dout, const uint16_t* out, const float* lse, uint16_t* dqkv16,
                                                   float* dbias_partial, float* delta_ws, int64_t B, int64_t S, int64_t H, int64_t dh, float qscale, float p,
                                                   uint64_t key, uint64_t site, void* stream) {
    if (!pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (const int rc = pv_stream_bwd_args(qkv, dout, out, lse, dqkv16, delta_ws, dbias_partial, B, S, H, dh)) return rc;
    return pv_dispatch_attn_stream_bwd<true, false, true>(dh, qkv, dout, out, lse, nullptr, dqkv16, dbias_partial, delta_ws, B, S, H, qscale, 0.f,
                                                          pv_drop_make(key, site, p), stream);
}
