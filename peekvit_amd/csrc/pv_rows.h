// The building blocks of a one-wave-per-row kernel (wave = 64 lanes, lane l holds the row's 16-byte chunks l, l + 64, ...): the row in
// registers, its LayerNorm, the ResidualViT gate arithmetic, the guarded row stores, the dispatch on the hidden width, the segment scan -
// and the fp32 classification head's tile and dot loops, which the plain head and the exit head share.
// A kernel that must round like another one CALLS these functions - it does not restate them: the arithmetic exists once, so a change to a
// reduction order or a contraction pragma reaches every kernel that depends on it.  Everything here is inlined into the including file and
// compiles under that file's flags (peekvit_amd/_build.py FILE_FLAGS).
#pragma once
#include "pv_common.h"

// row registers per lane by hidden width: MACRO(NCH) with NCH = the float4 chunks a lane holds (D <= 4096)
#define PV_DISPATCH_NCH(D, MACRO)              \
    do {                                       \
        int nch_ = (int)(((D) / 4 + 63) / 64); \
        if (nch_ <= 1) { MACRO(1); }           \
        else if (nch_ == 2) { MACRO(2); }      \
        else if (nch_ == 3) { MACRO(3); }      \
        else if (nch_ == 4) { MACRO(4); }      \
        else if (nch_ <= 8) { MACRO(8); }      \
        else { MACRO(16); }                    \
    } while (0)

// ---- LayerNorm row helpers (one wave per row, the row stays in registers; two-pass mean / variance in fp32).  Shared by the
// standalone LN kernel and the GEMM-fused LN pass so both round identically. -------------------------------------------
template <int NCH>
struct RowRegs {
    float4 v[NCH];
};

template <int NCH>
__device__ __forceinline__ void pv_load_row(RowRegs<NCH>& r, const float* __restrict__ xr, int nvec, int lane) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        int idx = lane + 64 * j;
        r.v[j] = idx < nvec ? reinterpret_cast<const float4*>(xr)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// A scalar fp32 add the compiler cannot fold into a packed (v_pk_add_f32) tree.  Round 4: v_pk_*_f32 whose LOW result reads the HIGH register
// of a source pair (an op_sel bit set - what hipcc emits for a horizontal add of a packed pair, or to broadcast a value that sits in an
// odd register) returned wrong low results in lanes 48-63 about 1e-5 of the time on gfx950 while vector-memory loads were returning into
// VGPRs (scripts/dbg/gelu_glitch.py); the sums below run under exactly such loads in the GEMM-fused LayerNorm
// epilogues.  Same operation, same rounding as `a + b`.
__device__ __forceinline__ float pv_add_s(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// JB rows at once (round 4): the SAME per-row arithmetic, written step by step ACROSS the rows, so that the JB independent chains of
// cross-lane reductions (two wave sums per row, each a dependent chain of four DPP adds, four v_readlane and three scalar adds) interleave
// instead of running one after the other - the GEMM-fused LayerNorm passes are latency-bound on exactly these chains.  JB = 1 is the
// standalone kernel's form; every row rounds identically for any JB.
//
// pv_ln_rows_stats: mean and rstd of the JB rows, the first two phases of pv_ln_rows_regs, for a kernel that normalises elsewhere (the tiled
// exit head keeps the two statistics in LDS and normalises an element as it is staged).
template <int NCH, int JB>
__device__ __forceinline__ void pv_ln_rows_stats(const RowRegs<NCH> (&r)[JB], int D, int nvec, int lane, float eps, float (&mean)[JB], float (&rstd)[JB]) {
    // every operation rounded on its own: which multiply-adds hipcc contracts into FMAs depends on the code this is inlined into, and the
    // standalone kernel and the GEMM-fused passes must agree to the bit (tests/test_hip_ops.py found a last-bit difference at N = 512)
#pragma clang fp contract(off)
    float s[JB], q[JB];
#pragma unroll
    for (int b = 0; b < JB; ++b) {
        s[b] = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) s[b] += pv_add_s(r[b].v[j].x + r[b].v[j].y, r[b].v[j].z + r[b].v[j].w);
    }
#pragma unroll
    for (int b = 0; b < JB; ++b) mean[b] = pv_wave_sum(s[b]) / (float)D;
#pragma unroll
    for (int b = 0; b < JB; ++b) {
        q[b] = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            if (lane + 64 * j < nvec) {
                float a = r[b].v[j].x - mean[b], bb = r[b].v[j].y - mean[b], c = r[b].v[j].z - mean[b], d = r[b].v[j].w - mean[b];
                q[b] += pv_add_s(a * a + bb * bb, c * c + d * d);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < JB; ++b) rstd[b] = 1.0f / sqrtf(pv_wave_sum(q[b]) / (float)D + eps);
}

// normalise in place: v <- (v - mean) * rstd * gamma + beta   (lanes beyond nvec keep zeros).  gamma / beta already in registers
// (the lane's NCH float4 of each): ONE arithmetic for the standalone kernel and the GEMM-fused passes.
template <int NCH, int JB>
__device__ __forceinline__ void pv_ln_rows_regs(RowRegs<NCH> (&r)[JB], const float4 (&gm)[NCH], const float4 (&bt)[NCH], int D, int nvec, int lane, float eps) {
#pragma clang fp contract(off)          // (as in pv_ln_rows_stats)
    float mean[JB], rstd[JB];
    pv_ln_rows_stats<NCH, JB>(r, D, nvec, lane, eps, mean, rstd);
#pragma unroll
    for (int b = 0; b < JB; ++b) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            int idx = lane + 64 * j;
            if (idx < nvec) {
                const float4 g = gm[j], be = bt[j];
                r[b].v[j].x = (r[b].v[j].x - mean[b]) * rstd[b] * g.x + be.x;
                r[b].v[j].y = (r[b].v[j].y - mean[b]) * rstd[b] * g.y + be.y;
                r[b].v[j].z = (r[b].v[j].z - mean[b]) * rstd[b] * g.z + be.z;
                r[b].v[j].w = (r[b].v[j].w - mean[b]) * rstd[b] * g.w + be.w;
            }
        }
    }
}

// Sixteen lanes per row (round 4, the full-row GEMM's epilogue): lane l16 of a 16-lane DPP row holds the 16-byte chunks l16 + 16 k (k < KC =
// D / 64) of ITS token row - every lane busy at any D, reductions by DPP alone, four token rows per wave at once.  The arithmetic AND its
// order are pv_ln_rows_regs': the wave-per-row form gives lane L = l16 + 16 i the chunks L and L + 64, sums a lane's chunks first
// ((0 + S_i) + S_{i+4}), then the 16 lanes of each DPP row, then (r0 + r1) + (r2 + r3); here a lane forms the same four partials itself and
// runs the same DPP tree on each of them, so every row rounds identically to the standalone kernel's (tests/test_hip_ops.py, bitwise).
// gamma / beta: the lane's chunks are read from an LDS copy (gb = gamma[D] | beta[D] floats).
template <int KC>
__device__ __forceinline__ void pv_ln_row16(float4 (&v)[KC], const __attribute__((address_space(3))) char* gb, int D, int l16, float eps) {
#pragma clang fp contract(off)
    static_assert(KC >= 4 && KC <= 8, "D = 256 .. 512");
    float pp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s_ = 0.f;
        s_ += pv_add_s(v[i].x + v[i].y, v[i].z + v[i].w);
        if (i + 4 < KC) s_ += pv_add_s(v[(i + 4) % KC].x + v[(i + 4) % KC].y, v[(i + 4) % KC].z + v[(i + 4) % KC].w);
        pp[i] = pv_row16_sum(s_);
    }
    const float mean = ((pp[0] + pp[1]) + (pp[2] + pp[3])) / (float)D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float q_ = 0.f;
        {
            const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q_ += pv_add_s(a * a + bb * bb, c * c + d * d);
        }
        if (i + 4 < KC) {
            const float a = v[(i + 4) % KC].x - mean, bb = v[(i + 4) % KC].y - mean, c = v[(i + 4) % KC].z - mean, d = v[(i + 4) % KC].w - mean;
            q_ += pv_add_s(a * a + bb * bb, c * c + d * d);
        }
        pp[i] = pv_row16_sum(q_);
    }
    const float rstd = 1.0f / sqrtf(((pp[0] + pp[1]) + (pp[2] + pp[3])) / (float)D + eps);
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const f32x4 g = *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(gb + (l16 + 16 * k) * 16);
        const f32x4 be = *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(gb + D * 4 + (l16 + 16 * k) * 16);
        v[k].x = (v[k].x - mean) * rstd * g[0] + be[0];
        v[k].y = (v[k].y - mean) * rstd * g[1] + be[1];
        v[k].z = (v[k].z - mean) * rstd * g[2] + be[2];
        v[k].w = (v[k].w - mean) * rstd * g[3] + be[3];
    }
}

template <int NCH>
__device__ __forceinline__ void pv_ln_row_regs(RowRegs<NCH>& r, const float4 (&gm)[NCH], const float4 (&bt)[NCH], int D, int nvec, int lane, float eps) {
    RowRegs<NCH> one[1] = {r};
    pv_ln_rows_regs<NCH, 1>(one, gm, bt, D, nvec, lane, eps);
    r = one[0];
}

template <int NCH>
__device__ __forceinline__ void pv_ln_load_affine(float4 (&gm)[NCH], float4 (&bt)[NCH], const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  int nvec, int lane) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int idx = lane + 64 * j < nvec ? lane + 64 * j : nvec - 1;
        gm[j] = reinterpret_cast<const float4*>(gamma)[idx];
        bt[j] = reinterpret_cast<const float4*>(beta)[idx];
    }
}

template <int NCH>
__device__ __forceinline__ void pv_ln_row(RowRegs<NCH>& r, const float* __restrict__ gamma, const float* __restrict__ beta, int D,
                                          int nvec, int lane, float eps) {
    float4 gm[NCH], bt[NCH];
    pv_ln_load_affine<NCH>(gm, bt, gamma, beta, nvec, lane);
    pv_ln_row_regs<NCH>(r, gm, bt, D, nvec, lane, eps);
}

// ---- ResidualViT gate (models/residualvit.py:197-235, eval, sigmoid gate): ONE arithmetic for the dense gate (pv_rowops.hip), its backward
// and the gate on packed rows (pv_sparse.hip) ---------------------------------------------------------------------------------
__device__ __forceinline__ float pv_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// the threshold's argument from the budget row (residualvit.py:212): x_row . wb summed over the wave, + bb[0], in every lane.  The caller takes
// pv_sigmoid of it inside `if (lane == 0)`: one lane's expf, not sixty-four.
__device__ __forceinline__ float pv_gate_budget_dot(const float* xr, const float* __restrict__ wb, const float* __restrict__ bb, int nvec, int lane) {
    float s = 0.f;
    for (int idx = lane; idx < nvec; idx += 64) {
        float4 v = reinterpret_cast<const float4*>(xr)[idx], w = reinterpret_cast<const float4*>(wb)[idx];
        s += (v.x * w.x + v.y * w.y) + (v.z * w.z + v.w * w.w);
    }
    return pv_wave_sum(s) + bb[0];
}

// the sigmoid's argument of a token row held in registers: (row . wg + bg) / temp + sbias   (blocks.py:69)
template <int NCH>
__device__ __forceinline__ float pv_gate_arg(const RowRegs<NCH>& r, const float* __restrict__ wg, const float* __restrict__ bg, float temp, float sbias,
                                             int nvec, int lane) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        int idx = lane + 64 * j;
        if (idx < nvec) {
            float4 w = reinterpret_cast<const float4*>(wg)[idx];
            s += (r.v[j].x * w.x + r.v[j].y * w.y) + (r.v[j].z * w.z + r.v[j].w * w.w);
        }
    }
    s = pv_wave_sum(s) + bg[0];
    return s / temp + sbias;
}

// its mask: relu(sigmoid(that argument) - thr)   (residualvit.py:66)
template <int NCH>
__device__ __forceinline__ float pv_gate_mask(const RowRegs<NCH>& r, const float* __restrict__ wg, const float* __restrict__ bg, float temp, float sbias,
                                              float thr, int nvec, int lane) {
    return fmaxf(pv_sigmoid(pv_gate_arg<NCH>(r, wg, bg, temp, sbias, nvec, lane)) - thr, 0.f);
}

// ---- guarded row stores: the lane's chunks below nvec ----------------------------------------------------------------------
template <int NCH>
__device__ __forceinline__ void pv_store_row(float* dst, const RowRegs<NCH>& r, int nvec, int lane) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        int idx = lane + 64 * j;
        if (idx < nvec) reinterpret_cast<float4*>(dst)[idx] = r.v[j];
    }
}

// the row as 16-bit operands (the plain form has no multiply: x * 1 is exact, but it is an instruction per element)
template <int NCH>
__device__ __forceinline__ void pv_store_row16(uint16_t* dst, const RowRegs<NCH>& r, int nvec, int lane) {
    u32x2* o = reinterpret_cast<u32x2*>(dst);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        int idx = lane + 64 * j;
        if (idx < nvec) o[idx] = (u32x2){pv_pack_bf16x2(r.v[j].x, r.v[j].y), pv_pack_bf16x2(r.v[j].z, r.v[j].w)};
    }
}

template <int NCH>
__device__ __forceinline__ void pv_store_row16_scaled(uint16_t* dst, const RowRegs<NCH>& r, float sc, int nvec, int lane) {
    u32x2* o = reinterpret_cast<u32x2*>(dst);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        int idx = lane + 64 * j;
        if (idx < nvec) o[idx] = (u32x2){pv_pack_bf16x2(r.v[j].x * sc, r.v[j].y * sc), pv_pack_bf16x2(r.v[j].z * sc, r.v[j].w * sc)};
    }
}

// ---- fp32 classification head: logits[B,C] = A[B,D] . w[C,D]^T + bias, ONE arithmetic per logit for pv_head_f32 and pv_exit_head_f32: a fused
// multiply-add chain over each 32-column K step (k ascending), the step sums added in order, then + bias -----------------------------------
#define PV_HEAD_TM 32          // rows of A per workgroup of the tiled form
// the tiled form's A loader: thread t stages row t >> 3 of the tile, four columns from (t & 7) << 2 of each K step
__device__ __forceinline__ int pv_head_a_row(int t) { return t >> 3; }
__device__ __forceinline__ int pv_head_a_col(int t) { return (t & 7) << 2; }

// 32 x 64 logits per workgroup of 256 threads, grid (ceil(C / 64), ceil(B / 32)); LDS-tiled, the NEXT K step's rows already in registers while
// this one is multiplied.  fetch_a(k0) returns the calling thread's float4 of K step k0: row blockIdx.y * 32 + pv_head_a_row(t), columns from
// k0 + pv_head_a_col(t); it is called only for a row below B and a column below D, everything else is zero padding (exact zeros in the sums).
template <typename FetchA>
__device__ __forceinline__ void pv_head_tile(FetchA fetch_a, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int B,
                                             int D, int C) {
    constexpr int BK = 32, TM = PV_HEAD_TM;
    __shared__ float As[BK][TM + 1];
    __shared__ float Ws[BK][65];
    const int t = threadIdx.x, tm = t >> 4, tn = t & 15;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * 64;
    float acc[2][4] = {};
    const int ar_ = pv_head_a_row(t), ak = pv_head_a_col(t);      // A loader: row ar_ (0..31), k offset ak (0..28)
    const int wr_ = t >> 2, wk = (t & 3) << 2;                  // W loader: row wr_ (0..63), k offsets wk and wk + 16
    const bool a_ok = m0 + ar_ < B, w_ok = n0 + wr_ < C;
    const float* wp = w + (int64_t)(w_ok ? n0 + wr_ : 0) * D + wk;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 av, wv[2];
    auto fetch = [&](int k0) {
        av = z4;
        if (a_ok && k0 + ak < D) av = fetch_a(k0);
#pragma unroll
        for (int h = 0; h < 2; ++h) wv[h] = (w_ok && k0 + wk + 16 * h < D) ? *reinterpret_cast<const float4*>(wp + k0 + 16 * h) : z4;
    };
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += BK) {
        As[ak + 0][ar_] = av.x; As[ak + 1][ar_] = av.y; As[ak + 2][ar_] = av.z; As[ak + 3][ar_] = av.w;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            Ws[16 * h + wk + 0][wr_] = wv[h].x; Ws[16 * h + wk + 1][wr_] = wv[h].y; Ws[16 * h + wk + 2][wr_] = wv[h].z; Ws[16 * h + wk + 3][wr_] = wv[h].w;
        }
        __syncthreads();
        if (k0 + BK < D) fetch(k0 + BK);
        float blk[2][4] = {};
#pragma unroll
        for (int k = 0; k < BK; ++k) {
            float ar[2], wr[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) ar[i] = As[k][tm + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) wr[j] = Ws[k][tn + 16 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) blk[i][j] = fmaf(ar[i], wr[j], blk[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __fadd_rn(acc[i][j], blk[i][j]);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m0 + tm + 16 * i;
        if (m >= B) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int n = n0 + tn + 16 * j;
            if (n < C) out[(int64_t)m * C + n] = acc[i][j] + (bias ? bias[n] : 0.f);
        }
    }
}

// one thread per logit (small batches): the tiled form's arithmetic, whose zero padding of a ragged last step adds exact zeros.  n4 = D / 4.
__device__ __forceinline__ float pv_head_dot(const float4* ar, const float4* __restrict__ wr, int n4) {
    float acc = 0.f;
    for (int k0 = 0; k0 < n4; k0 += 8) {
        float blk = 0.f;
        for (int k = k0; k < min(n4, k0 + 8); ++k) {
            const float4 av = ar[k], wv = wr[k];
            blk = fmaf(av.x, wv.x, blk); blk = fmaf(av.y, wv.y, blk); blk = fmaf(av.z, wv.z, blk); blk = fmaf(av.w, wv.w, blk);
        }
        acc = __fadd_rn(acc, blk);
    }
    return acc;
}

// ---- segment scan: per-image lengths -> segment table (A-ViT's pv_act_step, ResidualViT's pv_residual_pack_step) -----------------------
// seg_next[1 + b] holds image b's next length on entry, the inclusive prefix sum on exit; seg_next[0] = 0; totals = {rows in all, longest
// segment}.  One workgroup of 1024 threads, ceil(B / 1024) consecutive images per thread.  Templates (the parameter is unused), so
// only a file that calls pv_seg_scan instantiates the kernel.
template <int = 0>
__global__ __launch_bounds__(1024) void pv_seg_scan_kernel(int32_t* __restrict__ seg_next, int B, int32_t* __restrict__ totals) {
    __shared__ int wsum[16], wmax[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (B + 1023) / 1024, b0 = min(B, tid * per), b1 = min(B, b0 + per);
    int s = 0, mx = 0;
    for (int b = b0; b < b1; ++b) { s += seg_next[1 + b]; mx = max(mx, seg_next[1 + b]); }
    int incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (lane == 63) wsum[wave] = incl;
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    int run = base + incl - s;
    for (int b = b0; b < b1; ++b) { run += seg_next[1 + b]; seg_next[1 + b] = run; }
    if (tid == 0) seg_next[0] = 0;
    if (tid == 1023) {
        int m = 0;
        for (int w = 0; w < 16; ++w) m = max(m, wmax[w]);
        totals[0] = run;
        totals[1] = m;
    }
}

template <int = 0>
static inline int pv_seg_scan(int32_t* seg_next, int B, int32_t* totals, hipStream_t s) {
    PV_LAUNCH(pv_seg_scan_kernel<0>, dim3(1), dim3(1024), 0, s, seg_next, B, totals);
    return pv_check_launch();
}
