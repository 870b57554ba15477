// Routed top-1 mixture of experts (reference models/moevit.py, include/peekvit_hip_moe.h): the routing of one MoE layer and the gather of
// packed rows from per-expert planes.  The grouped GEMM that runs the experts is pv_gemm_grouped_bf16 in pv_gemm.hip.
//
// pv_moe_route = four launches, none of whose results depends on the order of concurrent work:
//   gate     one wave per row: LayerNorm (pv_ln_row_regs of pv_rows.h, which pv_layernorm_bf16 calls too), fp32 gate logits, argmax
//            (lowest index wins a tie), and per 256-row block the row count of every expert (integer LDS adds: the total does not depend
//            on their order);
//   scan     one workgroup: exclusive scan of the block counts per expert, segment offsets padded to 256 rows, block bases, tile table;
//   scatter  per 256-row block: a row's rank among the earlier rows of its block with the same expert -> its packed position (stable),
//            perm, and the 16-bit LayerNorm row written there;
//   pad      perm = -1 and zero 16-bit rows on every packed row no source row landed on.
#include "pv_rows.h"
#include "../../include/peekvit_hip_moe.h"

constexpr int MOE_RB = PV_MOE_TILE_ROWS;        // rows per histogram block (= the GEMM tile height: any value would do)

static inline int64_t pv_moe_blocks(int64_t M) { return (M + MOE_RB - 1) / MOE_RB; }

extern "C" int64_t pv_moe_packed_rows(int64_t M, int64_t E) {
    if (M <= 0 || E < 1 || E > PV_MOE_MAX_EXPERTS) return PV_ERR_INVALID_ARG;
    return (pv_moe_blocks(M) + E) * (int64_t)PV_MOE_TILE_ROWS;
}

// scratch: block counts -> block bases [nblk][E] int32, then the per-expert row counts [64] int32
extern "C" int64_t pv_moe_route_scratch_size(int64_t M, int64_t E) {
    if (M <= 0 || E < 1 || E > PV_MOE_MAX_EXPERTS) return PV_ERR_INVALID_ARG;
    const int64_t words = pv_moe_blocks(M) * E;
    return ((words + 3) / 4 * 4 + PV_MOE_MAX_EXPERTS) * 4;
}

template <int NCH>
__global__ __launch_bounds__(256) void pv_moe_gate_kernel(const float* __restrict__ x, int64_t ldx, int M, int D, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, const float* __restrict__ gw,
                                                          const float* __restrict__ gb, int E, int32_t* __restrict__ expert, float* __restrict__ gap,
                                                          float* __restrict__ probs, int32_t* __restrict__ blockcnt) {
    __shared__ int cnt[PV_MOE_MAX_EXPERTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    if (threadIdx.x < PV_MOE_MAX_EXPERTS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int r0 = blockIdx.x * MOE_RB, r1 = min(M, r0 + MOE_RB);
    float4 gm[NCH], bt[NCH];
    pv_ln_load_affine<NCH>(gm, bt, gamma, beta, nvec, lane);
    for (int row = r0 + wave; row < r1; row += 4) {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + (int64_t)row * ldx, nvec, lane);
        pv_ln_row_regs<NCH>(r, gm, bt, D, nvec, lane, eps);
        float best = -__builtin_inff(), second = -__builtin_inff();
        int bi = 0;
        for (int e = 0; e < E; ++e) {
            const float4* w = reinterpret_cast<const float4*>(gw + (int64_t)e * D);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int idx = lane + 64 * j;
                if (idx < nvec) {
                    const float4 wv = w[idx];
                    s = fmaf(r.v[j].x, wv.x, s); s = fmaf(r.v[j].y, wv.y, s); s = fmaf(r.v[j].z, wv.z, s); s = fmaf(r.v[j].w, wv.w, s);
                }
            }
            s = pv_wave_sum(s) + gb[e];
            if (e == 0 || s > best) { second = best; best = s; bi = e; }      // strict: the first of equal maxima stays
            else if (s > second) second = s;
        }
        if (lane == 0) {
            expert[row] = bi;
            if (gap) gap[row] = best - second;
            atomicAdd(&cnt[bi], 1);
        }
        if (probs && lane < E) probs[(int64_t)row * E + lane] = lane == bi ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x < E) blockcnt[(int64_t)blockIdx.x * E + threadIdx.x] = cnt[threadIdx.x];
}

// one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void pv_moe_scan_kernel(int32_t* __restrict__ blk, int nblk, int E, int32_t* __restrict__ counts,
                                                           int32_t* __restrict__ seg, int32_t* __restrict__ tile_expert, int ntiles) {
    __shared__ int wsum[16];
    __shared__ int s_seg[PV_MOE_MAX_EXPERTS + 1];
    __shared__ int s_tot[PV_MOE_MAX_EXPERTS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int e = 0; e < E; ++e) {
        int carry = 0;
        for (int base = 0; base < nblk; base += 1024) {
            const int i = base + t;
            const int v = i < nblk ? blk[(int64_t)i * E + e] : 0;
            int incl = v;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off, 64);
                if (lane >= off) incl += y;
            }
            if (lane == 63) wsum[w] = incl;
            __syncthreads();
            int before = 0, total = 0;
            for (int k = 0; k < 16; ++k) {
                const int s = wsum[k];
                before += k < w ? s : 0;
                total += s;
            }
            if (i < nblk) blk[(int64_t)i * E + e] = carry + before + incl - v;      // exclusive, relative to the segment start
            carry += total;
            __syncthreads();                                                        // (wsum is rewritten by the next chunk)
        }
        if (t == 0) s_tot[e] = carry;
    }
    __syncthreads();
    if (t == 0) {
        int o = 0;
        for (int e = 0; e < E; ++e) {
            s_seg[e] = o;
            seg[e] = o;
            counts[e] = s_tot[e];
            o += (s_tot[e] + PV_MOE_TILE_ROWS - 1) / PV_MOE_TILE_ROWS * PV_MOE_TILE_ROWS;
        }
        s_seg[E] = o;
        seg[E] = o;
    }
    __syncthreads();
    for (int64_t i = t; i < (int64_t)nblk * E; i += 1024) blk[i] += s_seg[(int)(i % E)];
    for (int tt = t; tt < ntiles; tt += 1024) {
        const int row = tt * PV_MOE_TILE_ROWS;
        int ex = -1;
        for (int e = 0; e < E; ++e)
            if (row >= s_seg[e] && row < s_seg[e + 1]) ex = e;
        tile_expert[tt] = ex;
    }
}

template <int NCH>
__global__ __launch_bounds__(256) void pv_moe_scatter_kernel(const float* __restrict__ x, int64_t ldx, int M, int D, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, int E, const int32_t* __restrict__ expert,
                                                             const int32_t* __restrict__ bases, int32_t* __restrict__ perm, uint16_t* __restrict__ xln) {
    __shared__ int ex[MOE_RB];
    __shared__ int dst[MOE_RB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nvec = D >> 2;
    const int r0 = blockIdx.x * MOE_RB, r1 = min(M, r0 + MOE_RB);
    const int row = r0 + t;
    int e = row < r1 ? expert[row] : -1;
    e = e < E ? e : E - 1;                      // (defensive: an id out of range goes to the last expert instead of off the tables)
    ex[t] = e;
    __syncthreads();
    if (row < r1) {
        int rank = 0;
        for (int j = 0; j < t; ++j) rank += ex[j] == e ? 1 : 0;
        const int d = bases[(int64_t)blockIdx.x * E + e] + rank;
        dst[t] = d;
        perm[d] = row;
    }
    if (!xln) return;
    __syncthreads();
    float4 gm[NCH], bt[NCH];
    pv_ln_load_affine<NCH>(gm, bt, gamma, beta, nvec, lane);
    for (int k = wave; k < r1 - r0; k += 4) {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + (int64_t)(r0 + k) * ldx, nvec, lane);
        pv_ln_row_regs<NCH>(r, gm, bt, D, nvec, lane, eps);
        pv_store_row16<NCH>(xln + (int64_t)dst[k] * D, r, nvec, lane);
    }
}

// block b < E: the pad rows of segment b; blocks E .. gridDim.x - 1 share the rows behind the last segment
__global__ __launch_bounds__(256) void pv_moe_pad_kernel(const int32_t* __restrict__ seg, const int32_t* __restrict__ counts, int E, int64_t M_pad,
                                                         int D, int32_t* __restrict__ perm, uint16_t* __restrict__ xln) {
    int64_t lo, hi, step, first;
    if ((int)blockIdx.x < E) {
        lo = seg[blockIdx.x] + counts[blockIdx.x]; hi = seg[blockIdx.x + 1]; first = 0; step = 1;
    } else {
        lo = seg[E]; hi = M_pad; first = blockIdx.x - E; step = gridDim.x - E;
    }
    hi = hi < M_pad ? hi : M_pad;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n8 = D >> 2;       // u32x2 chunks per row
    for (int64_t p = lo + first * 256 + t; p < hi; p += step * 256) perm[p] = -1;
    if (!xln) return;
    for (int64_t p = lo + first * 4 + wave; p < hi; p += step * 4) {
        u32x2* o = reinterpret_cast<u32x2*>(xln + p * D);
        for (int c = lane; c < n8; c += 64) o[c] = (u32x2){0u, 0u};
    }
}

extern "C" int pv_moe_route(const float* x, int64_t ldx, int64_t M, int64_t D, const float* ln_gamma, const float* ln_beta, float ln_eps,
                            const float* gate_w, const float* gate_b, int64_t E, int32_t* expert, float* gap, float* probs, int32_t* seg, int32_t* perm,
                            int32_t* tile_expert, uint16_t* xln, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!x || !ln_gamma || !ln_beta || !gate_w || !gate_b || !expert || !seg || !perm || !tile_expert || !scratch) return PV_ERR_INVALID_ARG;
    if (M <= 0 || D <= 0 || E < 1 || E > PV_MOE_MAX_EXPERTS) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096 || M >= 0x7fffffff - (1 << 24)) return PV_ERR_UNSUPPORTED;
    if (ldx % 4 || ldx < D) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x | (uintptr_t)ln_gamma | (uintptr_t)ln_beta | (uintptr_t)gate_w | (uintptr_t)scratch) & 15) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)gate_b | (uintptr_t)expert | (uintptr_t)seg | (uintptr_t)perm | (uintptr_t)tile_expert) & 3) return PV_ERR_INVALID_ARG;
    if ((gap && ((uintptr_t)gap & 3)) || (probs && ((uintptr_t)probs & 3)) || (xln && ((uintptr_t)xln & 7))) return PV_ERR_INVALID_ARG;
    if (scratch_bytes < pv_moe_route_scratch_size(M, E)) return PV_ERR_INVALID_ARG;
    const int64_t nblk = pv_moe_blocks(M), M_pad = pv_moe_packed_rows(M, E);
    int32_t* blk = reinterpret_cast<int32_t*>(scratch);
    int32_t* counts = blk + (nblk * E + 3) / 4 * 4;
    hipStream_t s = (hipStream_t)stream;
#define GATE_LAUNCH(N) PV_LAUNCH(pv_moe_gate_kernel<N>, dim3((unsigned)nblk), dim3(256), 0, s, x, ldx, (int)M, (int)D, ln_gamma, ln_beta, ln_eps, gate_w, \
                                 gate_b, (int)E, expert, gap, probs, blk)
    PV_DISPATCH_NCH(D, GATE_LAUNCH);
#undef GATE_LAUNCH
    int rc = pv_check_launch();
    if (rc) return rc;
    PV_LAUNCH(pv_moe_scan_kernel, dim3(1), dim3(1024), 0, s, blk, (int)nblk, (int)E, counts, seg, tile_expert, (int)(M_pad / PV_MOE_TILE_ROWS));
    if ((rc = pv_check_launch())) return rc;
#define SCAT_LAUNCH(N) PV_LAUNCH(pv_moe_scatter_kernel<N>, dim3((unsigned)nblk), dim3(256), 0, s, x, ldx, (int)M, (int)D, ln_gamma, ln_beta, ln_eps, \
                                 (int)E, expert, blk, perm, xln)
    PV_DISPATCH_NCH(D, SCAT_LAUNCH);
#undef SCAT_LAUNCH
    if ((rc = pv_check_launch())) return rc;
    PV_LAUNCH(pv_moe_pad_kernel, dim3((unsigned)(E + 32)), dim3(256), 0, s, seg, counts, (int)E, M_pad, (int)D, perm, xln);
    return pv_check_launch();
}

// packed row p, 16-byte chunk c: one thread per chunk, grid-stride
__global__ __launch_bounds__(256) void pv_moe_gather_kernel(const uint16_t* __restrict__ src, int64_t plane_stride, int64_t ld,
                                                            const int32_t* __restrict__ expert, const int32_t* __restrict__ perm, int M, int E,
                                                            int64_t M_pad, int D, uint16_t* __restrict__ out) {
    const int nc = D >> 3;
    const int64_t total = M_pad * nc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i / nc;
        const int c = (int)(i - p * nc);
        const int sr = perm[p];
        u32x4 v = {0u, 0u, 0u, 0u};
        if (sr >= 0 && sr < M) {
            int e = expert[sr];
            e = e < 0 ? 0 : (e < E ? e : E - 1);
            v = *reinterpret_cast<const u32x4*>(src + (int64_t)e * plane_stride + (int64_t)sr * ld + c * 8);
        }
        *reinterpret_cast<u32x4*>(out + p * D + c * 8) = v;
    }
}

extern "C" int pv_moe_gather_bf16(const uint16_t* src, int64_t plane_stride, int64_t ld, const int32_t* expert, const int32_t* perm, int64_t M,
                                  int64_t M_pad, int64_t D, int64_t E, uint16_t* out, void* stream) {
    if (!src || !expert || !perm || !out || M <= 0 || M_pad <= 0 || D <= 0 || E < 1 || E > PV_MOE_MAX_EXPERTS) return PV_ERR_INVALID_ARG;
    if (M > 0x7fffffff || M_pad > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (D % 8 || ld % 8 || ld < D || plane_stride < M * ld || plane_stride % 8) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)src & 15) || ((uintptr_t)out & 15) || ((uintptr_t)expert & 3) || ((uintptr_t)perm & 3)) return PV_ERR_INVALID_ARG;
    PV_LAUNCH(pv_moe_gather_kernel, dim3(pv_stream_grid(M_pad * (D / 8), 256)), dim3(256), 0, (hipStream_t)stream, src, plane_stride, ld, expert, perm,
              (int)M, (int)E, M_pad, (int)D, out);
    return pv_check_launch();
}
