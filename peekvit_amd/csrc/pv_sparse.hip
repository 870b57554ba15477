// ResidualViT exact token compaction (include/peekvit_hip_sparse.h): the gate of one block on the PACKED row matrix and
// the compaction that writes the next packed input.
//
// Image b is the row segment [seg[b], seg[b+1]) of x: its class row first, its budget row last, in between one row per live token and one
// row per class of tokens that were masked together in an earlier block (mult = how many tokens the row stands for).  Three launches:
//   gate     one workgroup per image: threshold from the budget row, the mask of every row (one wave per row; pv_rows.h's gate functions,
//            which pv_residual_gate calls too), the dense mask through tok_row, and the next segment length;
//   scan     one workgroup: lengths -> next segment table and the totals word (pv_seg_scan, pv_rows.h);
//   compact  one workgroup per image: stable compaction (class row | rows with mask > 0 | one zero row for all rows with mask 0 | budget
//            row), the row tables, mask * x and - from the same registers - row_scale * LayerNorm 1 of the written row.
// Nothing depends on the order of concurrent work.
#include "pv_rows.h"
#include "../../include/peekvit_hip_sparse.h"
#include "../../include/peekvit_hip_sparse_train.h"

#define PV_SP_MAXL 256          // rows of one segment the kernels can hold (one thread per row); the entry point admits PV_SPARSE_MAX_LEN

// TRAIN (pv_residual_pack_step_train, include/peekvit_hip_sparse_train.h): the same arithmetic; the sigmoid's argument of every row also goes to gate_arg
template <int NCH, bool TRAIN = false>
__global__ __launch_bounds__(256) void pv_sp_gate_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ tok_row,
                                                         int N, int D, const float* __restrict__ wg, const float* __restrict__ bg,
                                                         const float* __restrict__ wb, const float* __restrict__ bb, float temp, float sbias,
                                                         float* __restrict__ mask_row, float* __restrict__ mask_out, float* __restrict__ thr_out,
                                                         int32_t* __restrict__ len_next, float* __restrict__ gate_arg = nullptr) {
    __shared__ float thr_s;
    __shared__ float smask[PV_SP_MAXL];
    __shared__ int wlive[4], wdead[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0;
    if (L < 2 || L > PV_SP_MAXL) {          // (workgroup-uniform; a table this library did not write: the image drops out instead of indexing past LDS)
        if (tid == 0) len_next[b] = 0;
        return;
    }
    if (wave == 0) {   // threshold from the budget row (the segment's last), models/residualvit.py:212
        const float s = pv_gate_budget_dot(x + (int64_t)(s0 + L - 1) * D, wb, bb, nvec, lane);
        if (lane == 0) {
            thr_s = pv_sigmoid(s);
            thr_out[b] = thr_s;
        }
    }
    __syncthreads();
    const float thr = thr_s;
    for (int i = wave; i < L; i += 4) {
        float m = 1.0f, t = 0.f;                         // class row, budget row: scale 1
        if (i != 0 && i != L - 1) {
            RowRegs<NCH> r;
            pv_load_row<NCH>(r, x + (int64_t)(s0 + i) * D, nvec, lane);
            if constexpr (TRAIN) {                       // (pv_gate_mask's two steps, with the argument kept)
                t = pv_gate_arg<NCH>(r, wg, bg, temp, sbias, nvec, lane);
                m = fmaxf(pv_sigmoid(t) - thr, 0.f);
            } else {
                m = pv_gate_mask<NCH>(r, wg, bg, temp, sbias, thr, nvec, lane);
            }
        }
        if (lane == 0) {
            smask[i] = m;
            if constexpr (TRAIN) gate_arg[s0 + i] = t;
        }
    }
    __syncthreads();
    bool live = false, dead = false;
    if (tid < L) {
        const float m = smask[tid];
        mask_row[s0 + tid] = m;
        const bool mid = tid != 0 && tid != L - 1;
        live = mid && m > 0.f;
        dead = mid && !(m > 0.f);
    }
    const unsigned long long bl = __ballot(live), bd = __ballot(dead);
    if (lane == 0) { wlive[wave] = __popcll(bl); wdead[wave] = __popcll(bd); }
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        rrow = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        mask_out[(int64_t)b * N + t] = smask[rrow];
    }
    __syncthreads();
    if (tid == 0) {
        const int nl = wlive[0] + wlive[1] + wlive[2] + wlive[3], nd = wdead[0] + wdead[1] + wdead[2] + wdead[3];
        len_next[b] = 2 + nl + (nd > 0 ? 1 : 0);
    }
}

// TRAIN: the source row of every written row (relative to the segment start; -1 for the zero row) also goes to src_next
template <int NCH, bool LN, bool TRAIN = false>
__global__ __launch_bounds__(256) void pv_sp_compact_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ mult,
                                                            const int32_t* __restrict__ tok_row, int N, int D, const float* __restrict__ mask_row,
                                                            const int32_t* __restrict__ seg_next, float* __restrict__ x_next,
                                                            float* __restrict__ rs_next, int32_t* __restrict__ mult_next, float* __restrict__ lm_next,
                                                            int32_t* __restrict__ tok_row_next, const float* __restrict__ ln_gamma,
                                                            const float* __restrict__ ln_beta, float ln_eps, uint16_t* __restrict__ ln_out,
                                                            int32_t* __restrict__ src_next = nullptr) {
    __shared__ int wkeep[4], wdead[4], wdmult[4];
    __shared__ int src[PV_SP_MAXL], newidx[PV_SP_MAXL];
    __shared__ float sscale[PV_SP_MAXL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0, d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    if (L < 2 || L > PV_SP_MAXL || Ln < 2 || Ln > L) return;          // (workgroup-uniform: the gate kernel gave such an image length 0)
    float m = 0.f;
    int mu = 0;
    bool keep = false, dead = false;
    if (tid < L) {
        m = mask_row[s0 + tid];
        mu = mult[s0 + tid];
        keep = tid == 0 || (tid < L - 1 && m > 0.f);      // the budget row is placed behind the zero row, below
        dead = tid != 0 && tid < L - 1 && !(m > 0.f);
    }
    const unsigned long long bk = __ballot(keep), bd = __ballot(dead);
    const int before = __popcll(bk & ((1ull << lane) - 1ull));
    int dm = dead ? mu : 0;
    for (int o = 32; o > 0; o >>= 1) dm += __shfl_xor(dm, o, 64);
    if (lane == 0) { wkeep[wave] = __popcll(bk); wdead[wave] = __popcll(bd); wdmult[wave] = dm; }
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wkeep[w];
    const int nkeep = wkeep[0] + wkeep[1] + wkeep[2] + wkeep[3];
    const int ndead = wdead[0] + wdead[1] + wdead[2] + wdead[3];
    const int zi = ndead > 0 ? nkeep : -1;                 // the zero row's place
    const int bi = nkeep + (ndead > 0 ? 1 : 0);            // the budget row's place (= Ln - 1)
    if (bi != Ln - 1) return;                              // (uniform: tables that do not belong together)
    if (tid < L) {
        int j;
        if (keep) j = base + before;                       // stable: kept rows stay in order
        else if (tid == L - 1) j = bi;
        else j = zi;
        newidx[tid] = j;
        if (keep || tid == L - 1) {
            const bool special = tid == 0 || tid == L - 1;
            src[j] = tid;
            sscale[j] = special ? 1.0f : m;
            rs_next[d0 + j] = special ? 1.0f : m;
            mult_next[d0 + j] = mu;
            lm_next[d0 + j] = logf((float)mu);
        }
    }
    if (tid == 0 && zi >= 0) {
        const int zm = wdmult[0] + wdmult[1] + wdmult[2] + wdmult[3];
        src[zi] = -1;
        sscale[zi] = 0.f;
        rs_next[d0 + zi] = 0.f;
        mult_next[d0 + zi] = zm;
        lm_next[d0 + zi] = logf((float)zm);
    }
    __syncthreads();
    if constexpr (TRAIN)
        if (tid < Ln) src_next[d0 + tid] = src[tid];
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        rrow = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        tok_row_next[(int64_t)b * N + t] = newidx[rrow];
    }
    float4 gm[LN ? NCH : 1], bt[LN ? NCH : 1];
    if constexpr (LN) pv_ln_load_affine<NCH>(gm, bt, ln_gamma, ln_beta, nvec, lane);
    for (int j = wave; j < Ln; j += 4) {
        const int i = src[j];
        float* const xw = x_next + (int64_t)(d0 + j) * D;
        if (i < 0) {                                       // the zero row: mask * x = 0, and 0 * LayerNorm(0 row) = 0
            for (int v = lane; v < nvec; v += 64) reinterpret_cast<float4*>(xw)[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (LN) {
                u32x2* o = reinterpret_cast<u32x2*>(ln_out + (int64_t)(d0 + j) * D);
                for (int v = lane; v < nvec; v += 64) o[v] = (u32x2){0u, 0u};
            }
            continue;
        }
        const float sc = sscale[j];
        const bool special = i == 0 || i == L - 1;
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + (int64_t)(s0 + i) * D, nvec, lane);
        if (!special) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) { r.v[k].x *= sc; r.v[k].y *= sc; r.v[k].z *= sc; r.v[k].w *= sc; }
        }
        pv_store_row<NCH>(xw, r, nvec, lane);
        if constexpr (LN) {      // the block's first LayerNorm on the row just written, times its scale (residualvit.py:251)
            pv_ln_row_regs<NCH>(r, gm, bt, D, nvec, lane, ln_eps);
            pv_store_row16_scaled<NCH>(ln_out + (int64_t)(d0 + j) * D, r, sc, nvec, lane);
        }
    }
}

// the three launches of one step; TRAIN: with the two tables the backward reads (gate_arg [R], src_next [R'])
template <bool TRAIN>
static int pv_pack_step_launch(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                               const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                               float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next, int32_t* tok_row_next,
                               float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta, float ln_eps,
                               uint16_t* ln_out, float* gate_arg, int32_t* src_next, hipStream_t s) {
    dim3 grid((unsigned)B);
#define SPG_LAUNCH(NC) PV_LAUNCH((pv_sp_gate_kernel<NC, TRAIN>), grid, dim3(256), 0, s, x, seg_start, tok_row, (int)N, (int)D, wg, bg, wb, bb, temp, sigmoid_bias, \
                                 mask_row, mask_out, thr_out, seg_next + 1, gate_arg)
    PV_DISPATCH_NCH(D, SPG_LAUNCH);
#undef SPG_LAUNCH
    int rc = pv_check_launch();
    if (rc != PV_OK) return rc;
    if ((rc = pv_seg_scan(seg_next, (int)B, totals, s)) != PV_OK) return rc;
#define SPC_LAUNCH(NC) do { if (ln_out) PV_LAUNCH((pv_sp_compact_kernel<NC, true, TRAIN>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D, mask_row, \
                                                  seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out, src_next); \
                            else PV_LAUNCH((pv_sp_compact_kernel<NC, false, TRAIN>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D, mask_row,        \
                                           seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out, src_next); } while (0)
    PV_DISPATCH_NCH(D, SPC_LAUNCH);
#undef SPC_LAUNCH
    return pv_check_launch();
}

static int pv_pack_step_check(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                              const float* wg, const float* bg, const float* wb, const float* bb, float temp, float* mask_row, float* x_next,
                              float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next, int32_t* tok_row_next, float* mask_out,
                              float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta, uint16_t* ln_out) {
    if (!x || !seg_start || !mult || !tok_row || !wg || !bg || !wb || !bb || !mask_row || !x_next || !row_scale_next || !mult_next || !log_mult_next ||
        !seg_next || !tok_row_next || !mask_out || !thr_out || !totals || B <= 0 || N < 0 || D <= 0 || temp == 0.f)
        return PV_ERR_INVALID_ARG;
    if (ln_out && (!ln_gamma || !ln_beta)) return PV_ERR_INVALID_ARG;
    if (x == x_next) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096 || N + 2 > PV_SPARSE_MAX_LEN || B > 0x7fffffff || ((uintptr_t)x & 15) || ((uintptr_t)x_next & 15) || ((uintptr_t)wg & 15) ||
        ((uintptr_t)wb & 15))
        return PV_ERR_UNSUPPORTED;
    if (ln_out && (((uintptr_t)ln_gamma & 15) || ((uintptr_t)ln_beta & 15) || ((uintptr_t)ln_out & 7))) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

extern "C" int pv_residual_pack_step(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                                     const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                                     float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                                     int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma, const float* ln_beta,
                                     float ln_eps, uint16_t* ln_out, void* stream) {
    const int rc = pv_pack_step_check(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, mask_row, x_next, row_scale_next, mult_next, log_mult_next,
                                      seg_next, tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_out);
    if (rc != PV_OK) return rc;
    return pv_pack_step_launch<false>(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, sigmoid_bias, mask_row, x_next, row_scale_next, mult_next,
                                      log_mult_next, seg_next, tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_eps, ln_out, nullptr, nullptr,
                                      (hipStream_t)stream);
}

// The same step for training (include/peekvit_hip_sparse_train.h): the TRAIN instantiations of the two kernels above, which also leave the tables
// pv_residual_pack_step_bwd reads.
extern "C" int pv_residual_pack_step_train(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                                           const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                                           float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                                           int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma,
                                           const float* ln_beta, float ln_eps, uint16_t* ln_out, float* gate_arg, int32_t* src_next, void* stream) {
    if (!gate_arg || !src_next) return PV_ERR_INVALID_ARG;
    const int rc = pv_pack_step_check(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, mask_row, x_next, row_scale_next, mult_next, log_mult_next,
                                      seg_next, tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_out);
    if (rc != PV_OK) return rc;
    return pv_pack_step_launch<true>(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, sigmoid_bias, mask_row, x_next, row_scale_next, mult_next,
                                     log_mult_next, seg_next, tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_eps, ln_out, gate_arg, src_next,
                                     (hipStream_t)stream);
}
