// ResidualViT exact token compaction past PV_SPARSE_MAX_LEN rows (include/peekvit_hip_sparse_long.h): pv_sparse.hip's gate +
// compaction step for segments of up to PV_SPARSE_LONG_MAX_LEN rows.  The same three launches (gate, pv_seg_scan, compact), one workgroup of 256
// threads per image; where pv_sparse.hip gives every row of a segment one thread, these kernels walk the segment in chunks of 256 rows and carry
// the number of rows kept so far from chunk to chunk, so the compaction stays stable (class row | live rows in order | one zero row | budget row).
// Every row's arithmetic - threshold, mask, mask * x, LayerNorm 1 - is pv_rows.h's, called as pv_sparse.hip calls it: at N + 2 <= PV_SPARSE_MAX_LEN
// every output has pv_residual_pack_step's bits.  The per-segment tables live in LDS: the masks as fp32 (gate, 16 KiB), the two row maps as
// 16-bit indices (compact, 2 x 8 KiB); a written row's scale is read back from mask_row.  Nothing depends on the order of concurrent work.
// The TRAIN instantiations (pv_residual_pack_step_long_train, include/peekvit_hip_sparse_long_train.h, section 35) also leave gate_arg and src_next.
#include "pv_rows.h"
#include "../../include/peekvit_hip_sparse_long_train.h"

#define PV_SPL_MAXL PV_SPARSE_LONG_MAX_LEN      // rows of one segment the LDS tables hold
#define PV_SPL_CHUNK 256                        // rows per step of the walk (one thread per row)
#define PV_SPL_NONE 0xffffu                     // src of the zero row (no row index reaches it: PV_SPL_MAXL <= 0xffff)

// sum of one int per wave over the workgroup's four waves (every thread gets it); `slot` is the caller's __shared__ int[4]
__device__ __forceinline__ int pv_spl_block_sum(int v, int* slot, int lane, int wave) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                             // the slot's previous readers are done
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    return slot[0] + slot[1] + slot[2] + slot[3];
}

// ONE body for the inference kernel and the training one (TRAIN: pv_residual_pack_step_long_train, include/peekvit_hip_sparse_long_train.h - the same
// arithmetic; the sigmoid's argument of every row also goes to gate_arg, as pv_sparse.hip's TRAIN).  Two __global__ functions wrap it, so the inference
// kernel keeps its name and its code.
template <int NCH, bool TRAIN>
__device__ __forceinline__ void pv_spl_gate_body(const float* x, const int32_t* seg, const int32_t* tok_row,
                                                 int N, int D, const float* wg, const float* bg,
                                                 const float* wb, const float* bb, float temp, float sbias,
                                                 float* mask_row, float* mask_out, float* thr_out,
                                                 int32_t* len_next, float* gate_arg) {
    __shared__ float thr_s;
    __shared__ float smask[PV_SPL_MAXL];
    __shared__ int slot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0;
    if (L < 2 || L > PV_SPL_MAXL) {          // (workgroup-uniform; a table this library did not write: the image drops out instead of indexing past LDS)
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
    int nlive = 0, ndead = 0;                            // this thread's rows, one per chunk
    for (int i = tid; i < L; i += PV_SPL_CHUNK) {
        const float m = smask[i];
        mask_row[s0 + i] = m;
        const bool mid = i != 0 && i != L - 1;
        nlive += mid && m > 0.f;
        ndead += mid && !(m > 0.f);
    }
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        rrow = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        mask_out[(int64_t)b * N + t] = smask[rrow];
    }
    const int nl = pv_spl_block_sum(nlive, slot, lane, wave), nd = pv_spl_block_sum(ndead, slot, lane, wave);
    if (tid == 0) len_next[b] = 2 + nl + (nd > 0 ? 1 : 0);
}

template <int NCH>
__global__ __launch_bounds__(256) void pv_spl_gate_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ tok_row,
                                                          int N, int D, const float* __restrict__ wg, const float* __restrict__ bg,
                                                          const float* __restrict__ wb, const float* __restrict__ bb, float temp, float sbias,
                                                          float* __restrict__ mask_row, float* __restrict__ mask_out, float* __restrict__ thr_out,
                                                          int32_t* __restrict__ len_next) {
    pv_spl_gate_body<NCH, false>(x, seg, tok_row, N, D, wg, bg, wb, bb, temp, sbias, mask_row, mask_out, thr_out, len_next, nullptr);
}

template <int NCH>
__global__ __launch_bounds__(256) void pv_spl_gate_train_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ tok_row,
                                                                int N, int D, const float* __restrict__ wg, const float* __restrict__ bg,
                                                                const float* __restrict__ wb, const float* __restrict__ bb, float temp, float sbias,
                                                                float* __restrict__ mask_row, float* __restrict__ mask_out, float* __restrict__ thr_out,
                                                                int32_t* __restrict__ len_next, float* __restrict__ gate_arg) {
    pv_spl_gate_body<NCH, true>(x, seg, tok_row, N, D, wg, bg, wb, bb, temp, sbias, mask_row, mask_out, thr_out, len_next, gate_arg);
}

// ONE body again.  TRAIN: the source row of every written row (relative to the segment start; -1 for the zero row) also goes to src_next - the 16-bit
// map in LDS holds it already.
template <int NCH, bool LN, bool TRAIN>
__device__ __forceinline__ void pv_spl_compact_body(const float* x, const int32_t* seg, const int32_t* mult,
                                                    const int32_t* tok_row, int N, int D, const float* mask_row,
                                                    const int32_t* seg_next, float* x_next,
                                                    float* rs_next, int32_t* mult_next, float* lm_next,
                                                    int32_t* tok_row_next, const float* ln_gamma,
                                                    const float* ln_beta, float ln_eps, uint16_t* ln_out,
                                                    int32_t* src_next) {
    __shared__ int slot[4];
    __shared__ int wkeep[2][4];                          // kept rows of the chunk per wave, double-buffered over the chunks
    __shared__ uint16_t src[PV_SPL_MAXL], newidx[PV_SPL_MAXL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0, d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    if (L < 2 || L > PV_SPL_MAXL || Ln < 2 || Ln > L) return;          // (workgroup-uniform: the gate kernel gave such an image length 0)
    // first walk: how many rows are kept, how many collapse, and how many tokens the collapsing rows stand for
    int ck = 0, cd = 0, cm = 0;
    for (int i = tid; i < L; i += PV_SPL_CHUNK) {
        const float m = mask_row[s0 + i];
        const bool mid = i != 0 && i < L - 1;
        const bool dead = mid && !(m > 0.f);
        ck += i == 0 || (mid && m > 0.f);
        cd += dead;
        cm += dead ? mult[s0 + i] : 0;
    }
    const int nkeep = pv_spl_block_sum(ck, slot, lane, wave), ndead = pv_spl_block_sum(cd, slot, lane, wave);
    const int zm = pv_spl_block_sum(cm, slot, lane, wave);
    const int zi = ndead > 0 ? nkeep : -1;                 // the zero row's place
    const int bi = nkeep + (ndead > 0 ? 1 : 0);            // the budget row's place (= Ln - 1)
    if (bi != Ln - 1) return;                              // (uniform: tables that do not belong together)
    // second walk: the places, chunk by chunk, `carry` = rows kept in the chunks before
    int carry = 0;
    for (int c0 = 0, it = 0; c0 < L; c0 += PV_SPL_CHUNK, ++it) {
        const int i = c0 + tid;
        float m = 0.f;
        int mu = 0;
        bool keep = false;
        if (i < L) {
            m = mask_row[s0 + i];
            mu = mult[s0 + i];
            keep = i == 0 || (i < L - 1 && m > 0.f);       // the budget row is placed behind the zero row, below
        }
        const unsigned long long bk = __ballot(keep);
        const int before = __popcll(bk & ((1ull << lane) - 1ull));
        int* const wk = wkeep[it & 1];                     // (the other buffer may still be read by a wave that is one chunk behind)
        if (lane == 0) wk[wave] = __popcll(bk);
        __syncthreads();
        int base = carry;
        for (int w = 0; w < wave; ++w) base += wk[w];
        carry += wk[0] + wk[1] + wk[2] + wk[3];
        if (i < L) {
            int j;
            if (keep) j = base + before;                   // stable: kept rows stay in order
            else if (i == L - 1) j = bi;
            else j = zi;
            newidx[i] = (uint16_t)j;
            if (keep || i == L - 1) {
                const bool special = i == 0 || i == L - 1;
                src[j] = (uint16_t)i;
                rs_next[d0 + j] = special ? 1.0f : m;
                mult_next[d0 + j] = mu;
                lm_next[d0 + j] = logf((float)mu);
            }
        }
    }
    if (tid == 0 && zi >= 0) {
        src[zi] = (uint16_t)PV_SPL_NONE;
        rs_next[d0 + zi] = 0.f;
        mult_next[d0 + zi] = zm;
        lm_next[d0 + zi] = logf((float)zm);
    }
    __syncthreads();
    if constexpr (TRAIN) {
        for (int j = tid; j < Ln; j += 256) {
            const unsigned i = src[j];
            src_next[d0 + j] = i == PV_SPL_NONE ? -1 : (int)i;
        }
    }
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        rrow = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        tok_row_next[(int64_t)b * N + t] = newidx[rrow];
    }
    float4 gm[LN ? NCH : 1], bt[LN ? NCH : 1];
    if constexpr (LN) pv_ln_load_affine<NCH>(gm, bt, ln_gamma, ln_beta, nvec, lane);
    for (int j = wave; j < Ln; j += 4) {
        const unsigned i = src[j];
        float* const xw = x_next + (int64_t)(d0 + j) * D;
        if (i == PV_SPL_NONE) {                            // the zero row: mask * x = 0, and 0 * LayerNorm(0 row) = 0
            for (int v = lane; v < nvec; v += 64) reinterpret_cast<float4*>(xw)[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (LN) {
                u32x2* o = reinterpret_cast<u32x2*>(ln_out + (int64_t)(d0 + j) * D);
                for (int v = lane; v < nvec; v += 64) o[v] = (u32x2){0u, 0u};
            }
            continue;
        }
        const bool special = i == 0u || i == (unsigned)(L - 1);
        const float sc = special ? 1.0f : mask_row[s0 + (int)i];
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + (int64_t)(s0 + (int)i) * D, nvec, lane);
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

template <int NCH, bool LN>
__global__ __launch_bounds__(256) void pv_spl_compact_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ mult,
                                                             const int32_t* __restrict__ tok_row, int N, int D, const float* __restrict__ mask_row,
                                                             const int32_t* __restrict__ seg_next, float* __restrict__ x_next,
                                                             float* __restrict__ rs_next, int32_t* __restrict__ mult_next, float* __restrict__ lm_next,
                                                             int32_t* __restrict__ tok_row_next, const float* __restrict__ ln_gamma,
                                                             const float* __restrict__ ln_beta, float ln_eps, uint16_t* __restrict__ ln_out) {
    pv_spl_compact_body<NCH, LN, false>(x, seg, mult, tok_row, N, D, mask_row, seg_next, x_next, rs_next, mult_next, lm_next, tok_row_next, ln_gamma, ln_beta,
                                        ln_eps, ln_out, nullptr);
}

template <int NCH, bool LN>
__global__ __launch_bounds__(256) void pv_spl_compact_train_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ mult,
                                                                   const int32_t* __restrict__ tok_row, int N, int D, const float* __restrict__ mask_row,
                                                                   const int32_t* __restrict__ seg_next, float* __restrict__ x_next,
                                                                   float* __restrict__ rs_next, int32_t* __restrict__ mult_next, float* __restrict__ lm_next,
                                                                   int32_t* __restrict__ tok_row_next, const float* __restrict__ ln_gamma,
                                                                   const float* __restrict__ ln_beta, float ln_eps, uint16_t* __restrict__ ln_out,
                                                                   int32_t* __restrict__ src_next) {
    pv_spl_compact_body<NCH, LN, true>(x, seg, mult, tok_row, N, D, mask_row, seg_next, x_next, rs_next, mult_next, lm_next, tok_row_next, ln_gamma, ln_beta,
                                       ln_eps, ln_out, src_next);
}

// (pv_residual_pack_step's checks with this header's row limit)
static int pv_spl_check(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D, const float* wg,
                        const float* bg, const float* wb, const float* bb, float temp, float* mask_row, float* x_next, float* row_scale_next,
                        int32_t* mult_next, float* log_mult_next, int32_t* seg_next, int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals,
                        const float* ln_gamma, const float* ln_beta, uint16_t* ln_out) {
    if (!x || !seg_start || !mult || !tok_row || !wg || !bg || !wb || !bb || !mask_row || !x_next || !row_scale_next || !mult_next || !log_mult_next ||
        !seg_next || !tok_row_next || !mask_out || !thr_out || !totals || B <= 0 || N < 0 || D <= 0 || temp == 0.f)
        return PV_ERR_INVALID_ARG;
    if (ln_out && (!ln_gamma || !ln_beta)) return PV_ERR_INVALID_ARG;
    if (x == x_next) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096 || N + 2 > PV_SPARSE_LONG_MAX_LEN || B > 0x7fffffff || ((uintptr_t)x & 15) || ((uintptr_t)x_next & 15) || ((uintptr_t)wg & 15) ||
        ((uintptr_t)wb & 15))
        return PV_ERR_UNSUPPORTED;
    if (ln_out && (((uintptr_t)ln_gamma & 15) || ((uintptr_t)ln_beta & 15) || ((uintptr_t)ln_out & 7))) return PV_ERR_UNSUPPORTED;
    return PV_OK;
}

extern "C" int pv_residual_pack_step_long(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N, int64_t D,
                                          const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias, float* mask_row,
                                          float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next, int32_t* seg_next,
                                          int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals, const float* ln_gamma,
                                          const float* ln_beta, float ln_eps, uint16_t* ln_out, void* stream) {
    int rc = pv_spl_check(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, mask_row, x_next, row_scale_next, mult_next, log_mult_next, seg_next,
                          tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_out);
    if (rc != PV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)B);
#define SPLG_LAUNCH(NC) PV_LAUNCH((pv_spl_gate_kernel<NC>), grid, dim3(256), 0, s, x, seg_start, tok_row, (int)N, (int)D, wg, bg, wb, bb, temp, sigmoid_bias, \
                                  mask_row, mask_out, thr_out, seg_next + 1)
    PV_DISPATCH_NCH(D, SPLG_LAUNCH);
#undef SPLG_LAUNCH
    rc = pv_check_launch();
    if (rc != PV_OK) return rc;
    if ((rc = pv_seg_scan(seg_next, (int)B, totals, s)) != PV_OK) return rc;
#define SPLC_LAUNCH(NC) do { if (ln_out) PV_LAUNCH((pv_spl_compact_kernel<NC, true>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D, mask_row, \
                                                   seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out);     \
                             else PV_LAUNCH((pv_spl_compact_kernel<NC, false>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D, mask_row,        \
                                            seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out); } while (0)
    PV_DISPATCH_NCH(D, SPLC_LAUNCH);
#undef SPLC_LAUNCH
    return pv_check_launch();
}

// The same step for training (include/peekvit_hip_sparse_long_train.h): the TRAIN instantiations of the two bodies above, which also leave the tables
// pv_residual_pack_step_long_bwd reads.
extern "C" int pv_residual_pack_step_long_train(const float* x, const int32_t* seg_start, const int32_t* mult, const int32_t* tok_row, int64_t B, int64_t N,
                                                int64_t D, const float* wg, const float* bg, const float* wb, const float* bb, float temp, float sigmoid_bias,
                                                float* mask_row, float* x_next, float* row_scale_next, int32_t* mult_next, float* log_mult_next,
                                                int32_t* seg_next, int32_t* tok_row_next, float* mask_out, float* thr_out, int32_t* totals,
                                                const float* ln_gamma, const float* ln_beta, float ln_eps, uint16_t* ln_out, float* gate_arg,
                                                int32_t* src_next, void* stream) {
    if (!gate_arg || !src_next) return PV_ERR_INVALID_ARG;
    int rc = pv_spl_check(x, seg_start, mult, tok_row, B, N, D, wg, bg, wb, bb, temp, mask_row, x_next, row_scale_next, mult_next, log_mult_next, seg_next,
                          tok_row_next, mask_out, thr_out, totals, ln_gamma, ln_beta, ln_out);
    if (rc != PV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)B);
#define SPLG_LAUNCH(NC) PV_LAUNCH((pv_spl_gate_train_kernel<NC>), grid, dim3(256), 0, s, x, seg_start, tok_row, (int)N, (int)D, wg, bg, wb, bb, temp, sigmoid_bias, \
                                  mask_row, mask_out, thr_out, seg_next + 1, gate_arg)
    PV_DISPATCH_NCH(D, SPLG_LAUNCH);
#undef SPLG_LAUNCH
    rc = pv_check_launch();
    if (rc != PV_OK) return rc;
    if ((rc = pv_seg_scan(seg_next, (int)B, totals, s)) != PV_OK) return rc;
#define SPLC_LAUNCH(NC) do { if (ln_out) PV_LAUNCH((pv_spl_compact_train_kernel<NC, true>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D,          \
                                                   mask_row, seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out, \
                                                   src_next);                                                                                                           \
                             else PV_LAUNCH((pv_spl_compact_train_kernel<NC, false>), grid, dim3(256), 0, s, x, seg_start, mult, tok_row, (int)N, (int)D, mask_row,       \
                                            seg_next, x_next, row_scale_next, mult_next, log_mult_next, tok_row_next, ln_gamma, ln_beta, ln_eps, ln_out, src_next); } while (0)
    PV_DISPATCH_NCH(D, SPLC_LAUNCH);
#undef SPLC_LAUNCH
    return pv_check_launch();
}
