// A-ViT's halting step on the packed live rows past PV_AVIT_PACK_MAX_S tokens per image (include/peekvit_hip_avit_long.h):
// pv_avit_pack_train.hip's three forward launches (state update, pv_seg_scan, compaction) and its backward for up to PV_AVIT_LONG_MAX_S tokens.  One
// workgroup of 256 threads per image, as there; where that file gives every token (and every row) one thread, these kernels walk the tokens and the
// segment in chunks of 256 and carry the h sum, the live count and the number of rows kept so far from chunk to chunk.  The resident kernels are not
// edited (their code stays as it is), so every expression that must round like theirs is restated here in their form: at S <= PV_AVIT_PACK_MAX_S each
// output has their bits (tests/test_hip_avit_long.py).  SAVE = false is the inference step: the same code without the stores to sv, ycls and src_next.
#include "pv_rows.h"
#include "../../include/peekvit_hip_avit_long.h"

#define PV_AVL_MAXS PV_AVIT_LONG_MAX_S
#define PV_AVL_CHUNK 256                        // tokens / rows per step of a walk (one thread each)

// (workgroup-uniform) the rows of image b, or 0 when the table does not describe rows inside [0, R)
__device__ __forceinline__ int pv_avl_segment(const int32_t* seg, int b, int S, int R, int& s0) {
    s0 = seg[b];
    const int L = seg[b + 1] - s0;
    return (s0 >= 0 && L >= 1 && L <= S + 1 && (int64_t)s0 + L <= R) ? L : 0;
}

template <bool SAVE>
__global__ __launch_bounds__(256) void pv_avit_long_update_kernel(
    const float* __restrict__ y, const int32_t* __restrict__ seg, const int32_t* __restrict__ nh, const int32_t* __restrict__ pos, int S, int D, int nc,
    int R, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in, float* c_out, float* R_out,
    float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out, float* __restrict__ h_part, float gate_scale,
    float gate_center, float thr, int last, int32_t* __restrict__ nh_next, int32_t* __restrict__ len_next, float* __restrict__ sv,
    float* __restrict__ ycls) {
    __shared__ int rowof[PV_AVL_MAXS];                // token -> row of the segment (-1: no row)
    __shared__ float red_h[2][4], cls_w[PV_AVIT_PACK_MAX_CLS], s_hrep;          // (the wave sums of a chunk, double-buffered over the chunks)
    __shared__ int red_n[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    int s0;
    const int L = pv_avl_segment(seg, b, S, R, s0);
    const int n_h = min(max(nh[b], 0), S);
    for (int t = tid; t < S; t += 256) rowof[t] = -1;
    if (tid < PV_AVIT_PACK_MAX_CLS) cls_w[tid] = 0.f;
    if (tid == 0) s_hrep = 0.f;
    __syncthreads();
    for (int i = tid; i < L; i += 256) {
        const int64_t row = s0 + i;
        const int p = pos[row];
        if (p >= 0 && p < S) {
            rowof[p] = i;
        } else {                                   // the representative row (p < 0), or a row no token of this image owns
            const float h = p < 0 ? pv_sigmoid(y[row * D] * gate_scale - gate_center) : 0.f;
            if (p < 0) s_hrep = h;
            if constexpr (SAVE) {
                sv[row] = h;
                sv[(int64_t)R + row] = 0.f;
                sv[2 * (int64_t)R + row] = p < 0 ? (float)PV_AVIT_PACK_REP : 0.f;
            }
        }
    }
    __syncthreads();
    float hsum = 0.f;                                  // (every thread carries both; thread 0 writes them)
    int n_live = 0;
    for (int c0 = 0, it = 0; c0 < S; c0 += PV_AVL_CHUNK, ++it) {
        const int tk = c0 + tid;
        float hv = 0.f;
        bool running = false;
        if (tk < S) {
            const int64_t t = (int64_t)b * S + tk;
            const int i = rowof[tk];
            const float c = c_in[t], Rr = R_in[t], rho = rho_in[t], cnt = counter_in[t];
            if (i >= 0) {
                const int64_t row = s0 + i;
                const float m = m_in[t];
                const float h = pv_sigmoid(y[row * D] * gate_scale - gate_center);
                const float hh = last ? 1.0f : h;
                const float c1 = c + hh;
                const float reached = c1 > thr ? m : 0.f, nr = c1 < thr ? 1.f : 0.f;
                const float w = m * (Rr * reached + hh * nr);
                hv = h;
                running = nr != 0.f;
                c_out[t] = c1;
                rho_out[t] = (rho + m) + Rr * reached;
                R_out[t] = Rr - nr * hh;
                counter_out[t] = cnt + nr;
                m_out[t] = nr;
                if (tk < nc) cls_w[tk] = w;
                if constexpr (SAVE) {
                    sv[row] = h;
                    sv[(int64_t)R + row] = w;
                    sv[2 * (int64_t)R + row] = (float)((reached != 0.f ? PV_AVIT_PACK_REACHED : 0) + (nr != 0.f ? PV_AVIT_PACK_NOT_REACHED : 0) +
                                                       (m != 0.f ? PV_AVIT_PACK_LIVE : 0) + (nr == 0.f && !last ? PV_AVIT_PACK_MERGED : 0));
                }
            } else {                                   // halted before this layer: the state stays, the token is not running
                c_out[t] = c;
                rho_out[t] = rho;
                R_out[t] = Rr;
                counter_out[t] = cnt;
                m_out[t] = 0.f;
            }
        }
        hv = pv_wave_sum(hv);
        const int n_run = __popcll(__ballot(running));
        float* const rh = red_h[it & 1];               // (the other buffer may still be read by a wave that is one chunk behind)
        int* const rn = red_n[it & 1];
        if (lane == 0) { rh[wave] = hv; rn[wave] = n_run; }
        __syncthreads();
        const float cs = (rh[0] + rh[1]) + (rh[2] + rh[3]);
        hsum = it == 0 ? cs : hsum + cs;               // the chunk sums in chunk order; one chunk is the resident step's sum
        n_live += rn[0] + rn[1] + rn[2] + rn[3];
    }
    if (tid == 0) {
        h_part[b] = hsum + s_hrep * (float)n_h;
        if (nh_next) nh_next[b] = S - n_live;
        if (len_next) len_next[b] = n_live + (S - n_live > 0 ? 1 : 0);
    }
    for (int e = tid; e < nc * nvec; e += 256) {          // class rows: acc' = acc + y * w, and the row itself for the backward
        const int p = e / nvec, v = e - p * nvec;
        const int i = rowof[p];
        const int64_t o = ((int64_t)b * nc + p) * nvec + v;
        const float4 a = reinterpret_cast<const float4*>(acc_in)[o];
        float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= 0) yv = reinterpret_cast<const float4*>(y)[(int64_t)(s0 + i) * nvec + v];
        const float w = cls_w[p];
        if constexpr (SAVE) reinterpret_cast<float4*>(ycls)[o] = yv;
        reinterpret_cast<float4*>(acc_out)[o] = i >= 0 ? make_float4(a.x + yv.x * w, a.y + yv.y * w, a.z + yv.z * w, a.w + yv.w * w) : a;
    }
}

template <bool SAVE>
__global__ __launch_bounds__(256) void pv_avit_long_compact_kernel(const float* __restrict__ y, const int32_t* __restrict__ seg,
                                                                   const int32_t* __restrict__ pos, int S, int D, int R, const float* __restrict__ mask,
                                                                   const int32_t* __restrict__ seg_next, const int32_t* __restrict__ nh_next,
                                                                   float* __restrict__ x_next, float* __restrict__ rs_next, float* __restrict__ lm_next,
                                                                   int32_t* __restrict__ pos_next, int32_t* __restrict__ src_next) {
    __shared__ int wcount[2][4];                       // kept rows of the chunk per wave, double-buffered over the chunks
    __shared__ uint16_t src[PV_AVL_MAXS];              // written row -> its row of the segment (at most S rows are kept; a row index is at most S)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    int s0;
    const int L = pv_avl_segment(seg, b, S, R, s0);
    const int d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    if (d0 < 0 || Ln < 1 || Ln > S || (int64_t)d0 + Ln > R) return;          // (workgroup-uniform, before any barrier)
    int carry = 0;                                     // rows kept in the chunks before
    for (int c0 = 0, it = 0; c0 < L; c0 += PV_AVL_CHUNK, ++it) {
        const int i = c0 + tid;
        int p = -1;
        bool keep = false;
        if (i < L) {
            p = pos[s0 + i];
            keep = p >= 0 && p < S && mask[(int64_t)b * S + p] != 0.0f;
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        int* const wc = wcount[it & 1];
        if (lane == 0) wc[wave] = __popcll(bal);
        __syncthreads();
        int base = carry;
        for (int w = 0; w < wave; ++w) base += wc[w];
        carry += wc[0] + wc[1] + wc[2] + wc[3];
        const int j = base + before;                   // stable: survivors keep their order
        if (keep && j < Ln) {
            src[j] = (uint16_t)i;
            pos_next[d0 + j] = p;
            rs_next[d0 + j] = 1.0f;
            lm_next[d0 + j] = 0.0f;
            if constexpr (SAVE) src_next[d0 + j] = i;
        }
    }
    const int nkeep = min(carry, Ln);
    const int n_h = nh_next[b];
    const bool rep = n_h > 0 && Ln == nkeep + 1;
    if (rep && tid == 0) {
        pos_next[d0 + nkeep] = -1;
        rs_next[d0 + nkeep] = 0.0f;
        lm_next[d0 + nkeep] = logf((float)n_h);
        if constexpr (SAVE) src_next[d0 + nkeep] = -1;
    }
    __syncthreads();
    for (int k = wave; k < nkeep; k += 4) {
        const float4* s = reinterpret_cast<const float4*>(y + (int64_t)(s0 + (int)src[k]) * D);
        float4* d = reinterpret_cast<float4*>(x_next + (int64_t)(d0 + k) * D);
        for (int v = lane; v < nvec; v += 64) d[v] = s[v];
    }
    if (rep && wave == 0) {
        float4* d = reinterpret_cast<float4*>(x_next + (int64_t)(d0 + nkeep) * D);
        for (int v = lane; v < nvec; v += 64) d[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

extern "C" int pv_avit_pack_step_long(const float* y, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos, int64_t B, int64_t S,
                                      int64_t D, int64_t R, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in,
                                      const float* m_in, float* c_out, float* R_out, float* rho_out, float* counter_out, float* m_out,
                                      const float* acc_in, float* acc_out, int64_t n_cls, float* h_part, float gate_scale, float gate_center,
                                      float threshold, int last, float* x_next, float* row_scale_next, int32_t* seg_next, int32_t* n_halted_next,
                                      float* log_mult_next, int32_t* pos_next, int32_t* totals, float* sv, float* ycls, int32_t* src_next, void* stream) {
    if (!y || !seg_start || !n_halted || !pos || !c_in || !R_in || !rho_in || !counter_in || !m_in || !c_out || !R_out || !rho_out || !counter_out ||
        !m_out || !acc_in || !acc_out || !h_part)
        return PV_ERR_INVALID_ARG;
    const bool save = sv || ycls;                     // the training step; all three null: the inference step
    if (save ? (!sv || !ycls) : src_next != nullptr) return PV_ERR_INVALID_ARG;
    if (!last && (!x_next || !row_scale_next || !seg_next || !n_halted_next || !log_mult_next || !pos_next || !totals || (save && !src_next)))
        return PV_ERR_INVALID_ARG;
    if (B <= 0 || S <= 0 || D <= 0 || R <= 0 || n_cls <= 0 || n_cls > S) return PV_ERR_INVALID_ARG;
    if (S > PV_AVIT_LONG_MAX_S || n_cls > PV_AVIT_PACK_MAX_CLS || D % 4 || D > PV_AVIT_PACK_MAX_D || B >= 0x7fffffff / S || R > 0x7fffffff)
        return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)y | (uintptr_t)x_next | (uintptr_t)acc_in | (uintptr_t)acc_out | (uintptr_t)ycls) & 15) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)seg_start | (uintptr_t)n_halted | (uintptr_t)pos | (uintptr_t)c_in | (uintptr_t)R_in | (uintptr_t)rho_in | (uintptr_t)counter_in |
         (uintptr_t)m_in | (uintptr_t)c_out | (uintptr_t)R_out | (uintptr_t)rho_out | (uintptr_t)counter_out | (uintptr_t)m_out | (uintptr_t)h_part |
         (uintptr_t)row_scale_next | (uintptr_t)seg_next | (uintptr_t)n_halted_next | (uintptr_t)log_mult_next | (uintptr_t)pos_next | (uintptr_t)totals |
         (uintptr_t)sv | (uintptr_t)src_next) & 3)
        return PV_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
#define AVL_UPDATE(SAVE) PV_LAUNCH((pv_avit_long_update_kernel<SAVE>), dim3((unsigned)B), dim3(256), 0, s, y, seg_start, n_halted, pos, (int)S, (int)D, \
                                   (int)n_cls, (int)R, c_in, R_in, rho_in, counter_in, m_in, c_out, R_out, rho_out, counter_out, m_out, acc_in, acc_out,   \
                                   h_part, gate_scale, gate_center, threshold, last, last ? nullptr : n_halted_next, last ? nullptr : seg_next + 1, sv, ycls)
    if (save) AVL_UPDATE(true);
    else AVL_UPDATE(false);
#undef AVL_UPDATE
    int rc = pv_check_launch();
    if (rc != PV_OK || last) return rc;
    if ((rc = pv_seg_scan(seg_next, (int)B, totals, s)) != PV_OK) return rc;
#define AVL_COMPACT(SAVE) PV_LAUNCH((pv_avit_long_compact_kernel<SAVE>), dim3((unsigned)B), dim3(256), 0, s, y, seg_start, pos, (int)S, (int)D, (int)R, \
                                    (const float*)m_out, (const int32_t*)seg_next, (const int32_t*)n_halted_next, x_next, row_scale_next, log_mult_next,  \
                                    pos_next, src_next)
    if (save) AVL_COMPACT(true);
    else AVL_COMPACT(false);
#undef AVL_COMPACT
    return pv_check_launch();
}

__global__ __launch_bounds__(256) void pv_avit_long_bwd_kernel(const float* __restrict__ g_next, const int32_t* __restrict__ seg, const int32_t* __restrict__ nh,
                                                               const int32_t* __restrict__ pos, const int32_t* __restrict__ seg_next,
                                                               const int32_t* __restrict__ src_next, const float* __restrict__ sv,
                                                               const float* __restrict__ ycls, const float* __restrict__ gR, const float* __restrict__ grho,
                                                               const float* __restrict__ gacc, const float* __restrict__ gh, float* G,
                                                               float* __restrict__ dy, uint16_t* __restrict__ dy16, float* __restrict__ dR, int S, int D, int nc,
                                                               int R, int Rn, float score_coef, float gate_scale, int last) {
    __shared__ int inv[PV_AVL_MAXS + 1], rowof[PV_AVL_MAXS];          // input row -> the row written from it; token -> input row
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    int s0;
    const int L = pv_avl_segment(seg, b, S, R, s0);
    const int n_h = min(max(nh[b], 0), S);
    const float G_old = G[b];
    const float gs = (gh != nullptr && b >= 1) ? gh[0] * score_coef : 0.f;          // d(score) / d(h) of a token of the images 1..
    for (int i = tid; i < S + 1; i += 256) inv[i] = -1;
    for (int t = tid; t < S; t += 256) rowof[t] = -1;
    __syncthreads();
    int d0 = 0;
    if (!last) {
        d0 = seg_next[b];
        int Ln = seg_next[b + 1] - d0;
        if (d0 < 0 || Ln < 1 || Ln > S || (int64_t)d0 + Ln > Rn) Ln = 0;
        for (int j = tid; j < Ln; j += 256) {
            const int i = src_next[d0 + j];
            if (i >= 0 && i < L) inv[i] = j;
        }
    }
    for (int i = tid; i < L; i += 256) {
        const int p = pos[s0 + i];
        if (p >= 0 && p < S) rowof[p] = i;
    }
    __syncthreads();
    int rep_i = -1;                                   // (workgroup-uniform) the representative row is the segment's last
    float G_new = G_old;
    if (L > 0 && pos[s0 + L - 1] < 0) {
        rep_i = L - 1;
        const float h = sv[s0 + L - 1];
        G_new = G_old + gs * h * (1.0f - h) * gate_scale;
    }
    for (int i = wave; i < L; i += 4) {               // (wave-uniform)
        const int64_t row = s0 + i;
        const int p = pos[row];
        float4* dr = reinterpret_cast<float4*>(dy + row * D);
        u32x2* d16 = reinterpret_cast<u32x2*>(dy16 != nullptr ? dy16 + row * D : nullptr);
        if (p < 0 || p >= S) {                        // representative row: the total of its n members, channel 0 only
            const float v0 = i == rep_i ? (float)n_h * G_new : 0.f;
            for (int v = lane; v < nvec; v += 64) {
                const float4 o = make_float4(v == 0 ? v0 : 0.f, 0.f, 0.f, 0.f);
                dr[v] = o;
                if (dy16 != nullptr) d16[v] = (u32x2){pv_pack_bf16x2(o.x, o.y), pv_pack_bf16x2(o.z, o.w)};
            }
            continue;
        }
        const int64_t t = (int64_t)b * S + p;
        const float h = sv[row], w = sv[(int64_t)R + row];
        const int fl = (int)sv[2 * (int64_t)R + row];
        const float reached = (fl & PV_AVIT_PACK_REACHED) ? 1.f : 0.f, nr = (fl & PV_AVIT_PACK_NOT_REACHED) ? 1.f : 0.f;
        const int jn = last ? -1 : inv[i];
        const float4* src4 = jn >= 0 ? reinterpret_cast<const float4*>(g_next + (int64_t)(d0 + jn) * D) : nullptr;
        const float pass = (!last && jn < 0) ? G_old : 0.f;          // merged: every later layer's score term passes through
        const bool cls = p < nc;
        const float4* ga = reinterpret_cast<const float4*>(gacc + ((int64_t)b * nc + (cls ? p : 0)) * D);
        const float g_r = gR[t];
        float dot = 0.f;
        if (cls) {
            const float4* yc = reinterpret_cast<const float4*>(ycls + ((int64_t)b * nc + p) * D);
            for (int v = lane; v < nvec; v += 64) {
                const float4 g = ga[v], q = yc[v];
                dot += (g.x * q.x + g.y * q.y) + (g.z * q.z + g.w * q.w);
            }
            dot = pv_wave_sum(dot);
        }
        float dh = gs;
        if (!last) dh += nr * (dot - g_r);
        const float e0 = dh * h * (1.0f - h) * gate_scale + pass;
        for (int v = lane; v < nvec; v += 64) {
            float4 o = src4 != nullptr ? src4[v] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (cls) {
                const float4 g = ga[v];
                o.x += g.x * w; o.y += g.y * w; o.z += g.z * w; o.w += g.w * w;
            }
            if (v == 0) o.x += e0;
            dr[v] = o;
            // (the plain pack, as pv_avit_pack_step_bwd: a value beyond fp16's range becomes inf in the copy, which the training pass checks)
            if (dy16 != nullptr) d16[v] = (u32x2){pv_pack_bf16x2(o.x, o.y), pv_pack_bf16x2(o.z, o.w)};
        }
        if (lane == 0) dR[t] = g_r + grho[t] * reached + reached * dot;
    }
    for (int t = tid; t < S; t += 256)                // R' = R for a token without a row
        if (rowof[t] < 0) dR[(int64_t)b * S + t] = gR[(int64_t)b * S + t];
    if (tid == 0) G[b] = G_new;                       // (G_old was read before the barriers above)
}

extern "C" int pv_avit_pack_step_long_bwd(const float* g_next, const int32_t* seg_start, const int32_t* n_halted, const int32_t* pos,
                                          const int32_t* seg_next, const int32_t* src_next, const float* sv, const float* ycls, const float* gR,
                                          const float* grho, const float* gacc, const float* gh, float* G, float* dy, uint16_t* dy16, float* dR, int64_t B,
                                          int64_t S, int64_t D, int64_t R, int64_t R_next, int64_t n_cls, float gate_scale, int last, void* stream) {
    if (!seg_start || !n_halted || !pos || !sv || !ycls || !gR || !grho || !gacc || !G || !dy || !dR) return PV_ERR_INVALID_ARG;
    if (!last && (!g_next || !seg_next || !src_next || R_next <= 0)) return PV_ERR_INVALID_ARG;
    if (B <= 0 || S <= 0 || D <= 0 || R <= 0 || n_cls <= 0 || n_cls > S || dR == gR) return PV_ERR_INVALID_ARG;
    if (S > PV_AVIT_LONG_MAX_S || n_cls > PV_AVIT_PACK_MAX_CLS || D % 4 || D > PV_AVIT_PACK_MAX_D || B >= 0x7fffffff / S || R > 0x7fffffff ||
        R_next > 0x7fffffff)
        return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)dy | (uintptr_t)g_next | (uintptr_t)gacc | (uintptr_t)ycls) & 15) return PV_ERR_INVALID_ARG;
    if ((uintptr_t)dy16 & 7) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)seg_start | (uintptr_t)n_halted | (uintptr_t)pos | (uintptr_t)seg_next | (uintptr_t)src_next | (uintptr_t)sv | (uintptr_t)gR |
         (uintptr_t)grho | (uintptr_t)gh | (uintptr_t)G | (uintptr_t)dR) & 3)
        return PV_ERR_INVALID_ARG;
    const float score_coef = B > 1 ? 1.0f / ((float)(B - 1) * (float)S) : 0.f;          // mean(h[1:]): no image behind the first at B = 1
    PV_LAUNCH(pv_avit_long_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, g_next, seg_start, n_halted, pos, seg_next, src_next, sv, ycls,
              gR, grho, gacc, gh, G, dy, dy16, dR, (int)S, (int)D, (int)n_cls, (int)R, (int)(last ? 0 : R_next), score_coef, gate_scale, last);
    return pv_check_launch();
}
