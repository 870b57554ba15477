// A-ViT's halting step in training (reference models/adavit.py:170-217, include/peekvit_hip_avit_train.h): forward and backward, one launch each.
//
// Forward: one workgroup of 16 waves per image, wave w owns the token rows w, w + 16, ...  A row's arithmetic is wave-uniform (one channel of y and
// five state values); the wave's 64 lanes do the row-wide work: the class rows' accumulation and copy, the zero fill of a halted row.  The image's
// sum of h is added row by row inside each wave, then over the 16 waves in order - a fixed order, no atomics.
// Backward: one wave per token row, grid-strided; only channel 0 of a row and the class rows are touched.
#include "pv_rows.h"
#include "../../include/peekvit_hip_avit_train.h"

#define PV_AVIT_WAVES 16

__global__ __launch_bounds__(PV_AVIT_WAVES * 64) void pv_avit_act_fwd_kernel(
    float* __restrict__ y, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in, float* c_out,
    float* R_out, float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out, float* __restrict__ h_part,
    float* __restrict__ sv, float* __restrict__ ycls, int S, int D, int n_cls, int64_t rows, float gate_scale, float gate_center, float thr, int last) {
    __shared__ float s_h[PV_AVIT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const int64_t b = blockIdx.x;
    float hsum = 0.f;
    for (int s = wave; s < S; s += PV_AVIT_WAVES) {          // (wave-uniform)
        const int64_t row = b * S + s;
        float4* yr = reinterpret_cast<float4*>(y + row * D);
        float h = 0.f;
        if (lane == 0) h = pv_sigmoid(y[row * D] * gate_scale - gate_center);          // one lane's expf, not sixty-four (pv_rows.h)
        h = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, h)));
        const float hh = last ? 1.0f : h;
        const float c = c_in[row], R = R_in[row], rho = rho_in[row], cnt = counter_in[row], m = m_in[row];
        const float c1 = c + hh;
        const float reached = c1 > thr ? m : 0.f, nr = c1 < thr ? 1.f : 0.f;
        const float w = m * (R * reached + hh * nr);
        hsum += h;
        if (s < n_cls) {                                      // class rows: acc' = acc + y * w, and the row itself for the backward
            const int64_t crow = b * n_cls + s;
            const float4* ai = reinterpret_cast<const float4*>(acc_in + crow * D);
            float4* ao = reinterpret_cast<float4*>(acc_out + crow * D);
            float4* yc = reinterpret_cast<float4*>(ycls + crow * D);
            for (int i = lane; i < nvec; i += 64) {
                const float4 v = yr[i], a = ai[i];
                yc[i] = v;
                ao[i] = make_float4(a.x + v.x * w, a.y + v.y * w, a.z + v.z * w, a.w + v.w * w);
            }
        }
        if (nr == 0.f) {                                      // halted from here on: the next block reads a zero row
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = lane; i < nvec; i += 64) yr[i] = z;
        }
        if (lane == 0) {
            c_out[row] = c1;
            rho_out[row] = (rho + m) + R * reached;
            R_out[row] = R - nr * hh;
            counter_out[row] = cnt + nr;
            m_out[row] = nr;
            sv[row] = h;
            sv[rows + row] = w;
            sv[2 * rows + row] = (float)((reached != 0.f ? PV_AVIT_REACHED : 0) + (nr != 0.f ? PV_AVIT_NOT_REACHED : 0) + (m != 0.f ? PV_AVIT_LIVE : 0));
        }
    }
    if (lane == 0) s_h[wave] = hsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < PV_AVIT_WAVES; ++k) t += s_h[k];
        h_part[b] = t;
    }
}

extern "C" int pv_avit_act_fwd(float* y, const float* c_in, const float* R_in, const float* rho_in, const float* counter_in, const float* m_in,
                               float* c_out, float* R_out, float* rho_out, float* counter_out, float* m_out, const float* acc_in, float* acc_out,
                               float* h_part, float* sv, float* ycls, int64_t B, int64_t S, int64_t D, int64_t n_cls, float gate_scale,
                               float gate_center, float threshold, int last, void* stream) {
    if (!y || !c_in || !R_in || !rho_in || !counter_in || !m_in || !c_out || !R_out || !rho_out || !counter_out || !m_out || !acc_in || !acc_out ||
        !h_part || !sv || !ycls)
        return PV_ERR_INVALID_ARG;
    if (B <= 0 || S <= 0 || D <= 0 || n_cls <= 0 || n_cls > S) return PV_ERR_INVALID_ARG;
    if (S > PV_AVIT_MAX_S || D % 4 || D > PV_AVIT_MAX_D || B >= 0x7fffffff / S) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)y | (uintptr_t)acc_in | (uintptr_t)acc_out | (uintptr_t)ycls) & 15) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)c_in | (uintptr_t)R_in | (uintptr_t)rho_in | (uintptr_t)counter_in | (uintptr_t)m_in | (uintptr_t)c_out | (uintptr_t)R_out |
         (uintptr_t)rho_out | (uintptr_t)counter_out | (uintptr_t)m_out | (uintptr_t)h_part | (uintptr_t)sv) & 3)
        return PV_ERR_INVALID_ARG;
    PV_LAUNCH(pv_avit_act_fwd_kernel, dim3((unsigned)B), dim3(PV_AVIT_WAVES * 64), 0, (hipStream_t)stream, y, c_in, R_in, rho_in, counter_in, m_in, c_out,
              R_out, rho_out, counter_out, m_out, acc_in, acc_out, h_part, sv, ycls, (int)S, (int)D, (int)n_cls, B * S, gate_scale, gate_center, threshold,
              last);
    return pv_check_launch();
}

__global__ __launch_bounds__(256) void pv_avit_act_bwd_kernel(float* __restrict__ dy, uint16_t* __restrict__ dy16, const float* gR, const float* __restrict__ grho,
                                                              const float* __restrict__ gacc, const float* __restrict__ gh, const float* __restrict__ sv,
                                                              const float* __restrict__ ycls, float* dR, int S, int D, int n_cls, int64_t rows,
                                                              float score_coef, float gate_scale, int last) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
    const float gscore = gh != nullptr ? gh[0] * score_coef : 0.f;          // d(score) / d(h) of a token of the images 1..
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t b = row / S;
        const int s = (int)(row - b * S);
        const float h = sv[row], w = sv[rows + row];
        const int fl = (int)sv[2 * rows + row];
        const float reached = (fl & PV_AVIT_REACHED) ? 1.f : 0.f, nr = (fl & PV_AVIT_NOT_REACHED) ? 1.f : 0.f, m = (fl & PV_AVIT_LIVE) ? 1.f : 0.f;
        const float g_r = gR[row];
        float dot = 0.f;
        float4* dr = reinterpret_cast<float4*>(dy + row * D);
        if (s < n_cls) {                                      // (wave-uniform)
            const int64_t crow = b * n_cls + s;
            const float4* ga = reinterpret_cast<const float4*>(gacc + crow * D);
            const float4* yc = reinterpret_cast<const float4*>(ycls + crow * D);
            for (int i = lane; i < nvec; i += 64) {
                const float4 g = ga[i], v = yc[i];
                dot += (g.x * v.x + g.y * v.y) + (g.z * v.z + g.w * v.w);
            }
            dot = pv_wave_sum(dot);
        }
        float dh = b >= 1 ? gscore : 0.f;
        if (!last) dh += nr * (m * dot - g_r);
        const float d0 = dh * h * (1.0f - h) * gate_scale;     // through the sigmoid gate into channel 0
        if (s < n_cls) {
            const float4* ga = reinterpret_cast<const float4*>(gacc + (b * n_cls + s) * D);
            u32x2* d16 = reinterpret_cast<u32x2*>(dy16 != nullptr ? dy16 + row * D : nullptr);
            for (int i = lane; i < nvec; i += 64) {
                const float4 g = ga[i];
                float4 v = dr[i];
                v.x += g.x * w; v.y += g.y * w; v.z += g.z * w; v.w += g.w * w;
                if (i == 0) v.x += d0;
                dr[i] = v;
                // (the plain pack: this entry point has no range-flag word.  A value beyond fp16's range becomes inf in the copy and shows in the
                // LayerNorm-backward column sums of the block in front, which the training pass checks - train_engine.TrainPass.note)
                if (dy16 != nullptr) d16[i] = (u32x2){pv_pack_bf16x2(v.x, v.y), pv_pack_bf16x2(v.z, v.w)};
            }
        } else if (lane == 0) {
            const float v = dy[row * D] + d0;
            dy[row * D] = v;
            if (dy16 != nullptr) dy16[row * D] = pv_f2bf(v);
        }
        if (lane == 0) dR[row] = g_r + grho[row] * reached + reached * dot;
    }
}

extern "C" int pv_avit_act_bwd(float* dy, uint16_t* dy16, const float* gR, const float* grho, const float* gacc, const float* gh, const float* sv,
                               const float* ycls, float* dR, int64_t B, int64_t S, int64_t D, int64_t n_cls, float gate_scale, int last, void* stream) {
    if (!dy || !gR || !grho || !gacc || !sv || !ycls || !dR) return PV_ERR_INVALID_ARG;
    if (B <= 0 || S <= 0 || D <= 0 || n_cls <= 0 || n_cls > S) return PV_ERR_INVALID_ARG;
    if (S > PV_AVIT_MAX_S || D % 4 || D > PV_AVIT_MAX_D || B >= 0x7fffffff / S) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)dy | (uintptr_t)gacc | (uintptr_t)ycls) & 15) return PV_ERR_INVALID_ARG;
    if ((uintptr_t)dy16 & 7) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)gR | (uintptr_t)grho | (uintptr_t)gh | (uintptr_t)sv | (uintptr_t)dR) & 3) return PV_ERR_INVALID_ARG;
    const int64_t rows = B * S;
    const float score_coef = B > 1 ? 1.0f / ((float)(B - 1) * (float)S) : 0.f;          // mean(h[1:]): no image behind the first at B = 1
    PV_LAUNCH(pv_avit_act_bwd_kernel, dim3(pv_stream_grid(rows, 4)), dim3(256), 0, (hipStream_t)stream, dy, dy16, gR, grho, gacc, gh, sv, ycls, dR, (int)S,
              (int)D, (int)n_cls, rows, score_coef, gate_scale, last);
    return pv_check_launch();
}
