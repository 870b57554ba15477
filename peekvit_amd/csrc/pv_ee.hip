// Early exit (reference models/eeresidualvit.py, include/peekvit_hip_ee.h): the fused per-layer exit head, the exit decision with its
// compaction plan, and the gather of whole images into the shrunken batch.
//
// pv_exit_head_f32 does the work of two kernels of pv_rowops.hip in one launch and rounds like them to the bit, because it is built from the
// same functions of pv_rows.h:
//   LayerNorm  pv_cls_pool (num_cls = 1): mean and rstd by pv_ln_rows_stats, every element (v - mean) * rstd * gamma + beta with each
//              operation rounded on its own (pv_ee_norm below), then pooled = 0 + y (the class-token sum over one token);
//   linear     pv_head_f32: pv_head_tile / pv_head_dot - a fused multiply-add chain per 32-column K step (k ascending), the step sums added
//              in order, then + bias.
// The tiled kernel keeps the two row statistics of its 32 images in LDS and normalises an element as it is staged; the small-batch kernel
// (one wave per 64 logits of one image) normalises the row in registers and reads it back from LDS.
//
// pv_exit_step = two launches: `conf` (one wave per live row: max softmax, decision, scatter of the exiting rows) and `plan` (one workgroup:
// exclusive scan of the survivor flags in row order -> next_live, src_row, count).  Nothing depends on the order of concurrent work.
#include "pv_rows.h"
#include "../../include/peekvit_hip_ee.h"

// pooled element of pv_cls_pool with one class token: 0 + ((v - mean) * rstd * gamma + beta), no operation fused
__device__ __forceinline__ float pv_ee_norm(float v, float mean, float rstd, float g, float be) {
#pragma clang fp contract(off)          // (the __f*_rn intrinsics are plain operators to hipcc: it fused the last multiply and add without this)
    const float y = (v - mean) * rstd * g + be;
    return 0.f + y;
}

// ------------------------------------------------------------------------------------------------
// tiled exit head: 32 images x 64 classes per workgroup (pv_head_tile, as pv_head_kernel)
// ------------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void pv_exit_head_kernel(const float* __restrict__ x, int64_t img_stride, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int B, int D, int C) {
    constexpr int TM = PV_HEAD_TM;
    __shared__ float s_mean[TM], s_rstd[TM];
    const int m0 = blockIdx.y * TM;
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = D >> 2;
        for (int rr = wave; rr < TM; rr += 4) {
            if (m0 + rr >= B) break;                    // (wave-uniform)
            RowRegs<NCH> r[1];
            pv_load_row<NCH>(r[0], x + (int64_t)(m0 + rr) * img_stride, nvec, lane);
            float mean[1], rstd[1];
            pv_ln_rows_stats<NCH, 1>(r, D, nvec, lane, eps, mean, rstd);
            if (lane == 0) { s_mean[rr] = mean[0]; s_rstd[rr] = rstd[0]; }
        }
    }
    __syncthreads();
    // (the row's two statistics are read once, here: a fetch that took (row, column) from the tile would read them from LDS in every K step, and
    // that form cost two VGPRs and a wave of occupancy, 7 -> 6)
    const int m = m0 + pv_head_a_row(threadIdx.x);
    const bool a_ok = m < B;
    const float mean = a_ok ? s_mean[m - m0] : 0.f, rstd = a_ok ? s_rstd[m - m0] : 0.f;
    const int ak = pv_head_a_col(threadIdx.x);
    const float* ap = x + (int64_t)(a_ok ? m : 0) * img_stride + ak;
    pv_head_tile([&](int k0) {          // normalise on load
        const float4 raw = *reinterpret_cast<const float4*>(ap + k0);
        const float4 g = *reinterpret_cast<const float4*>(gamma + k0 + ak), be = *reinterpret_cast<const float4*>(beta + k0 + ak);
        return make_float4(pv_ee_norm(raw.x, mean, rstd, g.x, be.x), pv_ee_norm(raw.y, mean, rstd, g.y, be.y),
                           pv_ee_norm(raw.z, mean, rstd, g.z, be.z), pv_ee_norm(raw.w, mean, rstd, g.w, be.w));
    }, w, bias, out, B, D, C);
}

// small batches: one wave per (64 classes, image); the normalised row goes through LDS, then one thread per logit (pv_head_dot, as
// pv_head_small_kernel)
template <int NCH>
__global__ __launch_bounds__(64) void pv_exit_head_small_kernel(const float* __restrict__ x, int64_t img_stride, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ out, int B, int D, int C) {
    __shared__ float4 s_row[PV_EE_MAX_D / 4];
    const int lane = threadIdx.x, b = blockIdx.y, nvec = D >> 2;
    {
        RowRegs<NCH> r;
        pv_load_row<NCH>(r, x + (int64_t)b * img_stride, nvec, lane);
        pv_ln_row<NCH>(r, gamma, beta, D, nvec, lane, eps);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = lane + 64 * j;
            if (idx < nvec) s_row[idx] = make_float4(__fadd_rn(0.f, r.v[j].x), __fadd_rn(0.f, r.v[j].y), __fadd_rn(0.f, r.v[j].z), __fadd_rn(0.f, r.v[j].w));
        }
    }
    __syncthreads();
    const int c = blockIdx.x * 64 + lane;
    if (c >= C) return;
    const float acc = pv_head_dot(s_row, reinterpret_cast<const float4*>(w + (int64_t)c * D), nvec);
    out[(int64_t)b * C + c] = acc + (bias ? bias[c] : 0.f);
}

extern "C" int pv_exit_head_f32(const float* x, int64_t img_stride, const float* ln_gamma, const float* ln_beta, float ln_eps, const float* w,
                                const float* bias, float* logits, int64_t B, int64_t D, int64_t C, void* stream) {
    if (!x || !ln_gamma || !ln_beta || !w || !logits || B <= 0 || D <= 0 || C <= 0) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > PV_EE_MAX_D || B > 0x7fffffff || C > 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (img_stride % 4 || img_stride < D) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x | (uintptr_t)ln_gamma | (uintptr_t)ln_beta | (uintptr_t)w) & 15) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)logits & 3) || (bias && ((uintptr_t)bias & 3))) return PV_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (B <= 16) {
        if ((C + 63) / 64 > 0x7fffffff) return PV_ERR_UNSUPPORTED;
#define EH_SMALL(N) PV_LAUNCH(pv_exit_head_small_kernel<N>, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(64), 0, s, x, img_stride, ln_gamma, ln_beta, \
                              ln_eps, w, bias, logits, (int)B, (int)D, (int)C)
        PV_DISPATCH_NCH(D, EH_SMALL);
#undef EH_SMALL
        return pv_check_launch();
    }
    if ((B + 31) / 32 > 65535) return PV_ERR_UNSUPPORTED;
    dim3 grid((unsigned)((C + 63) / 64), (unsigned)((B + 31) / 32));
#define EH_TILED(N) PV_LAUNCH(pv_exit_head_kernel<N>, grid, dim3(256), 0, s, x, img_stride, ln_gamma, ln_beta, ln_eps, w, bias, logits, (int)B, (int)D, (int)C)
    PV_DISPATCH_NCH(D, EH_TILED);
#undef EH_TILED
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// exit decision + compaction plan
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_exit_conf_kernel(const float* __restrict__ logits, int64_t ldl, const int32_t* __restrict__ live, int n_live,
                                                           int C, float threshold, int64_t layer, float* __restrict__ row_conf,
                                                           float* __restrict__ out_logits, int64_t ldo, int64_t* __restrict__ out_layer,
                                                           float* __restrict__ out_conf, int n_total, int32_t* __restrict__ count_all_exit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool all_exit = count_all_exit != nullptr;       // threshold -inf: every row exits, a NaN row too; nobody is left to plan for
    if (all_exit && blockIdx.x == 0 && threadIdx.x == 0) *count_all_exit = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_live; r += (int64_t)gridDim.x * 4) {
        const float* lr = logits + r * ldl;
        float m = -__builtin_inff();
        for (int c = lane; c < C; c += 64) m = fmaxf(m, lr[c]);
        m = pv_wave_max(m);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = __fadd_rn(s, expf(__fsub_rn(lr[c], m)));
        s = pv_wave_sum(s);
        const float conf = __fdiv_rn(1.0f, s);          // the maximum's own term is exp(0) = 1
        if (lane == 0) row_conf[r] = conf;
        const int idx = live[r];
        if ((all_exit || conf >= threshold) && idx >= 0 && idx < n_total) {
            float* o = out_logits + (int64_t)idx * ldo;
            for (int c = lane; c < C; c += 64) o[c] = lr[c];
            if (lane == 0) { out_layer[idx] = layer; out_conf[idx] = conf; }
        }
    }
}

// one workgroup of 1024 threads: survivors in row order
__global__ __launch_bounds__(1024) void pv_exit_plan_kernel(const float* __restrict__ row_conf, const int32_t* __restrict__ live, int n_live, float threshold,
                                                            int n_total, int32_t* __restrict__ next_live, int32_t* __restrict__ src_row,
                                                            int32_t* __restrict__ count) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;
    for (int base = 0; base < n_live; base += 1024) {
        const int i = base + t;
        const int idx = i < n_live ? live[i] : -1;
        const int v = (i < n_live && idx >= 0 && idx < n_total && !(row_conf[i] >= threshold)) ? 1 : 0;
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
            const int sk = wsum[k];
            before += k < w ? sk : 0;
            total += sk;
        }
        if (v) {
            const int pos = carry + before + incl - 1;      // < n_live: at most one position per row
            next_live[pos] = idx;
            src_row[pos] = i;
        }
        carry += total;
        __syncthreads();                                    // (wsum is rewritten by the next chunk)
    }
    if (t == 0) *count = carry;
}

extern "C" int pv_exit_step(const float* logits, int64_t ldl, const int32_t* live, int64_t n_live, int64_t C, float threshold, int64_t layer,
                            float* row_conf, float* out_logits, int64_t ldo, int64_t* out_layer, float* out_conf, int64_t n_total,
                            int32_t* next_live, int32_t* src_row, int32_t* count, void* stream) {
    if (!logits || !live || !row_conf || !out_logits || !out_layer || !out_conf || !next_live || !src_row || !count) return PV_ERR_INVALID_ARG;
    if (n_live <= 0 || C <= 0 || n_total <= 0 || ldl < C || ldo < C || threshold != threshold) return PV_ERR_INVALID_ARG;
    if (n_live >= 0x7fffffff || n_total >= 0x7fffffff || C >= 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)logits | (uintptr_t)live | (uintptr_t)row_conf | (uintptr_t)out_logits | (uintptr_t)out_conf | (uintptr_t)next_live |
         (uintptr_t)src_row | (uintptr_t)count) & 3) return PV_ERR_INVALID_ARG;
    if ((uintptr_t)out_layer & 7) return PV_ERR_INVALID_ARG;
    {   // the scattered rows must not land on the rows being read
        const uintptr_t a0 = (uintptr_t)logits, a1 = a0 + (uintptr_t)((n_live - 1) * ldl + C) * 4;
        const uintptr_t b0 = (uintptr_t)out_logits, b1 = b0 + (uintptr_t)((n_total - 1) * ldo + C) * 4;
        if (a0 < b1 && b0 < a1) return PV_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool all_exit = threshold == -__builtin_inff();
    PV_LAUNCH(pv_exit_conf_kernel, dim3(pv_stream_grid(n_live, 4)), dim3(256), 0, s, logits, ldl, live, (int)n_live, (int)C, threshold, layer, row_conf,
              out_logits, ldo, out_layer, out_conf, (int)n_total, all_exit ? count : (int32_t*)nullptr);
    int rc = pv_check_launch();
    if (rc || all_exit) return rc;
    PV_LAUNCH(pv_exit_plan_kernel, dim3(1), dim3(1024), 0, s, (const float*)row_conf, live, (int)n_live, threshold, (int)n_total, next_live, src_row, count);
    return pv_check_launch();
}

// ------------------------------------------------------------------------------------------------
// compaction of whole images
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_gather_images_kernel(const float* __restrict__ x, int n_in, const int32_t* __restrict__ src_row, int n_out,
                                                               int64_t nvec, float* __restrict__ out) {
    for (int j = blockIdx.y; j < n_out; j += gridDim.y) {
        const int sr = src_row[j];
        if (sr < 0 || sr >= n_in) continue;
        const float4* src = reinterpret_cast<const float4*>(x) + (int64_t)sr * nvec;
        float4* dst = reinterpret_cast<float4*>(out) + (int64_t)j * nvec;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
    }
}

extern "C" int pv_gather_images_f32(const float* x, int64_t n_in, const int32_t* src_row, int64_t n_out, int64_t image_elems, float* out, void* stream) {
    if (!x || !src_row || !out || n_in <= 0 || n_out <= 0 || image_elems <= 0) return PV_ERR_INVALID_ARG;
    if (n_in >= 0x7fffffff || n_out >= 0x7fffffff) return PV_ERR_UNSUPPORTED;
    if (image_elems % 4) return PV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)src_row & 3)) return PV_ERR_INVALID_ARG;
    {
        const uintptr_t a0 = (uintptr_t)x, a1 = a0 + (uintptr_t)(n_in * image_elems) * 4;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uintptr_t)(n_out * image_elems) * 4;
        if (a0 < b1 && b0 < a1) return PV_ERR_INVALID_ARG;
    }
    const int64_t nvec = image_elems / 4;
    int64_t gx = (nvec + 1023) / 1024;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    const int64_t gy = n_out < 16384 ? n_out : 16384;
    PV_LAUNCH(pv_gather_images_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, x, (int)n_in, src_row, (int)n_out, nvec, out);
    return pv_check_launch();
}
