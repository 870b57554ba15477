// ResidualViT training on the packed live rows past PV_SPARSE_MAX_LEN rows per image (include/peekvit_hip_sparse_long_train.h): the
// backward of the pack step for segments of up to PV_SPARSE_LONG_MAX_LEN rows.  (The other three entry points of that header are further
// instantiations of existing bodies and sit with them: the streaming forward with statistics in pv_attention.hip, the ragged backward's dQ kernel in
// pv_sparse_train.hip, the TRAIN form of the chunked pack step in pv_sparse_long.hip.)
#include "pv_rows.h"
#include "../../include/peekvit_hip_sparse_long_train.h"

// pv_sp_pack_bwd_kernel (pv_sparse_train.hip) for N + 2 <= PV_SPARSE_LONG_MAX_LEN.
// One workgroup per image still; the tables that were one thread per row are walked in strides of 256 and held as 16-bit indices (pv_sparse_long.hip's
// choice).  The sum of dmask over a row's tokens must stay one owner's, in token order, but not N steps in every thread: the tokens are counted per
// row first (integer LDS adds, order-free, two 16-bit counts per word); a row of one token then gets that token's value from the thread that holds
// the token, and a live row of several tokens - one merged class can come live again per layer - is walked by one wave, 64 tokens per step, which
// adds the matching values in token order.  (0.f + v: that kernel starts from +0 and adds +0 for every token of another row, so only the sign
// of a zero could differ.)  The row loop, its wave-to-row assignment and the order of every sum are that kernel's: at N + 2 <= PV_SPARSE_MAX_LEN the
// outputs have its bits.  The four waves' dwg partials are combined one wave at a time, in that kernel's order ((acc + t0) + t1) + t2, through one
// buffer that shares its LDS with the counts and the token table, which are dead by then.
#define PV_SPLT_MAXL PV_SPARSE_LONG_MAX_LEN
#define PV_SPLT_NONE 0xffffu            // inverse table: the row merged into the zero row (no row index reaches it)

template <int NCH>
__global__ __launch_bounds__(256) void pv_spl_pack_bwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, const int32_t* __restrict__ tok_row,
                                                              int N, int D, const float* __restrict__ mask_row, const float* __restrict__ gate_arg,
                                                              const float* __restrict__ thr_in, const int32_t* __restrict__ seg_next,
                                                              const int32_t* __restrict__ src_next, const float* __restrict__ G, const float* __restrict__ drs,
                                                              const float* __restrict__ dmask, const float* __restrict__ wg, const float* __restrict__ wb,
                                                              float temp, float* __restrict__ dx, float* __restrict__ dm_row, float* __restrict__ dwg_part,
                                                              float* __restrict__ dwb_part, float* __restrict__ scal_part) {
    static_assert(NCH * 64 * sizeof(float4) <= PV_SPLT_MAXL * 4, "the dwg buffer shares the LDS of the counts and the token table");
    __shared__ __attribute__((aligned(16))) char shared_tab[PV_SPLT_MAXL * 4];       // counts (2 per word) | token -> row; later one wave's dwg partial
    __shared__ uint16_t inv[PV_SPLT_MAXL];
    __shared__ float dms[PV_SPLT_MAXL];
    __shared__ float red_s[4][2];
    unsigned* const cnt = reinterpret_cast<unsigned*>(shared_tab);                    // [PV_SPLT_MAXL / 2]
    uint16_t* const stok = reinterpret_cast<uint16_t*>(shared_tab + PV_SPLT_MAXL * 2); // [PV_SPLT_MAXL]
    float4* const red_w = reinterpret_cast<float4*>(shared_tab);                      // [NCH * 64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nvec = D >> 2;
    const int b = blockIdx.x;
    const int s0 = seg[b], L = seg[b + 1] - s0, d0 = seg_next[b], Ln = seg_next[b + 1] - d0;
    if (L < 2 || L > N + 2 || N + 2 > PV_SPLT_MAXL || Ln < 2 || Ln > L) {          // (workgroup-uniform: tables this library did not write - the image adds nothing)
        for (int idx = tid; idx < nvec; idx += 256) {
            reinterpret_cast<float4*>(dwg_part + (int64_t)b * D)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(dwb_part + (int64_t)b * D)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 4) scal_part[b * 4 + tid] = 0.f;
        return;
    }
    for (int i = tid; i < L; i += 256) { inv[i] = (uint16_t)PV_SPLT_NONE; dms[i] = 0.f; }
    for (int i = tid; i < (L + 1) / 2; i += 256) cnt[i] = 0u;
    __syncthreads();
    for (int t = tid; t < N; t += 256) {
        int rrow = tok_row[(int64_t)b * N + t];
        rrow = rrow < 0 ? 0 : (rrow > L - 1 ? L - 1 : rrow);
        stok[t] = (uint16_t)rrow;
        if (dmask) atomicAdd(&cnt[rrow >> 1], 1u << ((rrow & 1) << 4));          // (N < 65536: a count never carries into its neighbour)
    }
    for (int j = tid; j < Ln; j += 256) {
        const int i = src_next[d0 + j];
        if (i >= 0 && i < L) inv[i] = (uint16_t)j;
    }
    if (tid == 0) { dm_row[s0] = 0.f; dm_row[s0 + L - 1] = 0.f; }
    __syncthreads();
    if (dmask) {          // (uniform)
        for (int t = tid; t < N; t += 256) {               // rows of one token: the token's own value
            const int rrow = stok[t];
            if (((cnt[rrow >> 1] >> ((rrow & 1) << 4)) & 0xffffu) == 1u) dms[rrow] = 0.f + dmask[(int64_t)b * N + t];
        }
        for (int i = 1 + wave; i < L - 1; i += 4) {        // live rows of several tokens: this wave owns the row and adds in token order
            const unsigned jn = inv[i];
            if (((cnt[i >> 1] >> ((i & 1) << 4)) & 0xffffu) < 2u || jn < 1u || jn >= (unsigned)(Ln - 1)) continue;      // (wave-uniform)
            float s = 0.f;
            for (int t0 = 0; t0 < N; t0 += 64) {
                const int t = t0 + lane;
                const bool hit = t < N && stok[t] == i;
                const float v = hit ? dmask[(int64_t)b * N + t] : 0.f;
                unsigned long long hits = __ballot(hit);
                while (hits) {                             // (uniform)
                    const int src_lane = __builtin_ctzll(hits);
                    s += __shfl(v, src_lane, 64);
                    hits &= hits - 1ull;
                }
            }
            if (lane == 0) dms[i] = s;
        }
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
        const int jn = inv[i] == PV_SPLT_NONE ? -1 : (int)inv[i];      // (wave-uniform)
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
    // combine the four waves: dwg partial of the image (wave 0 adds wave 1's, then wave 2's, then wave 3's), dbg, dthr
    if (lane == 0) { red_s[wave][0] = dbg; red_s[wave][1] = dthr; }      // every lane of a wave holds the same dbg / dthr
    for (int w = 1; w < 4; ++w) {
        __syncthreads();                           // the buffer's previous readers are done (the first time: the counts' and the token table's)
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) red_w[lane + 64 * j] = acc[j];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const float4 tw = red_w[lane + 64 * j];
                acc[j].x += tw.x; acc[j].y += tw.y; acc[j].z += tw.z; acc[j].w += tw.w;
            }
        }
    }
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
                reinterpret_cast<float4*>(dwg_part + (int64_t)b * D)[idx] = acc[j];
                const float4 xv = xb4[idx], gv = g4[idx], w = reinterpret_cast<const float4*>(wb)[idx];
                d4[idx] = make_float4(gv.x + du * w.x, gv.y + du * w.y, gv.z + du * w.z, gv.w + du * w.w);
                reinterpret_cast<float4*>(dwb_part + (int64_t)b * D)[idx] = make_float4(du * xv.x, du * xv.y, du * xv.z, du * xv.w);
            }
        }
        if (lane == 0) { scal_part[b * 4] = dbg_t; scal_part[b * 4 + 1] = du; scal_part[b * 4 + 2] = 0.f; scal_part[b * 4 + 3] = 0.f; }
    }
}

extern "C" int pv_residual_pack_step_long_bwd(const float* x, const int32_t* seg_start, const int32_t* tok_row, const float* mask_row, const float* gate_arg,
                                              const float* thr, const int32_t* seg_next, const int32_t* src_next, const float* g_next,
                                              const float* drow_scale, const float* dmask, int64_t B, int64_t N, int64_t D, const float* wg, const float* wb,
                                              float temp, float* dx, float* dm_row, float* dwg_part, float* dwb_part, float* scal_part, void* stream) {
    if (!x || !seg_start || !tok_row || !mask_row || !gate_arg || !thr || !seg_next || !src_next || !g_next || !drow_scale || !wg || !wb || !dx || !dm_row ||
        !dwg_part || !dwb_part || !scal_part || B <= 0 || N < 0 || D <= 0 || temp == 0.f)
        return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x | (uintptr_t)g_next | (uintptr_t)dx | (uintptr_t)wg | (uintptr_t)wb | (uintptr_t)dwg_part | (uintptr_t)dwb_part | (uintptr_t)scal_part) & 15)
        return PV_ERR_INVALID_ARG;
    if (x == dx || g_next == dx) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096 || N + 2 > PV_SPARSE_LONG_MAX_LEN || B > 0x7fffffff) return PV_ERR_UNSUPPORTED;
#define SPLB_LAUNCH(NC) PV_LAUNCH(pv_spl_pack_bwd_kernel<NC>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, x, seg_start, tok_row, (int)N, (int)D, mask_row, \
                                  gate_arg, thr, seg_next, src_next, g_next, drow_scale, dmask, wg, wb, temp, dx, dm_row, dwg_part, dwb_part, scal_part)
    PV_DISPATCH_NCH(D, SPLB_LAUNCH);
#undef SPLB_LAUNCH
    return pv_check_launch();
}
