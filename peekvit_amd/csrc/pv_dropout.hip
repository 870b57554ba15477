// Dropout row kernels of the training path on gfx950 (include/peekvit_hip_dropout.h): the encoder-input site, the branch
// site's residual add and its backward, and the mask as bytes for the tests.  One wave per row (pv_rows.h: the row in registers, guarded row stores),
// so the 64-bit part of the mask - the row key - is formed once per row; an element costs pv_drop_keep's two 32-bit multiplies.  HBM-bound: fp32 row
// kernels under register loads, built with pv_rowops.hip's flags.  Vector stores only, no atomics.
#include "pv_common.h"
#include "pv_rows.h"
#include "pv_dropout.h"
#include "../../include/peekvit_hip_dropout.h"

// the lane's 16-bit chunks of a row as floats (chunk = four values; lanes beyond nvec keep zeros)
template <int NCH>
__device__ __forceinline__ void pv_load_row16(RowRegs<NCH>& r, const uint16_t* ur, int nvec, int lane) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int idx = lane + 64 * j;
        u32x2 w = {0u, 0u};
        if (idx < nvec) w = reinterpret_cast<const u32x2*>(ur)[idx];
        r.v[j] = make_float4(pv_unpack_lo(w[0]), pv_unpack_hi(w[0]), pv_unpack_lo(w[1]), pv_unpack_hi(w[1]));
    }
}

// v <- v o keep * scale on the lane's chunks of row `row`
template <int NCH>
__device__ __forceinline__ void pv_drop_row(RowRegs<NCH>& r, uint64_t rk, uint32_t thr, float scale, int lane) {
    const uint32_t lo = (uint32_t)rk, hi = (uint32_t)(rk >> 32);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const uint32_t col = 4u * (uint32_t)(lane + 64 * j);
        r.v[j].x = pv_drop_keep(lo, hi, col, thr) ? r.v[j].x * scale : 0.f;
        r.v[j].y = pv_drop_keep(lo, hi, col + 1, thr) ? r.v[j].y * scale : 0.f;
        r.v[j].z = pv_drop_keep(lo, hi, col + 2, thr) ? r.v[j].z * scale : 0.f;
        r.v[j].w = pv_drop_keep(lo, hi, col + 3, thr) ? r.v[j].w * scale : 0.f;
    }
}

// MODE 0: out = x o keep * scale     1: out = fma(float(u) o keep, scale, x)     2: out16 = round16(float(u) o keep * scale)
// (x and out may be the same array: a lane reads its chunks of a row before it writes them - no __restrict__ on either)
template <int NCH, int MODE>
__global__ __launch_bounds__(256) void pv_dropout_rows_kernel(const float* x, const uint16_t* u, float* out, uint16_t* out16, PvDrop dr, int64_t rows, int D) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nvec = D >> 2;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wid; row < rows; row += (int64_t)gridDim.x * 4) {
        const uint64_t rk = pv_drop_row_key(dr.base, (uint64_t)row);
        RowRegs<NCH> r;
        if constexpr (MODE == 0) {
            pv_load_row<NCH>(r, x + row * D, nvec, lane);
            pv_drop_row<NCH>(r, rk, dr.thr, dr.scale, lane);
            pv_store_row<NCH>(out + row * D, r, nvec, lane);
        } else if constexpr (MODE == 1) {
            RowRegs<NCH> xr;
            pv_load_row<NCH>(xr, x + row * D, nvec, lane);
            pv_load_row16<NCH>(r, u + row * D, nvec, lane);
            pv_drop_row<NCH>(r, rk, dr.thr, 1.0f, lane);          // (the mask alone: u or 0, exactly)
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                r.v[j] = make_float4(fmaf(r.v[j].x, dr.scale, xr.v[j].x), fmaf(r.v[j].y, dr.scale, xr.v[j].y), fmaf(r.v[j].z, dr.scale, xr.v[j].z),
                                     fmaf(r.v[j].w, dr.scale, xr.v[j].w));
            pv_store_row<NCH>(out + row * D, r, nvec, lane);
        } else {
            pv_load_row16<NCH>(r, u + row * D, nvec, lane);
            pv_drop_row<NCH>(r, rk, dr.thr, dr.scale, lane);
            pv_store_row16<NCH>(out16 + row * D, r, nvec, lane);
        }
    }
}

__global__ __launch_bounds__(256) void pv_dropout_keep_u8_kernel(uint8_t* __restrict__ keep, PvDrop dr, int64_t rows, int64_t cols) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * cols; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / cols;
        const uint64_t rk = pv_drop_row_key(dr.base, (uint64_t)row);
        keep[e] = pv_drop_keep((uint32_t)rk, (uint32_t)(rk >> 32), (uint32_t)(e - row * cols), dr.thr) ? 1 : 0;
    }
}

template <int MODE>
static int pv_launch_dropout_rows(const float* x, const uint16_t* u, float* out, uint16_t* out16, const PvDrop& dr, int64_t rows, int64_t D, hipStream_t s) {
    const unsigned grid = pv_stream_grid(rows, 4);
#define PV_DROP_CASE(N) PV_LAUNCH((pv_dropout_rows_kernel<N, MODE>), dim3(grid), dim3(256), 0, s, x, u, out, out16, dr, rows, (int)D)
    PV_DISPATCH_NCH(D, PV_DROP_CASE);
#undef PV_DROP_CASE
    return pv_check_launch();
}

extern "C" int pv_dropout_keep_u8(uint8_t* keep, uint64_t key, uint64_t site, int64_t rows, int64_t cols, float p, void* stream) {
    if (!keep || rows <= 0 || cols <= 0 || !pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (cols > 0xffffffffll || rows > (int64_t)0x7fffffffffffffffll / cols) return PV_ERR_UNSUPPORTED;
    PV_LAUNCH(pv_dropout_keep_u8_kernel, dim3(pv_stream_grid(rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, keep, pv_drop_make(key, site, p), rows, cols);
    return pv_check_launch();
}

extern "C" int pv_dropout_f32(const float* x, float* out, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream) {
    if (!x || !out || rows <= 0 || D <= 0 || !pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    return pv_launch_dropout_rows<0>(x, nullptr, out, nullptr, pv_drop_make(key, site, p), rows, D, (hipStream_t)stream);
}

extern "C" int pv_dropout_residual(const float* x, const uint16_t* u, float* out, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream) {
    if (!x || !u || !out || rows <= 0 || D <= 0 || !pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)u & 7)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    return pv_launch_dropout_rows<1>(x, u, out, nullptr, pv_drop_make(key, site, p), rows, D, (hipStream_t)stream);
}

extern "C" int pv_dropout_bwd16(const uint16_t* d, uint16_t* du, uint64_t key, uint64_t site, int64_t rows, int64_t D, float p, void* stream) {
    if (!d || !du || d == du || rows <= 0 || D <= 0 || !pv_drop_p_ok(p)) return PV_ERR_INVALID_ARG;
    if (((uintptr_t)d & 7) || ((uintptr_t)du & 7)) return PV_ERR_INVALID_ARG;
    if (D % 4 || D > 4096) return PV_ERR_UNSUPPORTED;
    return pv_launch_dropout_rows<2>(nullptr, d, nullptr, du, pv_drop_make(key, site, p), rows, D, (hipStream_t)stream);
}
