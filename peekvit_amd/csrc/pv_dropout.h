// The dropout mask of the training path: a STATELESS, layout-free decision per element.  Nothing is stored - the forward and both backward launches
// of a site call the same function again - so a mask costs no memory and no second pass, and the kernels may visit a site's elements in any lane
// layout.  include/peekvit_hip_dropout.h is the C ABI, tests/dropout_ref.py the same arithmetic in numpy (bit for bit), DESIGN.md section 31 the why.
//
//   keep(key, site, row, col)     key   64 bits, drawn once per training pass (train_engine.dropout_key)
//                                 site  64 bits, the number of the dropout site inside the pass (call order)
//                                 row   element sites [rows, D]: the token row; attention sites [B H S, S]: (b H + h) S + q
//                                 col   the channel; the key index k
//
// Bit by bit (all arithmetic modulo 2^64 / 2^32):
//   sm(z)   splitmix64's finaliser:  z += 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
//                                    return z ^ z >> 31
//   lb(x)   lowbias32:               x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  return x ^ x >> 16
//   base = sm(key ^ sm(site))                                        on the HOST, once per launch (pv_drop_base)
//   rk   = sm(base ^ row * 0xD1B54A32D192ED03)                       once per row (pv_drop_row_key): the 64-bit part
//   w    = lb((lo32(rk) + col * 0x9E3779B1) ^ hi32(rk))              per element: two 32-bit multiplies and five ALU operations
//   keep iff w >= thr,  thr = floor(p * 2^32)  (p fp32, the product in fp64: exact)               P(drop) = thr / 2^32, within 2^-32 of p
// Survivors are multiplied by the fp32 value 1 / (1 - p).  p = 0: thr = 0, every element is kept and the factor is 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PV_DROP_FN __host__ __device__ __forceinline__
#else
#define PV_DROP_FN static inline
#endif

PV_DROP_FN uint64_t pv_drop_sm64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

PV_DROP_FN uint32_t pv_drop_lb32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    return x ^ (x >> 16);
}

PV_DROP_FN uint64_t pv_drop_base(uint64_t key, uint64_t site) { return pv_drop_sm64(key ^ pv_drop_sm64(site)); }

PV_DROP_FN uint64_t pv_drop_row_key(uint64_t base, uint64_t row) { return pv_drop_sm64(base ^ (row * 0xD1B54A32D192ED03ull)); }

// the element's 32-bit word from the two halves of its row key
PV_DROP_FN uint32_t pv_drop_word(uint32_t rk_lo, uint32_t rk_hi, uint32_t col) { return pv_drop_lb32((rk_lo + col * 0x9E3779B1u) ^ rk_hi); }

PV_DROP_FN bool pv_drop_keep(uint32_t rk_lo, uint32_t rk_hi, uint32_t col, uint32_t thr) { return pv_drop_word(rk_lo, rk_hi, col) >= thr; }

// what a launch carries instead of (key, site, p): formed on the host by the entry points
struct PvDrop {
    uint64_t base;      // pv_drop_base(key, site)
    uint32_t thr;       // floor(p * 2^32)
    float scale;        // 1 / (1 - p), fp32
    float omp;          // 1 - p, fp32 (the forward's inv = 1 / (l (1 - p)))
};

static inline bool pv_drop_p_ok(float p) { return p >= 0.f && p < 1.f; }          // (false for a NaN)

static inline PvDrop pv_drop_make(uint64_t key, uint64_t site, float p) {
    PvDrop d;
    d.base = pv_drop_base(key, site);
    d.thr = (uint32_t)((double)p * 4294967296.0);          // p < 1 in fp32: the product is below 2^32 and exact in fp64
    d.omp = 1.0f - p;
    d.scale = 1.0f / d.omp;
    return d;
}
