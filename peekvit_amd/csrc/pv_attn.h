// What the attention sources share (pv_attention.hip: the forward kernels and the LDS-resident backward kernels; pv_attention_stream.hip: the
// streaming backward kernels and the streaming training entry points): the LDS swizzle, the probability scale of the fp16 build and the
// launcher of the streaming forward.  The 16-bit packers are pv_common.h's.
#pragma once
#include "pv_common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8;

template <int CPR>   // 16-byte chunks per row (DHP / 8)
__device__ __forceinline__ int pv_swz(int row, int chunk) {
    const int L = row * CPR + chunk, line = L >> 3, pos = L & 7;
    return ((line << 3) + (pos ^ (line & 7))) << 4;
}

// Probabilities are packed as p * 2^PV_P_SHIFT in the fp16 build (the fp16 MFMA flushes subnormal operands; the factor cancels in O / l).
// Round 4: 2^10 instead of round 3's 2^14 - p <= 1 leaves SIX bits of fp16 headroom instead of two (an exponent computed against a
// maximum that is off by up to 4 score units still packs a finite value; round 3's carried-maximum experiment turned exactly such
// values into inf and then NaN rows), and everything down to p = 6e-8 stays a normal number: at most 197 x 6e-8 = 1.2e-5 of a row's
// mass can flush, two orders below the contract.  The streaming kernel (S > 416, wide heads) now applies the same scale.
#include "pv_dropout.h"
#ifndef PV_P_SHIFT
#ifdef PV_OPERAND_F16
#define PV_P_SHIFT 10.0f
#else
#define PV_P_SHIFT 0.0f
#endif
#endif
#define PV_P_UNSHIFT (1.0f / (float)(1 << (int)PV_P_SHIFT))       // 2^-PV_P_SHIFT, exact

// pv_attn_stream_kernel<dh, LSE = true> (pv_attention.hip) for dh = 32 / 48 / 64 at ANY S >= 1: out and the rows' log2-sum-exp.  Arguments are the
// caller's to check; PV_ERR_UNSUPPORTED for another dh or more than 2^31 - 1 workgroups.
int pv_launch_attn_stream_lse(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int S, int H, int dh, uint32_t* flag, hipStream_t stream);
int pv_launch_attn_stream_lse_w(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int S, int H, int dh, uint32_t* flag, float tail_log_mult,
                                hipStream_t stream);
// the DROP instantiation of the same kernel (pv_attention_stream_lse_drop_bf16): dropout on the probabilities, the mask of pv_dropout.h
int pv_launch_attn_stream_lse_drop(const uint16_t* qkv, uint16_t* out, float* lse, int64_t B, int S, int H, int dh, uint32_t* flag, const PvDrop& dr,
                                   hipStream_t stream);
// pv_attn_stream_var_lse_kernel<64> (pv_attention.hip): the LSE + VAR instantiation of the streaming body - pv_attention_varlen_w_stream_bf16's `out`
// and the rows' log2-sum-exp, the key weights included, lse fp32 [R, H].  dh = 64, any max_len >= 1; PV_ERR_UNSUPPORTED above 2^31 - 1 workgroups.
int pv_launch_attn_stream_var_lse(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg, const float* lmul, int64_t B, int max_len, int H,
                                  uint32_t* flag, hipStream_t stream);
// pv_attn_kernel<64, ceil(max_len / 16), LSE, VAR, WLOG> (pv_attention.hip): pv_attention_varlen_w_bf16's kernel body with the rows' log2-sum-exp
// (lse fp32 [R, H], the key weights included).  dh = 64; PV_ERR_UNSUPPORTED for max_len > 208.
int pv_launch_attn_varlen_w_lse(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* seg, const float* lmul, int64_t B, int max_len, int H, uint32_t* flag,
                                hipStream_t stream);
