// Shared device helpers for the SpeechCLIP hot-path kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/speechclip_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef unsigned short bf16_t;  // raw storage type used in signatures

#define SC_WAVE 64

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
    __bf16 b = (__bf16)f;  // RNE; lowers to v_cvt_pk_bf16_f32 on gfx950
    return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ uint32_t pack2bf(float a, float b) {
    bf16x2_t v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float lo2f(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi2f(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// IEEE half as the second 16-bit operand format (round 6): the pre-LN encoder layers of HuBERT-large keep their GEMM / attention operands in f16 (11 significand
// bits instead of bf16's 8: the reference's own GPU precision for these models is fp16 autocast, config/speechCLIP/model_large/coco/spchclp_p.yaml:122).  The
// kernels that take both formats are templates on F16; everything format-dependent goes through these four helpers (conversion: v_cvt_pk_f16_f32, RNE).
typedef _Float16 sc_half2v_t __attribute__((ext_vector_type(2)));
typedef _Float16 sc_half8v_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pack2h(float a, float b) {
    sc_half2v_t v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, v);
}
template <bool F16> __device__ __forceinline__ uint32_t pack2x(float a, float b) {
    if constexpr (F16) return pack2h(a, b); else return pack2bf(a, b);
}
template <bool F16> __device__ __forceinline__ float lo2fx(uint32_t u) {
    if constexpr (F16) return (float)__builtin_bit_cast(sc_half2v_t, u)[0]; else return lo2f(u);
}
template <bool F16> __device__ __forceinline__ float hi2fx(uint32_t u) {
    if constexpr (F16) return (float)__builtin_bit_cast(sc_half2v_t, u)[1]; else return hi2f(u);
}
template <bool F16> __device__ __forceinline__ f32x4_t mfma_16x16x32(bf16x8_t a, bf16x8_t b, f32x4_t c) {      // operands as raw 16-bit x 8 registers
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(sc_half8v_t, a), __builtin_bit_cast(sc_half8v_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16> __device__ __forceinline__ f32x16_t mfma_32x32x16(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sc_half8v_t, a), __builtin_bit_cast(sc_half8v_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// erf via Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7): 1 rcp + 1 exp + a handful of FMAs.
__device__ __forceinline__ float fast_erf(float x) {
    float ax = fabsf(x);
    float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float poly = fmaf(fmaf(fmaf(fmaf(1.061405429f, t, -1.453152027f), t, 1.421413741f), t, -0.284496736f), t, 0.254829592f) * t;
    float r = 1.0f - poly * __expf(-ax * ax);
    return copysignf(r, x);
}
// erf-GELU (torch.nn.functional.gelu / fairseq "gelu") in the epilogues: x * sigmoid(a x + b x^3 + c x^5), least-squares fit of the
// EXACT erf form on [-6, 6]: max |err| 3.0e-5 (1/30 of a bf16 half-ulp at 1.0; the tanh form is 4.7e-4).  7 plain VALU ops + v_exp +
// v_rcp instead of ~16 + 2 for the A&S erf; the argument is clamped to [-8, 8] (the odd quintic changes sign beyond |x| ~ 10).
// gelu_erf_precise keeps the 1.5e-7 erf path for fp32 consumers.
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
#define SC_GELU_A (-1.59491694f * 1.44269504f)
#define SC_GELU_B (-0.0741006897f * 1.44269504f)
#define SC_GELU_C (7.17464634e-4f * 1.44269504f)
__device__ __forceinline__ float gelu_erf(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -8.0f, 8.0f);
    const float x2 = xc * xc;
    const float z = xc * fmaf(x2, fmaf(x2, SC_GELU_C, SC_GELU_B), SC_GELU_A);   // = -log2(e) * (a x + b x^3 + c x^5)
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z));
}
__device__ __forceinline__ f32x2_t gelu_erf2(f32x2_t x) {   // two values: the polynomial part packs into v_pk_* ops
    f32x2_t xc = {__builtin_amdgcn_fmed3f(x[0], -8.0f, 8.0f), __builtin_amdgcn_fmed3f(x[1], -8.0f, 8.0f)};
    const f32x2_t x2 = xc * xc;
    const f32x2_t z = xc * (x2 * (x2 * SC_GELU_C + SC_GELU_B) + SC_GELU_A);
    f32x2_t d = {1.0f + __builtin_amdgcn_exp2f(z[0]), 1.0f + __builtin_amdgcn_exp2f(z[1])};
    f32x2_t r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    return x * r;
}
// Transcendental-free form for the GEMM epilogues (v_exp/v_rcp are not packable; everything below is v_pk_fma_f32/v_pk_mul_f32, two
// values per issue): Phi(x) = 0.5 + xc * g(t), xc = clamp(x, +-4.25), t = 2 xc^2 / 4.25^2 - 1 in [-1, 1], g = degree-8 minimax
// polynomial (weighted for the error of x * Phi).  max |err| 1.7e-5 on [-4.25, 4.25]; outside, Phi(+-4.25) = 1 - 7e-6 / 7e-6
// (relative error 7e-6 on the positive side, |x| * 7e-6 absolute on the negative side).
#define SC_GELU_P_C 4.25f
#define SC_GELU_P_S 0.11072665f
#ifndef SC_GELU_F16
#define SC_GELU_F16 1
#endif
#if SC_GELU_F16
// Default since round 3 (-DSC_GELU_F16=0: the fp32 degree-8 form below).  The GELU of every bf16-OUTPUT epilogue (conv stack, fc1, conv layer 0) is
// evaluated in PACKED HALF precision (v_pk_*_f16: two elements per lane per full-rate instruction instead of one half-rate packed-fp32
// instruction): Phi(x) = 0.5 + xc g(t), xc = clamp(x, +-4), t = xc^2 / 8 - 1, g = degree-6 minimax; the conversion to half rounds toward zero, so
// |x| > 65504 saturates instead of overflowing.  Against the exact erf form (numpy float16 simulation, 2.2 M samples) the bf16-ROUNDED result has
// 1.06x the rms error of rounding the exact value to bf16 (absolute error <= ~1e-3, in the negative tail where 0.5 + xc g cancels in half
// precision): below the resolution of the bf16 activations it feeds.  Measured: -0.62 ms per step (44.52-44.56 vs 45.07-45.21, three interleaved
// passes), end-to-end parity metrics unchanged (centred cosines 0.9925-0.9995 on the same fixtures, loss equal to 5 digits).
// Round 6: degree 4 (default): 11 instead of 13 VALU instructions per value pair in the VALU-bound GELU epilogue.  The fit is a DENSITY-WEIGHTED least-squares
// fit of the error of x Phi on |x| <= 3.2 (weight: the mixture N(0, 0.6^2) / N(0, 1.5^2) that brackets the pre-activations of the conv stack and of fc1), not a
// minimax one: an approximation error is a smooth function of x, i.e. SYSTEMATIC -- it adds up coherently in the next GEMM's K sum where rounding noise averages
// out.  Measured in the fp32 oracle with only the GELU replaced (P-base, 4 pairs; 1 - mean centred cosine of the audio embedding): output rounding to bf16 alone
// 4.7e-4, degree 6 5.9e-4, this fit 6.6e-4, the minimax degree-4 fit tried first 2.1e-3 (the same minimax fit on the GPU: bench parity_check 0.99659 -> 0.99425).
// Beyond the fitted range the even-degree g with its positive leading coefficient grows and the clamp of Phi saturates, as for degree 6.  Numpy float16 simulation
// of this exact instruction sequence on EVERY finite bf16 input (tests/test_gemm8p_gpu.py feeds them through the kernel): rms error 1.035x the rms of rounding the
// exact erf-GELU to bf16 (degree 6: 1.015x), worst |error| / test tolerance 0.70, saturation exact beyond |x| = 5.5.  -DSC_GELU_DEG=6: rounds 3-5.
#ifndef SC_GELU_DEG
#define SC_GELU_DEG 4
#endif
#ifndef SC_GELU_TCLAMP        // 1: clamp the polynomial argument t to <= 1 (rounds 3-5); 0: rely on the Phi clamp alone (see gelu_poly2)
#define SC_GELU_TCLAMP (SC_GELU_DEG % 2 == 0 ? 0 : 1)
#endif
typedef _Float16 sc_half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t gelu_poly2(f32x2_t x) {
    // y = x Phi(x), Phi = clamp(1/2 + x g(t), 0, 1), t = x^2 / 8 - 1.  NOTHING but Phi is clamped (the VOP3P clamp bit of the v_pk_fma that forms it):
    // beyond |x| = 4 (t > 1) the even-degree g with its positive leading coefficient only grows, x g(t) leaves [-1/2, 1/2] and the clamp pins Phi to
    // 0 / 1; x^2 overflowing to +inf (|x| > 255) keeps every Horner step at +inf and Phi at clamp(+-inf).  (Rounds 3-5 also clamped t with a v_pk_min:
    // bit-identical results on every finite half input, tests/test_gemm8p_gpu.py::test_gelu_epilogue_every_bf16_input, 7 % of the epilogue's VALU work.)
    // The last product is formed in fp32 from the half operands (v_fma_mix_f32), which is also the conversion the bf16 pack needs.
    const sc_half2_t h = __builtin_bit_cast(sc_half2_t, __builtin_amdgcn_cvt_pkrtz(x[0], x[1]));
    const sc_half2_t one = {(_Float16)1.0f, (_Float16)1.0f}, zero = {(_Float16)0.0f, (_Float16)0.0f};
#if SC_GELU_TCLAMP
    const sc_half2_t t = __builtin_elementwise_min(h * h * (_Float16)0.125f - (_Float16)1.0f, one);
#else
    const sc_half2_t t = h * h * (_Float16)0.125f - (_Float16)1.0f;
#endif
#if SC_GELU_DEG == 4
    sc_half2_t g = t * (_Float16)0.067138671875f + (_Float16)-0.01300048828125f;
    g = g * t + (_Float16)0.055389404296875f;
    g = g * t + (_Float16)-0.08575439453125f;
    g = g * t + (_Float16)0.1759033203125f;
#elif SC_GELU_DEG == 5
    sc_half2_t g = t * (_Float16)-1.177580447e-02f + (_Float16)2.993807372e-02f;
    g = g * t + (_Float16)-3.959858472e-02f;
    g = g * t + (_Float16)5.414790186e-02f;
    g = g * t + (_Float16)-8.377277171e-02f;
    g = g * t + (_Float16)1.760021146e-01f;
#else
    sc_half2_t g = t * (_Float16)5.972025641e-03f + (_Float16)-1.655089296e-02f;
    g = g * t + (_Float16)2.409105964e-02f;
    g = g * t + (_Float16)-3.546234617e-02f;
    g = g * t + (_Float16)5.541019052e-02f;
    g = g * t + (_Float16)-8.442661829e-02f;
    g = g * t + (_Float16)1.759702165e-01f;
#endif
    const sc_half2_t phi = __builtin_elementwise_min(__builtin_elementwise_max(h * g + (_Float16)0.5f, zero), one);
    // (as asm: left to the compiler, one of the two epilogue copies converts all four halves and SLP-packs the products into v_pk_fma_f32)
    f32x2_t y;
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,1,0]" : "=v"(y[0]) : "v"(h), "v"(phi));
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "=v"(y[1]) : "v"(h), "v"(phi));
    return y;
}
// Eight pairs at once, every Horner step issued for all eight before the next step: identical arithmetic to gelu_poly2 per pair (bit-identical results),
// but the dependent v_pk_fma_f16 chain of one pair (latency + a hazard nop per step) is hidden behind the seven other pairs.  hipcc schedules the per-pair
// form one or two chains at a time: the GELU epilogue of a 256 x 256 tile was latency-bound (512 v_pk_fma_f16 + 372 s_nop per wave), round 5.
// XF32 (the f16-output epilogues): the last product takes the ORIGINAL fp32 x instead of its truncated half copy -- a result that keeps 11 significand bits would
// otherwise carry the systematic -1/2 ulp of the round-toward-zero conversion (invisible behind a bf16 rounding, not behind an f16 one).
template <bool XF32 = false>
__device__ __forceinline__ void gelu_poly2_x8(f32x2_t (&x)[8]) {
    const sc_half2_t one = {(_Float16)1.0f, (_Float16)1.0f}, zero = {(_Float16)0.0f, (_Float16)0.0f};
    sc_half2_t h[8], t[8], g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = __builtin_bit_cast(sc_half2_t, __builtin_amdgcn_cvt_pkrtz(x[i][0], x[i][1]));
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = h[i] * h[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = SC_GELU_TCLAMP ? __builtin_elementwise_min(t[i] * (_Float16)0.125f - (_Float16)1.0f, one) : t[i] * (_Float16)0.125f - (_Float16)1.0f;
#if SC_GELU_DEG == 4
    const float c[5] = {0.067138671875f, -0.01300048828125f, 0.055389404296875f, -0.08575439453125f, 0.1759033203125f};
    constexpr int NC = 5;
#elif SC_GELU_DEG == 5
    const float c[6] = {-1.177580447e-02f, 2.993807372e-02f, -3.959858472e-02f, 5.414790186e-02f, -8.377277171e-02f, 1.760021146e-01f};
    constexpr int NC = 6;
#else
    const float c[7] = {5.972025641e-03f, -1.655089296e-02f, 2.409105964e-02f, -3.546234617e-02f, 5.541019052e-02f, -8.442661829e-02f, 1.759702165e-01f};
    constexpr int NC = 7;
#endif
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = t[i] * (_Float16)c[0] + (_Float16)c[1];
#pragma unroll
    for (int k = 2; k < NC; ++k) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = g[i] * t[i] + (_Float16)c[k];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = __builtin_elementwise_min(__builtin_elementwise_max(h[i] * g[i] + (_Float16)0.5f, zero), one);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (XF32) {
            asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[0,1,0]" : "=v"(x[i][0]) : "v"(x[i][0]), "v"(g[i]));
            asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(x[i][1]) : "v"(x[i][1]), "v"(g[i]));
        } else {
        asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,1,0]" : "=v"(x[i][0]) : "v"(h[i]), "v"(g[i]));
        asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "=v"(x[i][1]) : "v"(h[i]), "v"(g[i]));
        }
    }
}
#endif
// fp32 degree-8 form (max |err| 1.7e-5): what every f32-OUTPUT epilogue uses (the packed-half form above carries ~11 bits and is meant for
// results that are rounded to bf16 right away), and the bf16 epilogues too with -DSC_GELU_F16=0.
__device__ __forceinline__ f32x2_t gelu_poly2_f32(f32x2_t x) {
    const f32x2_t xc = {__builtin_amdgcn_fmed3f(x[0], -SC_GELU_P_C, SC_GELU_P_C), __builtin_amdgcn_fmed3f(x[1], -SC_GELU_P_C, SC_GELU_P_C)};
    const f32x2_t t = xc * xc * SC_GELU_P_S - 1.0f;
    f32x2_t g = t * 2.012408951e-03f + -6.027759260e-03f;
    g = g * t + 9.229262475e-03f;
    g = g * t + -1.461630908e-02f;
    g = g * t + 2.532269481e-02f;
    g = g * t + -3.916527947e-02f;
    g = g * t + 5.573306025e-02f;
    g = g * t + -8.077754797e-02f;
    g = g * t + 1.659348977e-01f;
    return x * (xc * g + 0.5f);
}
#if !SC_GELU_F16
__device__ __forceinline__ f32x2_t gelu_poly2(f32x2_t x) { return gelu_poly2_f32(x); }
#endif
__device__ __forceinline__ float gelu_erf_precise(float x) { return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752f)); }
// Counter-based dropout masks: element idx of a tensor is kept iff hash(seed, idx) >= thresh (thresh = p * 2^32); the backward regenerates the
// mask from (seed, idx) instead of storing it.
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool keep_elem(uint32_t seed, uint32_t idx, uint32_t thresh) { return hash32(seed ^ hash32(idx + 0x9e3779b9U)) >= thresh; }
static inline uint32_t drop_thresh(float pd) { return pd <= 0.f ? 0u : (uint32_t)fmin(4294967295.0, (double)pd * 4294967296.0); }
// Attention-probability dropout: the flash kernel is VALU-bound, so ONE hash serves a PAIR of adjacent keys of a query row (16 random bits each):
// pair index = row_id * ceil(L / 2) + (key >> 1), row_id = (b*H + h)*L + query; key parity picks the half.  thresh16 = p * 2^16.
__device__ __forceinline__ uint32_t hash_pair(uint32_t seed, uint32_t pair_idx) { return hash32(pair_idx * 0x9E3779B1u + seed); }
static inline uint32_t drop_thresh16(float pd) { return pd <= 0.f ? 0u : (uint32_t)fmin(65535.0, (double)pd * 65536.0); }
// CLIP QuickGELU: x * sigmoid(1.702 x)
__device__ __forceinline__ float quick_gelu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x)); }

// What the GEMM kernels (gemm.hip, gemm8p.hip) share.
// LDS-DMA: 16 bytes per lane from global memory straight into LDS, lane L to lds_wave_base + 16 L.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// The activation (ACT: SC_ACT_*) of a GEMM epilogue on four consecutive results of a row, the one statement of it.  F32: the fp32 polynomial of GELU for
// fp32 outputs (the packed-half form carries ~11 bits, meant for 16-bit results).
template <int ACT, bool F32>
__device__ __forceinline__ f32x4_t epi_act(f32x4_t v4) {
    if (ACT == SC_ACT_GELU) {
        const f32x2_t g0 = F32 ? gelu_poly2_f32((f32x2_t){v4[0], v4[1]}) : gelu_poly2((f32x2_t){v4[0], v4[1]});
        const f32x2_t g1 = F32 ? gelu_poly2_f32((f32x2_t){v4[2], v4[3]}) : gelu_poly2((f32x2_t){v4[2], v4[3]});
        v4 = (f32x4_t){g0[0], g0[1], g1[0], g1[1]};
    } else if (ACT == SC_ACT_QUICKGELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v4[r] = quick_gelu(v4[r]);
    }
    return v4;
}
// Residual add on one packed pair of 16-bit results: o + r in fp32, rounded again.
template <bool F16> __device__ __forceinline__ uint32_t add_packed(uint32_t o, uint32_t r) {
    return pack2x<F16>(lo2fx<F16>(o) + lo2fx<F16>(r), hi2fx<F16>(o) + hi2fx<F16>(r));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// error plumbing (host)
void sc_set_error(const char* fmt, ...);
#define SC_CHECK_ARG(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            sc_set_error(__VA_ARGS__);     \
            return -1;                     \
        }                                  \
    } while (0)
#define SC_CHECK_LAUNCH()                                                   \
    do {                                                                    \
        hipError_t e_ = hipGetLastError();                                  \
        if (e_ != hipSuccess) {                                             \
            sc_set_error("%s:%d launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return -2;                                                      \
        }                                                                   \
    } while (0)
