// Device helpers of the Moffat fits (k_fit in stamps.hip, k_fit_ell in fit_ell.hip): wave-wide sums on the
// DPP path and the reciprocal, square-root, exp and log forms of the Levenberg-Marquardt iterations and their
// fp64 polish.  Everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

namespace mpsfr {
namespace {

// Wave-wide sums for the fit, on the DPP path instead of ds_bpermute shuffles (21 sums per model
// evaluation; a shuffle goes through the LDS crossbar and its latency sat on the critical path of
// the serial LM iterations).  Quad swaps, half-row and row mirrors give every lane its row-of-16
// sum; row_bcast15 / row_bcast31 fold the four rows into lane 63, which is read into a scalar
// register -- the LM state is wave-uniform and lives in SGPRs.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_term(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                         0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_term(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL,
                                                              ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK,
                                                              0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
__device__ __forceinline__ float lane63(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
__device__ __forceinline__ double lane63(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
template <typename T>
__device__ __forceinline__ T wave_total(T v) {
    v += dpp_term<0xB1, 0xf>(v);     // quad_perm [1,0,3,2]
    v += dpp_term<0x4E, 0xf>(v);     // quad_perm [2,3,0,1]
    v += dpp_term<0x141, 0xf>(v);    // row_half_mirror
    v += dpp_term<0x140, 0xf>(v);    // row_mirror: every lane holds its row's sum
    // rows 1..3 add lane 15 of the row before, then rows 2, 3 add lane 31: lane 63 = s2 + s3 + (s0 + s1).
    // All rows enabled (the other lanes hold partial sums nobody reads): with a row mask the
    // compiler cannot fuse the move into the addition and each step is three instructions, not one
    v += dpp_term<0x142, 0xf>(v);    // row_bcast15
    v += dpp_term<0x143, 0xf>(v);    // row_bcast31: lane 63 holds the total
    return lane63(v);
}

template <typename RE>
__device__ __forceinline__ RE fit_log(RE x);
template <>
__device__ __forceinline__ float fit_log<float>(float x) { return __logf(x); }
template <>
__device__ __forceinline__ double fit_log<double>(double x) { return log(x); }
template <typename RE>
__device__ __forceinline__ RE fit_exp(RE x);
template <>
__device__ __forceinline__ float fit_exp<float>(float x) { return __expf(x); }
template <>
__device__ __forceinline__ double fit_exp<double>(double x) { return exp(x); }

template <typename S>
__device__ __forceinline__ S fit_rcp(S x);
template <>
__device__ __forceinline__ float fit_rcp<float>(float x) { return __builtin_amdgcn_rcpf(x); }
template <>
__device__ __forceinline__ double fit_rcp<double>(double x) { return 1.0 / x; }
template <typename S>
__device__ __forceinline__ S fit_rsqrt(S x);
template <>
__device__ __forceinline__ float fit_rsqrt<float>(float x) { return __builtin_amdgcn_rsqf(x); }
template <>
__device__ __forceinline__ double fit_rsqrt<double>(double x) {
    // hardware seed (v_rsq_f64, ~2^-26) + two Newton steps: 9 instructions where sqrt and the
    // division took ~40; the ten of a 5 x 5 factorisation were most of its cost
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}

// Lean fp64 exp / log for the polish (arguments are tame: z <= 0 for the model, x >= 1 for the
// logarithm), ~18 and ~27 instructions against ~55 and ~65 for the general library routines.
//   exp: z = k ln2 + r, |r| <= ln2 / 2, degree-10 Taylor in r (remainder r^11 / 11! < 2.2e-13 --
//        the residuals it serves only have to beat the 1e-6 of the float model), v_ldexp_f64.
//   log: l0 = hardware log2 in fp32 (error ~1e-7), then log x = l0 + log1p(d) with
//        d = x exp(-l0) - 1 ~ 1e-7, three terms of the series (remainder d^4 / 4).
__device__ __forceinline__ double lean_exp(double z) {
    z = fmax(z, -700.0);
    const double k = rint(z * 1.4426950408889634074);
    double r = fma(-k, 6.93147180369123816490e-01, z);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 3628800.0;
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}
__device__ __forceinline__ double lean_log(double x) {
    const double l0 = (double)(__builtin_amdgcn_logf((float)x) * 0.69314718f);
    const double d = fma(x, lean_exp(-l0), -1.0);
    return l0 + d * fma(d, fma(d, 1.0 / 3.0, -0.5), 1.0);
}

template <typename RE>
__device__ __forceinline__ RE fit_exp2m1(RE eta);           // 2^eta - 1, eta in (0, 100)
template <>
__device__ __forceinline__ float fit_exp2m1<float>(float eta) {
    return __builtin_amdgcn_exp2f(eta) - 1.0f;
}
template <>
__device__ __forceinline__ double fit_exp2m1<double>(double eta) {
    return lean_exp(0.69314718055994530942 * eta) - 1.0;
}

// log2 / exp2 of the model passes.  Float: the bare hardware instructions -- the argument of the
// logarithm is >= 1 and the power is in (0, 1], so the denormal scaling and the extended-precision
// ln of __logf (11 instructions per pixel of the 56 the pass had) buy nothing, and the float phase
// only has to reach the basin of the fp64 polish.
template <typename RE>
__device__ __forceinline__ RE fit_log2(RE x);
template <>
__device__ __forceinline__ float fit_log2<float>(float x) { return __builtin_amdgcn_logf(x); }
template <>
__device__ __forceinline__ double fit_log2<double>(double x) { return log(x) * 1.4426950408889634074; }
template <typename RE>
__device__ __forceinline__ RE fit_exp2(RE x);
template <>
__device__ __forceinline__ float fit_exp2<float>(float x) { return __builtin_amdgcn_exp2f(x); }
template <>
__device__ __forceinline__ double fit_exp2<double>(double x) { return exp(x * 0.69314718055994530942); }

// a wave-uniform double into scalar registers (the value of the first active lane)
__device__ __forceinline__ double sgpr(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}

}  // namespace
}  // namespace mpsfr
