// Device code shared by the fit kernels (k_fit in stamps.hip, k_fit_ell in fit_ell.hip, k_fit_obs in fit_obs.hip,
// k_fit_psf in fit_psf.hip, k_fit_group in fit_group_impl.h, k_fit_spec in fit_spec.hip): wave-wide sums on the DPP
// path; the shared intake of the weighted fits, at the end of the file (fit_pixel, wave_first_max, FitStarScan, the
// refusal rules, FitNorm; wave_first_max also serves k_fit_ell and k_stamp_metrics); the reciprocal,
// square-root, exp and log forms of the Levenberg-Marquardt iterations and their fp64 polish; and, as templates over
// the number of variables NP, the normal equations (FitNormEq), their Marquardt-scaled Cholesky factor, solve and
// inverse (fit_chol, fit_chol_solve, fit_lm_solve, fit_spd_inverse), the damping and the predicted decrease
// (FitDamping, fit_predicted_decrease), the trial point with the step limit on eta (fit_trial_point), the descent loop
// over a kernel's Model (fit_lm_descend: k_fit, k_fit_ell, k_fit_obs, k_fit_psf; k_fit_group keeps its own loop over
// its normal equations in LDS and shares the damping and the predicted decrease), the fp64 polish (fit_polish:
// k_fit_ell, k_fit_obs, k_fit_psf), the wave-uniform factors of a Moffat model pass (MoffatPar), the moment start
// (fit_moment_start), the derived values and error columns of the elliptical row layout (FitEllRow, fit_ell_errors:
// k_fit_ell, k_fit_obs) and the constants of the iteration.  Everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include "device_common.h"

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

// N wave-wide sums at once, each with the additions of wave_total -- the same operands in the same tree, so the same
// bits -- in 89 instructions for 21 sums where 21 wave_total take 147, and without their dependent chains.  After the first quad swap lanes i and i ^ 1 hold the same partial sum
// of a value; of two values, one lane of the pair keeps the first and the other the second (one select), and the next
// step runs on half as many registers.  The same at the second quad swap, the half-row mirror and the row mirror: value
// k of 16 ends up alone in one lane of every row of register k / 16.  Which lane keeps which value is chosen so that the
// mirrors, which reverse the order of the lanes they cross, bring together lanes holding the same value: with b0..b3
// the bits of the lane in its row, the steps keep the second value of a pair where b0 ^ b2, b1 ^ b2, b2 ^ b3, b3 is set.
// An odd value out is reduced in all lanes as in wave_total.  The rows hold different values now, which row_bcast15 /
// row_bcast31 (lane 15 or 31 only) cannot carry: the two row steps are v_permlane16_swap (odd rows of one register
// against the even rows of another -- two registers of 16 values fold into one) and v_permlane32_swap, each followed by
// the addition wave_total makes there, (s1 + s0) and (s3 + s2), then their sum.  One v_readlane per value.
template <int CTRL>
__device__ __forceinline__ int dpp_pull(int own) {       // the value of the lane CTRL names; the lane's own where there is none
    return __builtin_amdgcn_update_dpp(own, own, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_pull(float own) {
    return __builtin_bit_cast(float, dpp_pull<CTRL>(__builtin_bit_cast(int, own)));
}
template <int CTRL>
__device__ __forceinline__ double dpp_pull(double own) {
    const long long b = __builtin_bit_cast(long long, own);
    const unsigned lo = (unsigned)dpp_pull<CTRL>((int)(b & 0xffffffffll));
    const unsigned hi = (unsigned)dpp_pull<CTRL>((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
__device__ __forceinline__ float lane_pick(bool second, float a, float b) { return second ? b : a; }
__device__ __forceinline__ double lane_pick(bool second, double a, double b) { return second ? b : a; }
// (inline assembly: s_nop 1 is the two wait states a vector write of either operand needs before the swap reads it;
// with the builtins of these instructions hipcc of ROCm 7.2 used the first result in place of the second)
__device__ __forceinline__ void rows_swap16(unsigned& a, unsigned& b) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void rows_swap32(unsigned& a, unsigned& b) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
template <bool HALVES>
__device__ __forceinline__ void rows_swap(float& a, float& b) {
    unsigned x = __builtin_bit_cast(unsigned, a), y = __builtin_bit_cast(unsigned, b);
    if constexpr (HALVES) rows_swap32(x, y);
    else rows_swap16(x, y);
    a = __builtin_bit_cast(float, x);
    b = __builtin_bit_cast(float, y);
}
template <bool HALVES>
__device__ __forceinline__ void rows_swap(double& a, double& b) {
    const unsigned long long x = __builtin_bit_cast(unsigned long long, a), y = __builtin_bit_cast(unsigned long long, b);
    unsigned xl = (unsigned)x, xh = (unsigned)(x >> 32), yl = (unsigned)y, yh = (unsigned)(y >> 32);
    if constexpr (HALVES) { rows_swap32(xl, yl); rows_swap32(xh, yh); }
    else { rows_swap16(xl, yl); rows_swap16(xh, yh); }
    a = __builtin_bit_cast(double, ((unsigned long long)xh << 32) | xl);
    b = __builtin_bit_cast(double, ((unsigned long long)yh << 32) | yl);
}
template <int LANE>
__device__ __forceinline__ float lane_value(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), LANE));
}
template <int LANE>
__device__ __forceinline__ double lane_value(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), LANE);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), LANE);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
// one in-row step of wave_totals: n values in, (n + 1) / 2 out
template <int CTRL, int N, typename T>
__device__ __forceinline__ void wave_totals_step(const T (&in)[N], T (&out)[(N + 1) / 2], bool second) {
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const T a = in[2 * j] + dpp_term<CTRL, 0xf>(in[2 * j]);
        const T b = in[2 * j + 1] + dpp_term<CTRL, 0xf>(in[2 * j + 1]);
        out[j] = lane_pick(second, a, b);
    }
    if constexpr (N % 2 == 1) out[N / 2] = in[N - 1] + dpp_term<CTRL, 0xf>(in[N - 1]);
}
// the lane of a row in which value k of 16 ends up (see above)
__host__ __device__ constexpr int wave_totals_lane(int k) {
    const int b3 = (k >> 3) & 1, b2 = ((k >> 2) & 1) ^ b3, b1 = ((k >> 1) & 1) ^ b2, b0 = (k & 1) ^ b2;
    return b3 * 8 + b2 * 4 + b1 * 2 + b0;
}
template <int K, int N, typename T>
__device__ __forceinline__ void wave_totals_read(T (&v)[N], T r) {
    if constexpr (K < N) {
        v[K] = lane_value<(K >> 4) * 16 + wave_totals_lane(K & 15)>(r);
        if constexpr (((K + 1) & 15) != 0) wave_totals_read<K + 1, N, T>(v, r);
    }
}
// v[k] = wave_total(v[k]) for all k, `lane` the lane of the caller; all 64 lanes must be active
template <int N, typename T>
__device__ __forceinline__ void wave_totals(T (&v)[N], int lane) {
    static_assert(N >= 1 && N <= 32, "one or two registers of 16 values");
    constexpr int N1 = (N + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2;
    T s1[N1], s2[N2], s3[N3], s4[N4];
    const int b2 = (lane >> 2) & 1;
    wave_totals_step<0xB1>(v, s1, ((lane ^ b2) & 1) != 0);                 // quad_perm [1,0,3,2]
    wave_totals_step<0x4E>(s1, s2, (((lane >> 1) ^ b2) & 1) != 0);         // quad_perm [2,3,0,1]
    wave_totals_step<0x141>(s2, s3, (((lane >> 3) ^ b2) & 1) != 0);        // row_half_mirror
    wave_totals_step<0x140>(s3, s4, (lane & 8) != 0);                      // row_mirror
    static_assert(N4 == (N + 15) / 16, "16 values per register");
    T a = s4[0], b = s4[N4 - 1];
    rows_swap<false>(a, b);                // a: rows (a0, b0, a2, b2); b: (a1, b1, a3, b3)
    T p = b + a, q = p;                    // s1 + s0 and s3 + s2 of the first register in rows 0, 2, of the second in 1, 3
    rows_swap<true>(p, q);                 // p: the lower sums in both halves, q: the upper ones
    const T t = q + p;                     // (s3 + s2) + (s1 + s0): rows 0, 2 the first register's totals, rows 1, 3 the second's
    wave_totals_read<0, N, T>(v, t);
    if constexpr (N > 16) wave_totals_read<16, N, T>(v, t);
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

// ------------------------------------------------------------------------------------------
// The Levenberg-Marquardt core of the fits, over NP variables.
// ------------------------------------------------------------------------------------------

constexpr double kFitIllCond = 100.0;       // MPSFR_FIT_ILL_CONDITIONED, include/mpsfr.h
constexpr double kFitMaxE = 0.95;           // |e| bound of the step acceptance test of the elliptical models
#ifndef MPSFR_FIT_MAXIT
#define MPSFR_FIT_MAXIT 200
#endif
constexpr int kFitMaxIt = MPSFR_FIT_MAXIT;  // cap of the LM iterations
constexpr double kFitMu0 = 1.0e-2, kFitMuMax = 1.0e15;      // damping: start value, and where it gives up
// the polish of the weighted fits (k_fit_obs, k_fit_psf, k_fit_group): the cap of its steps, and the fraction of the
// formal error below which a step ends it
constexpr int kFitPolishMax = 12;
constexpr double kFitPolishSigma = 1.0e-6;

template <typename T, int NP>
struct FitNormEq {
    T a[NP * (NP + 1) / 2];   // upper triangle of J^T [W] J, row-major: (0,0)(0,1)..(0,NP-1)(1,1)..
    T g[NP];                  // J^T [W] r
    T chi2;
};

// index of the diagonal element (k, k) in the row-major upper triangle
template <int NP>
__host__ __device__ constexpr int fit_diag(int k) { return k * NP - k * (k - 1) / 2; }

// Cholesky factor of the Marquardt-scaled normal matrix  A'_ij = A_ij / (d_i d_j) + mu delta_ij,
// d_i = sqrt(A_ii) -- the same system as (A + mu diag A) x = -g, but with a unit diagonal, which
// is what lets the float phase factor it in float.  Fully unrolled: the factor lives in registers
// (dynamic indexing put it in scratch).  Li holds 1 / L_ii.  Returns false if not positive definite.
// ROW_FIRST: L_ji (j > i) is scaled as (a d_j^-1) d_i^-1 (k_fit) instead of (a d_i^-1) d_j^-1 (k_fit_ell, k_fit_obs).
template <int NP, typename S, typename T, bool ROW_FIRST = false>
__device__ __forceinline__ bool fit_chol(const FitNormEq<T, NP>& ne, S mu, S L[NP][NP], S Li[NP], S id[NP]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const S d = (S)ne.a[fit_diag<NP>(i)];
        ok = ok && (d > (S)0);
        id[i] = fit_rsqrt<S>(d);
    }
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i; j < NP; ++j) {
                L[j][i] = ROW_FIRST ? (S)ne.a[k] * id[j] * id[i] : (S)ne.a[k] * id[i] * id[j];
                ++k;
            }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        S s = (S)1 + mu;
#pragma unroll
        for (int q = 0; q < j; ++q) s -= L[j][q] * L[j][q];
        ok = ok && (s > (S)0);
        Li[j] = fit_rsqrt<S>(s);
        L[j][j] = s * Li[j];
#pragma unroll
        for (int i = j + 1; i < NP; ++i) {
            S t = L[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) t -= L[i][q] * L[j][q];
            L[i][j] = t * Li[j];
        }
    }
    return ok;
}

// x = A^-1 b through the factor of fit_chol (b and x in unscaled units)
template <int NP, typename S, typename X>
__device__ __forceinline__ void fit_chol_solve(const S L[NP][NP], const S Li[NP], const S id[NP], const S b[NP],
                                               X* x) {
    S y[NP], z[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        S t = b[i] * id[i];
#pragma unroll
        for (int q = 0; q < i; ++q) t -= L[i][q] * y[q];
        y[i] = t * Li[i];
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        S t = y[i];
#pragma unroll
        for (int q = i + 1; q < NP; ++q) t -= L[q][i] * z[q];
        z[i] = t * Li[i];
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) x[i] = (X)(z[i] * id[i]);
}

// solve (A + mu diag(A)) x = -g; S = arithmetic type of the factorisation
template <int NP, typename S, typename T, bool ROW_FIRST = false>
__device__ __forceinline__ bool fit_lm_solve(const FitNormEq<T, NP>& ne, S mu, S* x) {
    S L[NP][NP], Li[NP], id[NP], b[NP];
    if (!fit_chol<NP, S, T, ROW_FIRST>(ne, mu, L, Li, id)) return false;
#pragma unroll
    for (int i = 0; i < NP; ++i) b[i] = -(S)ne.g[i];
    fit_chol_solve<NP, S, S>(L, Li, id, b, x);
    return true;
}

// inverse of the symmetric normal matrix: one factorisation, NP back-substitutions; false if singular
// (in the arithmetic of the normal matrix: the error columns of the mixed mode of k_fit and k_fit_ell need no fp64)
template <int NP, typename T, bool ROW_FIRST = false>
__device__ __forceinline__ bool fit_spd_inverse(const FitNormEq<T, NP>& ne, double cov[NP][NP]) {
    T L[NP][NP], Li[NP], id[NP];
    if (!fit_chol<NP, T, T, ROW_FIRST>(ne, (T)0, L, Li, id)) return false;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        T b[NP];
        double x[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) b[k] = (k == c) ? (T)1 : (T)0;
        fit_chol_solve<NP, T, double>(L, Li, id, b, x);
#pragma unroll
        for (int k = 0; k < NP; ++k) cov[k][c] = x[k];
    }
    return true;
}

// One column of that inverse per lane: lane c < NP solves column c (x[k] = entry (k, c)) with the factor, which every
// lane computes from the wave-uniform normal matrix; the operations of a column are those of fit_spd_inverse.  Lanes
// from NP on solve for a zero right-hand side.  False, and x = 0, if singular.
template <int NP, typename T, bool ROW_FIRST = false>
__device__ __forceinline__ bool fit_spd_inverse_column(const FitNormEq<T, NP>& ne, int lane, double x[NP]) {
    T L[NP][NP], Li[NP], id[NP], b[NP];
    if (!fit_chol<NP, T, T, ROW_FIRST>(ne, (T)0, L, Li, id)) {
#pragma unroll
        for (int k = 0; k < NP; ++k) x[k] = 0.0;
        return false;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) b[k] = (k == lane) ? (T)1 : (T)0;
    fit_chol_solve<NP, T, double>(L, Li, id, b, x);
    return true;
}

// Nielsen's damping of the Marquardt-scaled system: a rejected step (or a matrix that is not positive definite)
// multiplies mu by nu = 2, 4, 8, ...; an accepted one of gain ratio rho scales it by max(1/3, 1 - (2 rho - 1)^3).
template <typename S>
struct FitDamping {
    S mu = (S)kFitMu0, nu = (S)2;
    __device__ __forceinline__ bool raise() {       // true: the damping ran out
        mu *= nu;
        nu *= (S)2;
        return mu > (S)kFitMuMax;
    }
    __device__ __forceinline__ void lower(S rho) {
        const S c = (S)2 * rho - (S)1;
        mu = fmax(mu * fmax((S)(1.0 / 3.0), (S)1 - c * c * c), (S)1.0e-14);
        nu = (S)2;
    }
};

// predicted decrease of chi2 by the step dx of the damped system: dx^T (mu D dx - g) (k_fit_group; fit_lm_descend
// holds the same sum written out)
template <int NP, typename S, typename T>
__device__ __forceinline__ S fit_predicted_decrease(const FitNormEq<T, NP>& ne, S mu, const S* dx) {
    S pred = (S)0;
#pragma unroll
    for (int k = 0; k < NP; ++k) pred += dx[k] * (mu * (S)ne.a[fit_diag<NP>(k)] * dx[k] - (S)ne.g[k]);
    return pred;
}

// The trial point vn = v + dx.  With IETA >= 0 the step limit of the Moffat fits on eta = v[IETA] comes first: a stamp
// narrower than the PSF core has no finite minimum in n, its valley runs to the Gaussian limit eta -> 0; a step may
// cut eta to a fifth at most (the whole step is scaled), so the valley is descended geometrically instead of through
// rejected steps.
// The rounding is spelled out, because the rows are held to their bits: every vn[k] is the rounded sum of v[k] and the
// rounded dx[k] -- except eta on a limited step, which is fma(sc, dx, v) with the dx before the scaling.  That is what
// the compiler made of `dx *= sc; vn = v + dx` while the loop was written out in each kernel (it moved the sum of eta,
// which the test of the limit needs, into the limiting branch and contracted it there); left to itself it contracts
// other sums as well once the code around them changes.
template <int NP, int IETA, typename S>
__device__ __forceinline__ void fit_trial_point(const S* v, S* dx, S* vn) {
#pragma clang fp contract(off)
    if constexpr (IETA >= 0) {
        S ve = v[IETA] + dx[IETA];
        if (ve < (S)0.2 * v[IETA]) {
            const S sc = (S)-0.8 * v[IETA] * fit_rcp<S>(dx[IETA]);
            ve = fma(sc, dx[IETA], v[IETA]);
#pragma unroll
            for (int k = 0; k < NP; ++k) dx[k] *= sc;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) vn[k] = k == IETA ? ve : v[k] + dx[k];
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) vn[k] = v[k] + dx[k];
    }
}

// The Levenberg-Marquardt descent from v, whose normal equations are ne, for at most maxit iterations (counted in
// `it`); returns the status: `status` if the iterations run out, 0 at a minimum, 2 if the matrix stays singular.
// Model is the kernel's:
//     NP, ROW_FIRST (fit_chol)           IETA: the index of eta, or -1             BOUNDED
//     accumulate(v, ne)                  step_size(dx, vn)                          inside(vn)
// IETA >= 0 (the Moffat fits): the step limit on eta, and the stop at eta < 1.5e-3 (n > 666: Gaussian to 1e-3).
// BOUNDED (k_fit_psf): when the damping runs out after a step the domain refused, the fit rests on the bound of the
// domain: not converged (1).  Otherwise a damping that runs out means no further descent: at the minimum.
// The state is wave-uniform (the totals of a model pass are), so the control flow is.
template <typename Model, typename S, typename RE>
__device__ __forceinline__ int fit_lm_descend(const Model& m, S tol, int maxit, int status, S (&v)[Model::NP],
                                              FitNormEq<RE, Model::NP>& ne, int& it) {
    constexpr int NP = Model::NP;
    FitDamping<S> damp;
    bool bound = false;              // the last step was refused by the domain
    while (it < maxit) {
        ++it;
        S dx[NP];
        if (!fit_lm_solve<NP, S, RE, Model::ROW_FIRST>(ne, damp.mu, dx)) {
            if (damp.raise()) { status = 2; break; }
            continue;
        }
        S vn[NP];
        fit_trial_point<NP, Model::IETA, S>(v, dx, vn);
        const S rel = m.step_size(dx, vn);
        const bool inside = m.inside(vn);
        if (inside && rel < tol) {       // converged: take the last (tiny) Gauss-Newton step
#pragma unroll
            for (int k = 0; k < NP; ++k) v[k] = vn[k];
            status = 0;
            break;
        }
        FitNormEq<RE, NP> nn;
        S rho = (S)-1;
        if (inside) {
            m.accumulate(vn, nn);
            // fit_predicted_decrease, written out: through the function the wave sums that end the trial pass above
            // were scheduled one after the other (100 to 260 s_nop more per iteration in k_fit_obs, none here)
            S pred = (S)0;
#pragma unroll
            for (int k = 0; k < NP; ++k) pred += dx[k] * (damp.mu * (S)ne.a[fit_diag<NP>(k)] * dx[k] - (S)ne.g[k]);
            rho = ((S)ne.chi2 - (S)nn.chi2) * fit_rcp<S>(pred);    // NaN -> rejected
        }
        if (rho > (S)0) {
#pragma unroll
            for (int k = 0; k < NP; ++k) v[k] = vn[k];
            ne = nn;
            bound = false;
            if constexpr (Model::IETA >= 0) {
                if (v[Model::IETA] < (S)1.5e-3) { status = 0; break; }
            }
            damp.lower(rho);
        } else {
            bound = !inside;
            if (damp.raise()) { status = (Model::BOUNDED && bound) ? 1 : 0; break; }
        }
    }
    return status;
}

// The fp64 polish of the mixed mode, from the float solution vd: steps -A^-1 g, g the gradient of the fp64 residuals
// (P::gradient), A the float normal matrix of the last iteration (nf.a; the fixed point is where g vanishes, whatever
// matrix the step is solved with).  A step that leaves the domain or is larger than 0.1 ends it untaken.  It ends after
// a step below end.rel, or, where end.sigma > 0, below that fraction of the formal error: dx^T A dx <= sigma^2 chi2 /
// dof.  Returns chi2 at the point before the last step when that step was below 1e-3 -- chi2 is stationary at the
// minimum, so it differs from the value at the new point in second order only -- and -1 otherwise.  COUNT: the steps
// count as iterations.  P is the kernel's: gradient(vd, g, &chi2), step_size(dx, vn), inside(vn).
struct FitPolishEnd {
    int maxsteps;
    double rel;                  // a step below this relative size ends the polish
    double sigma = 0.0, dof = 1.0;
};
template <int NP, bool COUNT, typename P>
__device__ __forceinline__ double fit_polish(const P& p, const FitPolishEnd& end, FitNormEq<double, NP>& nf,
                                             double (&vd)[NP], int status, int& it) {
    double chi2 = -1.0;
    nf.chi2 = -1.0;
    for (int pz = 0; pz < end.maxsteps && status != 2; ++pz) {
        p.gradient(vd, nf.g, &nf.chi2);
        double dx[NP], vn[NP];
        if (!fit_lm_solve<NP, double, double>(nf, 1.0e-10, dx)) break;
#pragma unroll
        for (int k = 0; k < NP; ++k) vn[k] = vd[k] + dx[k];
        const double rel = p.step_size(dx, vn);
        if (!p.inside(vn) || rel >= 0.1) break;
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < NP; ++k) d2 -= dx[k] * nf.g[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) vd[k] = vn[k];
        if constexpr (COUNT) ++it;
        chi2 = rel < 1.0e-3 ? nf.chi2 : -1.0;
        if (rel < end.rel || (end.sigma > 0.0 && d2 <= end.sigma * end.sigma * nf.chi2 / end.dof)) break;
    }
    return chi2;
}

// Wave-uniform factors of a model pass at v = (I, p0, q0, w, [e1, e2,] eta at ieta, ...).  With
// K = 1/a^2 = 4 (2^eta - 1) / w^2:  Q = A x^2 - 2 B x y + C y^2, A = gK (1 - e1), B = gK e2, C = gK (1 + e1),
// g = 1 / sqrt(1 - e1^2 - e2^2); the circular model has A = C = K, B = 0.
template <typename RE, bool ELL>
struct MoffatPar {
    RE I, p0, q0, n, gK, A, B, C, e1g2, e2g2, w2, nsq2, dKn;
    __device__ __forceinline__ MoffatPar(const RE* v, int ieta) {
        I = v[0]; p0 = v[1]; q0 = v[2];
        n = fit_rcp<RE>(v[ieta]);
        const RE s_ = fit_exp2m1<RE>(v[ieta]);                // 2^eta - 1
        const RE iw = fit_rcp<RE>(v[3]);
        const RE K = (RE)4 * s_ * iw * iw;
        if constexpr (ELL) {
            const RE e1 = v[4], e2 = v[5];
            const RE g2 = fit_rcp<RE>((RE)1 - e1 * e1 - e2 * e2);
            const RE g = fit_rsqrt<RE>((RE)1 - e1 * e1 - e2 * e2);
            gK = g * K;
            A = gK * ((RE)1 - e1); B = gK * e2; C = gK * ((RE)1 + e1);
            e1g2 = e1 * g2; e2g2 = e2 * g2;
        } else {
            gK = K; A = K; B = (RE)0; C = K; e1g2 = (RE)0; e2g2 = (RE)0;
        }
        w2 = (RE)2 * iw;
        nsq2 = n * n * (RE)0.69314718055994530942;          // n^2 ln2: the logarithm is to base 2
        dKn = (s_ + (RE)1) * (RE)0.69314718055994530942 * fit_rcp<RE>(s_);   // (dK/d eta) / K
    }
};

// Start values of eta and the FWHM from the moments ms1 = sum d, ms2 = sum d^2 of the stamp over the disc of radius
// rm + 1/2 around its brightest pixel `best` (the sums are the caller's).  For a Moffat sampled at its centre
//     S1 = I pi a^2 / (n - 1)  T1,        T1 = 1 - (1 + R^2/a^2)^(1 - n)
//     S2 = I^2 pi a^2 / (2n - 1) T2,      T2 = 1 - (1 + R^2/a^2)^(1 - 2n)
// so (S2/T2) / (I S1/T1) = (n - 1)/(2n - 1) gives n and then a; the truncation factors T1, T2 by fixed-point
// iteration from T = 1.  Returns false, and leaves the values alone, when the disc is too small (brightest pixel
// within six pixels of an edge) or the moments have no sign.
__device__ __forceinline__ bool fit_moment_start(float ms1, float ms2, float best, int rm, float* eta0, double* fw0) {
    const float bf = best, r2 = ((float)rm + 0.5f) * ((float)rm + 0.5f);      // (the caller's disc: one value)
    if (!(rm >= 6 && ms1 > 0.f && best > 0.f)) return false;
    float t1 = 1.f, t2 = 1.f, nn = 2.5f, a2 = 1.f;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        float rho = (ms2 * t1) * __builtin_amdgcn_rcpf(bf * ms1 * t2);
        rho = fminf(fmaxf(rho, 0.05f), 0.47f);
        nn = (1.f - rho) * __builtin_amdgcn_rcpf(1.f - 2.f * rho);
        nn = fminf(fmaxf(nn, 1.1f), 15.f);
        a2 = ms1 * (nn - 1.f) * __builtin_amdgcn_rcpf(t1 * bf * 3.14159265f);
        const float lx = __builtin_amdgcn_logf(1.f + r2 * __builtin_amdgcn_rcpf(a2));
        t1 = 1.f - __builtin_amdgcn_exp2f((1.f - nn) * lx);
        t2 = 1.f - __builtin_amdgcn_exp2f((1.f - 2.f * nn) * lx);
    }
    *eta0 = __builtin_amdgcn_rcpf(nn);
    const float w = 2.f * __builtin_amdgcn_sqrtf(a2 * (__builtin_amdgcn_exp2f(*eta0) - 1.f));
    if (w == w) *fw0 = fmin(fmax((double)w, 1.5), (double)NS);
    return true;
}


// The derived values of a row of the elliptical layout (k_fit_ell, k_fit_obs) at v = (I, p0, q0, w, [e1, e2,] eta at
// ieta, ...): n = 1/eta, alpha = w / (2 sqrt(2^eta - 1)); with e = |(e1, e2)| and f = ((1 + e)/(1 - e))^(1/4) the
// semi-axes are alpha f and alpha / f, the FWHMs w f and w / f, the major axis at rot = atan2(e2, e1) / 2 (degrees in
// [0, 180)); flux = I pi alpha^2 / (n - 1).  Without ELL: e = 0, f = 1, rot = 0.
template <bool ELL>
struct FitEllRow {
    double I, w, e1, e2, n, p2, s2, al, esq, e, f, rot, flux;
    __device__ __forceinline__ FitEllRow(const double* vd, int ieta) {
        I = vd[0]; w = vd[3];
        e1 = 0.0; e2 = 0.0;
        if constexpr (ELL) { e1 = vd[4]; e2 = vd[5]; }
        const double eta = vd[ieta];
        n = 1.0 / eta;
        p2 = exp2(eta); s2 = p2 - 1.0;
        const double sq = sqrt(s2);
        al = w / (2.0 * sq);
        esq = e1 * e1 + e2 * e2; e = sqrt(esq);
        f = ELL ? sqrt(sqrt((1.0 + e) / (1.0 - e))) : 1.0;
        rot = 0.0;
        if constexpr (ELL) {
            rot = 0.5 * atan2(e2, e1) * (180.0 / kPi);
            if (rot < 0.0) rot += 180.0;
            if (rot >= 180.0) rot -= 180.0;
        }
        flux = I * kPi * al * al / (n - 1.0);
    }
    // columns 3 .. 8 and 19; `up`: the amplitude scale of the row (a power of two)
    __device__ __forceinline__ void write(double* o, double up) const {
        o[3] = al * f; o[4] = al / f; o[5] = n; o[6] = rot;
        o[7] = w * f; o[8] = w / f;
        o[19] = flux * up;
    }
};

// The error columns of that layout from the covariance cov * s of the variables, propagated to first order: o[11 ..
// 17] the errors of I, p0, q0, the two FWHMs, rot (degrees; undetermined for e -> 0: capped at 180) and n, o[20] that
// of the flux; o[11] and o[20] times `up`, the amplitude scale of the row (a power of two).
template <int NP, int IETA, bool ELL>
__device__ __forceinline__ void fit_ell_errors(const FitEllRow<ELL>& r, const double (&cov)[NP][NP], double s,
                                               double up, double* o) {
    auto quad = [&](const double* gr) {       // s g^T cov g over the variables of gr (NP entries)
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = 0; j < NP; ++j) q += gr[i] * cov[i][j] * gr[j];
        return sqrt(fmax(q * s, 0.0));
    };
    o[11] = sqrt(fmax(cov[0][0] * s, 0.0)) * up;
    o[12] = sqrt(fmax(cov[1][1] * s, 0.0));
    o[13] = sqrt(fmax(cov[2][2] * s, 0.0));
    if constexpr (ELL) {
        const double ue1 = r.e > 0.0 ? r.e1 / r.e : 1.0, ue2 = r.e > 0.0 ? r.e2 / r.e : 0.0;
        const double h = 0.5 / (1.0 - r.esq);                  // d ln f / d e
        double gmaj[NP], gmin[NP], grot[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) { gmaj[k] = 0.0; gmin[k] = 0.0; grot[k] = 0.0; }
        gmaj[3] = r.f; gmaj[4] = r.w * r.f * h * ue1; gmaj[5] = r.w * r.f * h * ue2;
        gmin[3] = 1.0 / r.f; gmin[4] = -r.w / r.f * h * ue1; gmin[5] = -r.w / r.f * h * ue2;
        o[14] = quad(gmaj);
        o[15] = quad(gmin);
        // rot: d/de1 = -e2 / (2 e^2), d/de2 = e1 / (2 e^2)
        double erot = 180.0;
        if (r.esq > 0.0) {
            grot[4] = -0.5 * r.e2 / r.esq; grot[5] = 0.5 * r.e1 / r.esq;
            erot = fmin(quad(grot) * (180.0 / kPi), 180.0);
            if (!(erot == erot)) erot = 180.0;
        }
        o[16] = erot;
    } else {
        o[14] = sqrt(fmax(cov[3][3] * s, 0.0));
        o[15] = o[14];
        o[16] = 0.0;
    }
    o[17] = r.n * r.n * sqrt(fmax(cov[IETA][IETA] * s, 0.0));          // |dn/d eta| = n^2
    // flux = I pi w^2 / (4 (2^eta - 1) (n - 1))
    double gfl[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) gfl[k] = 0.0;
    gfl[0] = kPi * r.al * r.al / (r.n - 1.0);
    gfl[3] = 2.0 * r.flux / r.w;
    gfl[IETA] = r.flux * (r.n * r.n / (r.n - 1.0) - r.p2 * 0.69314718055994530942 / r.s2);
    o[20] = quad(gfl) * up;
}

// The shared intake of the weighted fits (all of it in k_fit_psf and k_fit_spec, the pixel rule,
// the argmax step and the weight in k_fit_obs and k_fit_group, which keep the rest written out for their speed): what
// a kernel does with a star between reading its pointers and its first model pass.  Everything here is exact whatever
// the order -- maxima, minima, integer counts, products by powers of two -- so a row does not depend on which kernel
// or which lane map took the star in.  A lane's pixels are o = lane + 64 m, m = 0 .. kFitPix - 1.
constexpr int kFitPix = NS * NS / 64;
static_assert(kFitPix * 64 == NS * NS, "the lane map assumes 1600 pixels");
constexpr double kFitMinWeight = 0x1p-100;   // a used pixel keeps a weight > 0 (relative to the largest one)

// The validity of a pixel.  used: the value is finite and, with a variance plane, the variance is finite and > 0;
// every other pixel carries weight 0 and data 0 from the load on, so its stored value reaches no sum.
struct FitPixel {
    bool used, bad;       // bad: an infinite value under a valid variance (the row gets status 2)
};
__device__ __forceinline__ FitPixel fit_pixel(double d, double v, bool has_var) {
    const bool vok = !has_var || (v > 0.0 && v < __builtin_inf());       // (NaN fails both)
    const bool fin = fabs(d) < __builtin_inf();
    FitPixel p;
    p.used = vok && fin;
    p.bad = vok && !fin && d == d;
    return p;
}

// First maximum (in C order, as np.argmax) of a value per lane and its offset, over the wave; every lane gets it.
// One step of the ladder (the tie rule, written once) and the ladder.
__device__ __forceinline__ void wave_first_max_step(double& best, int& besto, int o) {
    const double ob = __shfl_xor(best, o, 64);
    const int oo = __shfl_xor(besto, o, 64);
    if (ob > best || (ob == best && oo < besto)) { best = ob; besto = oo; }
}
__device__ __forceinline__ void wave_first_max(double& best, int& besto) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_first_max_step(best, besto, o);
}

// The first pass over a star (vsrc is read only with has_var): the brightest used pixel (ARGMAX: and its offset, the
// first in C order), the smallest valid variance, the largest used modulus, the used and the bad pixels.  add() takes
// one pixel and reduce_step() is one step of the ladder over the wave: a kernel with a model stamp takes star and stamp
// in one loop and one ladder (psf_scan, fit_psf_common.h: k_fit_psf, k_fit_spec).  k_fit_obs and k_fit_group keep
// their first pass written out, for their speed (fit_obs.hip, fit_group_impl.h).
template <bool ARGMAX>
struct FitStarScan {
    double best = -3.0e38, vmin = 3.0e38, amax = 0.0;
    int besto = 0, nused = 0, nbad = 0;
    __device__ __forceinline__ void add(int o, double d, double v, bool has_var) {
        const FitPixel px = fit_pixel(d, v, has_var);
        nused += px.used ? 1 : 0;
        nbad += px.bad ? 1 : 0;
        if (px.used) {
            vmin = fmin(vmin, v);
            amax = fmax(amax, fabs(d));
            if constexpr (ARGMAX) {
                if (d > best) { best = d; besto = o; }
            } else {
                best = fmax(best, d);
            }
        }
    }
    __device__ __forceinline__ void reduce_step(int o) {
        if constexpr (ARGMAX) wave_first_max_step(best, besto, o);
        else best = fmax(best, __shfl_xor(best, o, 64));
        vmin = fmin(vmin, __shfl_xor(vmin, o, 64));
        amax = fmax(amax, __shfl_xor(amax, o, 64));
        nused += __shfl_xor(nused, o, 64);
        nbad += __shfl_xor(nbad, o, 64);
    }
};

// The refusal rules of a star.  An amplitude (the brightest used pixel of a star, the brightest pixel of a model
// stamp, in modulus) must lie in [2^-40, 2^40]: zero and NaN fail.
__device__ __forceinline__ bool fit_amplitude_ok(double a) { return a >= 0x1p-40 && a <= 0x1p40; }
// the pixels: an infinite pixel, or too few used pixels for np variables
__device__ __forceinline__ bool fit_pixels_refused(int nused, int nbad, int np) { return nbad > 0 || nused < np + 1; }
// the range: the brightest used pixel outside the amplitude range, or a used pixel beyond 2^60 times the brightest
// one in modulus (a deep negative outlier: the float copy of the normalised star must hold it)
__device__ __forceinline__ bool fit_range_refused(double best, double amax) {
    const double ab = fabs(best);
    return !fit_amplitude_ok(ab) || amax > 0x1p60 * ab;
}
template <bool ARGMAX>
__device__ __forceinline__ bool fit_star_refused(const FitStarScan<ARGMAX>& s, int np) {
    return fit_pixels_refused(s.nused, s.nbad, np) || fit_range_refused(s.best, s.amax);
}

// the weight of a used pixel of variance v (1 without a variance plane), the largest one normalised by 2^kv
__device__ __forceinline__ double fit_weight(double v, int kv) { return fmax(1.0 / ldexp(v, -kv), kFitMinWeight); }

// The normalisation by powers of two, which is exact: the brightest used pixel into [1, 2) (data times 2^-kx), the
// largest weight into (1/2, 1] (weights 2^kv / var).  A constant factor 4^k on the variance plane or 2^k on the data
// therefore changes no bit of the normalised star.
struct FitNorm {
    int kx = 0, kv = 0;
    double scale = 1.0;                      // 2^-kx
    FitNorm() = default;
    __device__ __forceinline__ FitNorm(double best, double vmin, bool has_var)
        : kx(ilogb(fabs(best))), kv(has_var ? ilogb(vmin) : 0), scale(ldexp(1.0, -kx)) {}
    // normalised value and weight of pixel o (0, 0 if it is not used); returns whether it is used
    __device__ __forceinline__ bool pixel(const double* src, const double* vsrc, bool has_var, int o, double& dn,
                                          double& wn) const {
        const double d = src[o];
        const double v = has_var ? vsrc[o] : 1.0;
        const bool used = fit_pixel(d, v, has_var).used;
        dn = used ? d * scale : 0.0;
        wn = used ? fit_weight(v, kv) : 0.0;
        return used;
    }
};

}  // namespace
}  // namespace mpsfr
