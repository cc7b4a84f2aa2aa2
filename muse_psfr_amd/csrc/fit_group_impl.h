// HIP kernel of the simultaneous PSF-model fit of blended stars, written for gfx950 (MI355X, wave64).  See DESIGN.md
// section 19.  Included by fit_group.hip (mixed mode, 2 and 3 sources), fit_group_k4.hip (mixed mode, 4 sources) and
// fit_group_f64.hip (f64 mode), which instantiate launch_fit_group_mode for their share of the 36 variants so that the
// shares compile side by side.
//
// K_FIT_GROUP: per stamp the minimum of
//     sum_used w (m - d)^2,   w = 1 / var,   m(p, q) = sum_{k < K} F_k P~(p - dp_k, q - dq_k) + b
// with P~ the Keys resampling of the stamp's model P (fit_psf_common.h), in one of three sets of variables:
//     MODE 0, free:    F_k, dp_k, dq_k, [b]     NP = 3 K + [1]      v = (F_0, dp_0, dq_0, F_1, ..., [b])
//     MODE 1, common:  F_k, Dp, Dq, [b]         NP = K + 2 + [1]    v = (F_0 .. F_{K-1}, Dp, Dq, [b]); dp_k = s_k + Dp
//     MODE 2, fixed:   F_k, [b]                 NP = K + [1]        v = (F_0 .. F_{K-1}, [b]); linear, closed form
// The structure is k_fit_psf's: one wave per stamp, the star and its weights in LDS rows of 40, the apron model stamp
// in rows of 72, 25 pixels per lane in the 8 x 8-block map, wave-uniform tap weights (8 weights and 8 derivatives for
// each of the K sources), wave_total sums, the normal equations and their Cholesky solve and inverse of fit_common.h
// at NP up to 13, the same Marquardt scaling, Nielsen damping, step acceptance, fp64 polish and normalisations.
// All arrays are indexed with compile-time indices only, and no instantiation uses scratch: a pixel pass keeps its
// accumulators in registers (the 91 + 13 of the largest variant in one pass in float, in two passes of 46 + 13 and 45
// in fp64), and the finished sums live in LDS (sne), from where a solve loads what it needs.
#pragma once
#include <utility>

#include "device_common.h"
#include "fit_common.h"
#include "fit_psf_common.h"

namespace mpsfr {

namespace {

constexpr int kGroupMax = 4;                       // MPSFR_MAX_GROUP
constexpr int FLAG_COMMON_SHIFT = 8;               // MPSFR_FIT_COMMON_SHIFT
constexpr int GRP_FREE = 0, GRP_COMMON = 1, GRP_FIXED = 2;
static_assert(NFIT_GROUP == 8 + 8 * kGroupMax + 8, "head, one block of 8 per source, correlations");

template <int K, int MODE, bool BG>
struct GrpDim {
    static constexpr int NP = (MODE == GRP_FREE ? 3 * K : MODE == GRP_COMMON ? K + 2 : K) + (BG ? 1 : 0);
    static constexpr int NA = NP * (NP + 1) / 2;
    static constexpr int IB = NP - 1;                    // (only with BG)
    static constexpr int IC = K;                         // Dp, then Dq (only MODE 1)
    __host__ __device__ static constexpr int iF(int k) { return MODE == GRP_FREE ? 3 * k : k; }
};

// the tap weights of the K sources along one axis
template <typename RE, int K>
struct GrpTaps {
    KeysTaps<RE> t[K];
};
template <typename RE, int... I>
__device__ __forceinline__ GrpTaps<RE, (int)sizeof...(I)> grp_taps(const RE* d, std::integer_sequence<int, I...>) {
    return {{KeysTaps<RE>(d[I])...}};
}

// The state of a fit: the variables v and what the model needs of them -- F_k, the positions (py_k, px_k) and b.
// s0: the given positions (start values, catalogue positions or fixed positions).
template <int K, int MODE, bool BG, typename S>
struct GrpPoint {
    S F[K], py[K], px[K], bk;
    __device__ __forceinline__ GrpPoint(const S* v, const double* s0) {
        using D = GrpDim<K, MODE, BG>;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            F[k] = v[D::iF(k)];
            if constexpr (MODE == GRP_FREE) {
                py[k] = v[3 * k + 1];
                px[k] = v[3 * k + 2];
            } else if constexpr (MODE == GRP_COMMON) {
                py[k] = (S)s0[2 * k] + v[D::IC];
                px[k] = (S)s0[2 * k + 1] + v[D::IC + 1];
            } else {
                py[k] = (S)s0[2 * k];
                px[k] = (S)s0[2 * k + 1];
            }
        }
        bk = (S)0;
        if constexpr (BG) bk = v[D::IB];
    }
    __device__ __forceinline__ bool inside() const {        // every source inside the domain (NaN fails)
        bool in = true;
#pragma unroll
        for (int k = 0; k < K; ++k) in = in && psf_inside<S>(py[k], px[k]);
        return in;
    }
    __device__ __forceinline__ bool off_bound() const {     // no source rests on the bound
        bool in = true;
#pragma unroll
        for (int k = 0; k < K; ++k) in = in && fabs(py[k]) < (S)kPsfMaxShift && fabs(px[k]) < (S)kPsfMaxShift;
        return in;
    }
};

// the Jacobian row of one pixel from the K interpolated values and derivatives
template <int K, int MODE, bool BG, typename T>
__device__ __forceinline__ void grp_jacobian(const T* F, const T* val, const T* gy, const T* gx, T* J) {
    using D = GrpDim<K, MODE, BG>;
    if constexpr (MODE == GRP_COMMON) {
        J[D::IC] = (T)0;
        J[D::IC + 1] = (T)0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        J[D::iF(k)] = val[k];
        if constexpr (MODE == GRP_FREE) {
            J[3 * k + 1] = -F[k] * gy[k];
            J[3 * k + 2] = -F[k] * gx[k];
        } else if constexpr (MODE == GRP_COMMON) {
            J[D::IC] -= F[k] * gy[k];
            J[D::IC + 1] -= F[k] * gx[k];
        }
    }
    if constexpr (BG) J[D::IB] = (T)1;
}

// Weighted normal equations over the lane's 25 pixels, summed over the wave (psf_accumulate of fit_psf.hip with K
// FIRs per pixel), rows R0 .. R1 - 1 of the upper triangle.  pix / wt / pl: the star, its weights and the apron model
// stamp in LDS (LT); the arithmetic is RE.  The sums go to LDS -- out[0 .. NA) the upper triangle, out[NA .. NA + NP)
// the gradient, out[NA + NP] chi2 -- and are read from there when a solve needs them (grp_load): in fp64 the 104 sums of the largest variant, held in registers
// beside the 104 accumulators and 64 tap weights of the next pass or beside the 91 elements of a Cholesky factor,
// overflow the register file.
template <typename RE, typename LT, int K, int MODE, bool BG, int R0, int R1>
__device__ __forceinline__ void grp_accumulate_rows(const LT* pix, const LT* wt, const LT* pl, int lane,
                                                    const GrpPoint<K, MODE, BG, RE>& pt, const GrpTaps<RE, K>& ty,
                                                    const GrpTaps<RE, K>& tx, RE* out) {
    using D = GrpDim<K, MODE, BG>;
    constexpr int NP = D::NP, NA = D::NA;
    constexpr int A0 = fit_diag<NP>(R0), NR = (R1 < NP ? fit_diag<NP>(R1) : NA) - A0;   // rows R0 .. R1 - 1
    constexpr bool HEAD = R0 == 0;                   // the pass that also sums the gradient and chi2
    constexpr bool DERIV = MODE != GRP_FIXED;
    RE a[NR], g[NP], chi2 = (RE)0;
#pragma unroll
    for (int k = 0; k < NR; ++k) a[k] = (RE)0;
#pragma unroll
    for (int k = 0; k < NP; ++k) g[k] = (RE)0;
    const int lr = lane >> 3, lc = lane & 7;
    static_assert(NS == 40, "5 x 5 blocks of 8 x 8 pixels");
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll 1
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            RE val[K], gy[K], gx[K], m = (RE)0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const LdsStamp<LT> st(pl, ty.t[k].f, tx.t[k].f);
                psf_interp<RE, DERIV>(st, p * kPsfStride + q, p, q, ty.t[k], tx.t[k], val[k], gy[k], gx[k]);
                m += pt.F[k] * val[k];
            }
            const RE w = (RE)wt[o];
            RE J[NP];
            grp_jacobian<K, MODE, BG, RE>(pt.F, val, gy, gx, J);
            if constexpr (HEAD) {
                const RE r = (m + pt.bk) - (RE)pix[o];
                const RE wr = w * r;
                chi2 += wr * r;
#pragma unroll
                for (int i = 0; i < NP; ++i) g[i] += J[i] * wr;
            }
            int k = 0;
#pragma unroll
            for (int i = R0; i < R1; ++i) {
                const RE wj = w * J[i];
#pragma unroll
                for (int j = i; j < NP; ++j) a[k++] += wj * J[j];
            }
        }
    }
    // lane 0 stores the totals; every lane reads them back after the caller's barrier
    if constexpr (HEAD) {
        const RE c2 = wave_total(chi2);
        if (lane == 0) out[NA + NP] = c2;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const RE t = wave_total(g[k]);
            if (lane == 0) out[NA + k] = t;
        }
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const RE t = wave_total(a[k]);
        if (lane == 0) out[A0 + k] = t;
    }
}

template <typename RE, typename LT, int K, int MODE, bool BG>
__device__ __forceinline__ void grp_accumulate(const LT* pix, const LT* wt, const LT* pl, int lane,
                                               const GrpPoint<K, MODE, BG, RE>& pt, RE* out) {
    constexpr int NP = GrpDim<K, MODE, BG>::NP;
    const auto ty = grp_taps<RE>(pt.py, std::make_integer_sequence<int, K>());
    const auto tx = grp_taps<RE>(pt.px, std::make_integer_sequence<int, K>());
    if constexpr (sizeof(RE) == 8 && NP >= 12) {
        // fp64, four free sources: the 91 (78) sums of the triangle in two pixel passes, rows 0 .. 3 and the rest,
        // 46 + 45 (42 + 36) -- in one pass they overflow the register file beside the 64 fp64 tap weights
        grp_accumulate_rows<RE, LT, K, MODE, BG, 0, 4>(pix, wt, pl, lane, pt, ty, tx, out);
        grp_accumulate_rows<RE, LT, K, MODE, BG, 4, NP>(pix, wt, pl, lane, pt, ty, tx, out);
    } else {
        grp_accumulate_rows<RE, LT, K, MODE, BG, 0, NP>(pix, wt, pl, lane, pt, ty, tx, out);
    }
    __syncthreads();       // (one wave: it only orders the stores of lane 0 before the loads of every lane)
}

// the normal equations from LDS: a (converted to T), and with ALL also g and chi2
template <bool ALL, int NP, typename T, typename TI>
__device__ __forceinline__ void grp_load(const TI* in, FitNormEq<T, NP>& ne) {
    constexpr int NA = NP * (NP + 1) / 2;
#pragma unroll
    for (int k = 0; k < NA; ++k) ne.a[k] = (T)in[k];
    if constexpr (ALL) {
#pragma unroll
        for (int k = 0; k < NP; ++k) ne.g[k] = (T)in[NA + k];
        ne.chi2 = (T)in[NA + NP];
    }
}

// weighted chi2 alone
template <typename RE, int K, int MODE, bool BG>
__device__ __forceinline__ RE grp_chi2(const RE* pix, const RE* wt, const RE* pl, int lane,
                                       const GrpPoint<K, MODE, BG, RE>& pt) {
    const auto ty = grp_taps<RE>(pt.py, std::make_integer_sequence<int, K>());
    const auto tx = grp_taps<RE>(pt.px, std::make_integer_sequence<int, K>());
    RE cs = (RE)0;
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll 1
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            RE m = (RE)0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const LdsStamp<RE> st(pl, ty.t[k].f, tx.t[k].f);
                RE val, gy, gx;
                psf_interp<RE, false>(st, p * kPsfStride + q, p, q, ty.t[k], tx.t[k], val, gy, gx);
                m += pt.F[k] * val;
            }
            const RE r = (m + pt.bk) - pix[o];
            cs += wt[o] * r * r;
        }
    }
    return wave_total(cs);
}

// fp64-residual gradient J^T W r and chi2 for the polish of the mixed mode (psf_gradient of fit_psf.hip): the model
// from the fp64 model stamp in memory and the residual against the fp64 stamp in memory are formed in fp64; the
// weight and the Jacobian, which multiply a noise-sized residual, and the per-lane partial sums run in float.
template <int K, int MODE, bool BG>
__device__ __forceinline__ void grp_gradient(const double* __restrict__ src, double scale,
                                             const double* __restrict__ psrc, double pscale, const float* wt, int lane,
                                             const GrpPoint<K, MODE, BG, double>& pt, double* gout, double* chi2out) {
    using D = GrpDim<K, MODE, BG>;
    constexpr int NP = D::NP;
    constexpr bool DERIV = MODE != GRP_FIXED;
    const auto ty = grp_taps<double>(pt.py, std::make_integer_sequence<int, K>());
    const auto tx = grp_taps<double>(pt.px, std::make_integer_sequence<int, K>());
    float Ff[K];
#pragma unroll
    for (int k = 0; k < K; ++k) Ff[k] = (float)pt.F[k];
    float g[NP], c2sum = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) g[k] = 0.f;
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll 1
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            float val[K], gy[K], gx[K];
            double m = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const GlobalStamp st{psrc, pscale, ty.t[k].f, tx.t[k].f};
                double vd, gyd, gxd;
                psf_interp<double, DERIV>(st, 0, p, q, ty.t[k], tx.t[k], vd, gyd, gxd);
                m += pt.F[k] * vd;
                val[k] = (float)vd; gy[k] = (float)gyd; gx[k] = (float)gxd;
            }
            const float w = wt[o];
            const double dd = src[o];
            const float r = w > 0.f ? (float)((m + pt.bk) - dd * scale) : 0.f;
            const float wr = w * r;
            c2sum += wr * r;
            float J[NP];
            grp_jacobian<K, MODE, BG, float>(Ff, val, gy, gx, J);
#pragma unroll
            for (int i = 0; i < NP; ++i) g[i] += J[i] * wr;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) gout[k] = wave_total((double)g[k]);
    *chi2out = (double)wave_total(c2sum);
}

// size of a step dx towards vn: relative to max_k |F_k| for every F_k and for b, absolute (pixels) for positions
template <int K, int MODE, bool BG, typename S>
__device__ __forceinline__ S grp_step_size(const S* dx, const S* vn) {
    using D = GrpDim<K, MODE, BG>;
    S fm = (S)0, df = (S)0, rel = (S)0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        fm = fmax(fm, fabs(vn[D::iF(k)]));
        df = fmax(df, fabs(dx[D::iF(k)]));
        if constexpr (MODE == GRP_FREE) rel = fmax(rel, fmax(fabs(dx[3 * k + 1]), fabs(dx[3 * k + 2])));
    }
    if constexpr (MODE == GRP_COMMON) rel = fmax(fabs(dx[D::IC]), fabs(dx[D::IC + 1]));
    if constexpr (BG) df = fmax(df, fabs(dx[D::IB]));
    return fmax(rel, df * fit_rcp<S>(fm + (S)1.0e-30));
}

// The undamped solve of the start: fit_lm_solve at mu = 0, refused unless every pivot of the unit-diagonal matrix
// exceeds 64 eps.  Two sources at one position make two columns equal; the last pivot is then rounding noise of
// either sign, and a positive one would pass fit_chol's test.  (The pivots of the groups this fit is meant for are
// above 1 / 10: the linear problem in (F_k, b) is well conditioned whenever the sources are apart.)
template <int NP, typename S, typename T>
__device__ __forceinline__ bool grp_start_solve(const FitNormEq<T, NP>& ne, S* x) {
    S L[NP][NP], Li[NP], id[NP], b[NP];
    bool ok = fit_chol<NP, S, T>(ne, (S)0, L, Li, id);
    constexpr S kMinPivot = (S)64 * (sizeof(S) == 4 ? (S)1.1920929e-7 : (S)2.220446049250313e-16);
#pragma unroll
    for (int j = 0; j < NP; ++j) ok = ok && L[j][j] * L[j][j] > kMinPivot;
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < NP; ++i) b[i] = -(S)ne.g[i];
    fit_chol_solve<NP, S, S>(L, Li, id, b, x);
    return true;
}

// one wave per stamp; RE = float: mixed mode (float iterations + fp64 polish), RE = double: f64 mode
template <typename RE, int K, int MODE, bool BG>
__global__ void __launch_bounds__(64)
k_fit_group(int nstamp, const double* __restrict__ stamps, const double* __restrict__ var, int npsf,
            const double* __restrict__ psf, const int32_t* __restrict__ psf_index, const double* __restrict__ shift,
            double* __restrict__ fit) {
    using D = GrpDim<K, MODE, BG>;
    using DL = GrpDim<K, GRP_FIXED, BG>;            // the linear problem in (F_k, [b])
    constexpr int NP = D::NP, NA = D::NA, NPL = DL::NP;
    static_assert(K >= 2 && K <= kGroupMax, "2 to 4 sources");
    using S = RE;
    using Point = GrpPoint<K, MODE, BG, S>;
    const int lane = threadIdx.x & 63;
    const int st = (int)blockIdx.x;
    if (st >= nstamp) return;
    const double* src = stamps + (size_t)st * NS * NS;
    const bool has_var = var != nullptr;
    const double* vsrc = has_var ? var + (size_t)st * NS * NS : src;
    __shared__ RE sp[NS * NS];
    __shared__ RE sw[NS * NS];
    __shared__ RE pl[kPsfSide * kPsfStride];
    constexpr int NE = NA + NP + 1;                // the normal equations of a point: a, g, chi2
    __shared__ RE sne[2 * NE];                     // of the current point and of a trial point
    __shared__ double snf[sizeof(RE) == 4 ? NE : 1];       // mixed mode only: the fp64 normal matrix of the errors
    __shared__ double scov[NP * NP];               // the covariance, column by column
    double* orow = fit + (size_t)st * NFIT_GROUP;
    int nused = 0;
    auto refuse = [&]() {                   // a row that is not fitted: zeros, status 2, n_used, nsrc
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NFIT_GROUP; ++k) orow[k] = 0.0;
            orow[4] = 2.0;
            orow[5] = (double)nused;
            orow[6] = (double)K;
        }
    };
    // the model stamp of this group and the given positions (the device form has not seen either on the host)
    const int ip = psf_index ? psf_index[st] : st;
    double s0[2 * K];
    bool args_ok = ip >= 0 && ip < npsf;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s0[2 * k] = shift[(size_t)st * 2 * K + 2 * k];
        s0[2 * k + 1] = shift[(size_t)st * 2 * K + 2 * k + 1];
        args_ok = args_ok && psf_inside<double>(s0[2 * k], s0[2 * k + 1]);
    }
    const double* psrc = psf + (size_t)(args_ok ? ip : 0) * NS * NS;
    // The intake of this kernel is written out over the shared pixel rule and weight (fit_pixel, fit_weight): through
    // psf_scan, the shared refusal predicates, FitNorm and psf_stamp_load the rows were the same, but the compiler
    // allocated the registers of the whole kernel differently and k_fit_group<double, 4, 1, true> ran 0.5 % slower
    // (profiles/fit_intake_shared.md).  The rules are those of the shared intake.
    // First pass over the stamp: the brightest used pixel, the smallest valid variance, the number of used pixels;
    // over the model stamp: max |P|, its sum, whether it is finite
    double best = -3.0e38, vmin = 3.0e38, amax = 0.0, pamax = 0.0, psum = 0.0;
    int nbad = 0, pbad = 0;
#pragma unroll 5
    for (int m = 0; m < kFitPix; ++m) {
        const int o = lane + m * 64;
        const double d = src[o];
        const double v = has_var ? vsrc[o] : 1.0;
        const FitPixel px = fit_pixel(d, v, has_var);
        nused += px.used ? 1 : 0;
        nbad += px.bad ? 1 : 0;
        if (px.used) {
            vmin = fmin(vmin, v);
            amax = fmax(amax, fabs(d));
            best = fmax(best, d);
        }
        const double pv = psrc[o];
        pbad += fabs(pv) < __builtin_inf() ? 0 : 1;
        pamax = fmax(pamax, fabs(pv));
        psum += pv;
    }
    psum = wave_total(psum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        best = fmax(best, __shfl_xor(best, o, 64));
        vmin = fmin(vmin, __shfl_xor(vmin, o, 64));
        amax = fmax(amax, __shfl_xor(amax, o, 64));
        pamax = fmax(pamax, __shfl_xor(pamax, o, 64));
        nused += __shfl_xor(nused, o, 64);
        nbad += __shfl_xor(nbad, o, 64);
        pbad += __shfl_xor(pbad, o, 64);
    }
    // rows that are not fitted: the rules of k_fit_psf with NP the variables of the group (fit_star_refused and
    // PsfStampScan::refused, written out)
    const double ab = fabs(best);
    if (!args_ok || nbad > 0 || pbad > 0 || nused < NP + 1 || !(ab >= 0x1p-40 && ab <= 0x1p40) ||
        !(pamax >= 0x1p-40 && pamax <= 0x1p40) || amax > 0x1p60 * ab) {
        refuse();
        return;
    }
    // normalisation by powers of two: the brightest used pixel into [1, 2), the largest weight into (1/2, 1], the
    // brightest model pixel (in modulus) into [1, 2)
    const int kx = ilogb(ab);
    const double scale = ldexp(1.0, -kx);
    const int kv = has_var ? ilogb(vmin) : 0;
    const int kp = ilogb(pamax);
    const double pscale = ldexp(1.0, -kp);
    for (int o = lane; o < kPsfSide * kPsfStride; o += 64) pl[o] = (RE)0;
    __syncthreads();
#pragma unroll 5
    for (int m = 0; m < kFitPix; ++m) {
        const int o = lane + m * 64;
        const double d = src[o];
        const double v = has_var ? vsrc[o] : 1.0;
        const bool used = fit_pixel(d, v, has_var).used;
        sp[o] = (RE)(used ? d * scale : 0.0);
        sw[o] = (RE)(used ? fit_weight(v, kv) : 0.0);
        const int p = o / NS, q = o - p * NS;
        pl[(p + kPsfApron) * kPsfStride + q + kPsfApron] = (RE)(psrc[o] * pscale);
    }
    __syncthreads();                 // (one wave: the passes read pixels other lanes wrote)
    // Start values: the given positions (a common offset of 0); the F_k and b from the closed-form weighted linear
    // solve there, followed by one more solve from its solution (the rounding of the first one) -- in fixed mode that
    // is the whole fit.
    S v[NP];
    int it = 0, status = 1, cur = 0;        // sne + cur * NE: the normal equations at v
    {
        S vl[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) vl[k] = (S)0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            grp_accumulate<RE, RE, K, GRP_FIXED, BG>(sp, sw, pl, lane, GrpPoint<K, GRP_FIXED, BG, S>(vl, s0), sne);
            FitNormEq<RE, NPL> nl;
            grp_load<true>(sne, nl);
            S dl[NPL];
            if (!grp_start_solve<NPL, S, RE>(nl, dl)) {              // a singular normal matrix
                refuse();
                return;
            }
#pragma unroll
            for (int k = 0; k < NPL; ++k) vl[k] += dl[k];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) v[k] = (S)0;
#pragma unroll
        for (int k = 0; k < K; ++k) v[D::iF(k)] = vl[k];
        if constexpr (MODE == GRP_FREE) {
#pragma unroll
            for (int k = 0; k < K; ++k) { v[3 * k + 1] = (S)s0[2 * k]; v[3 * k + 2] = (S)s0[2 * k + 1]; }
        }
        if constexpr (BG) v[D::IB] = vl[DL::IB];
        if constexpr (MODE == GRP_FIXED) {       // (sne holds the normal matrix, which does not depend on v)
            it = 1;
            status = 0;
        }
    }
    if constexpr (MODE != GRP_FIXED) {
        grp_accumulate<RE, RE, K, MODE, BG>(sp, sw, pl, lane, Point(v, s0), sne);
        const S tol = sizeof(RE) == 4 ? (S)1.0e-3 : (S)1.0e-12;
        FitDamping<S> damp;
        bool bound = false;              // the last step was refused by the domain
        while (it < kFitMaxIt) {
            ++it;
            S dx[NP], pred, chi2_cur;
            {
                FitNormEq<RE, NP> ne;
                grp_load<true>(sne + cur * NE, ne);
                if (!fit_lm_solve<NP, S, RE>(ne, damp.mu, dx)) {
                    if (damp.raise()) { status = 2; break; }
                    continue;
                }
                pred = fit_predicted_decrease<NP, S, RE>(ne, damp.mu, dx);
                chi2_cur = (S)ne.chi2;
            }
            S vn[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) vn[k] = v[k] + dx[k];
            const S rel = grp_step_size<K, MODE, BG, S>(dx, vn);
            const Point pn(vn, s0);
            const bool inside = pn.inside();
            if (inside && rel < tol) {       // converged: take the last (tiny) Gauss-Newton step
#pragma unroll
                for (int k = 0; k < NP; ++k) v[k] = vn[k];
                status = 0;
                break;
            }
            S rho = (S)-1;
            if (inside) {
                RE* trial = sne + (cur ^ 1) * NE;
                grp_accumulate<RE, RE, K, MODE, BG>(sp, sw, pl, lane, pn, trial);
                rho = (chi2_cur - (S)trial[NA + NP]) * fit_rcp<S>(pred);    // NaN -> rejected
            }
            if (rho > (S)0) {
#pragma unroll
                for (int k = 0; k < NP; ++k) v[k] = vn[k];
                cur ^= 1;
                bound = false;
                damp.lower(rho);
            } else {
                bound = !inside;
                // no further descent: at the minimum, or against the bound of a position
                if (damp.raise()) { status = bound ? 1 : 0; break; }
            }
        }
        // a fit that rests on the bound of a position has not found a minimum
        if (status == 0 && !Point(v, s0).off_bound()) status = 1;
    }
    const double dof = (double)(nused - NP);
    double vd[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) vd[k] = (double)v[k];
    double chi2 = -1.0;
    const RE* sa = sne + cur * NE;           // the normal matrix of the last iteration
    const double* serr = nullptr;            // the fp64 normal matrix of the covariance
    if constexpr (sizeof(RE) == 4) {
        // the fp64 polish of k_fit_psf: steps -A^-1 g, g the gradient of the fp64 residuals, A the float normal matrix
        // of the last iteration; it ends once a step is below kFitPolishSigma of the formal error
        for (int pz = 0; pz <= kFitPolishMax && status != 2; ++pz) {
            FitNormEq<double, NP> nf;
            grp_gradient<K, MODE, BG>(src, scale, psrc, pscale, sw, lane, GrpPoint<K, MODE, BG, double>(vd, s0), nf.g,
                                      &nf.chi2);
            chi2 = nf.chi2;                  // the residuals at the current point
            if (pz == kFitPolishMax) break;
            grp_load<false>(sa, nf);
            double dx[NP], vn[NP];
            if (!fit_lm_solve<NP, double, double>(nf, 1.0e-10, dx)) break;
#pragma unroll
            for (int k = 0; k < NP; ++k) vn[k] = vd[k] + dx[k];
            const double rel = grp_step_size<K, MODE, BG, double>(dx, vn);
            if (!GrpPoint<K, MODE, BG, double>(vn, s0).inside() || rel >= 0.1) break;
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < NP; ++k) d2 -= dx[k] * nf.g[k];
#pragma unroll
            for (int k = 0; k < NP; ++k) vd[k] = vn[k];
            if constexpr (MODE != GRP_FIXED) ++it;
            // chi2 belongs to the point before this step: chi2 is stationary at the minimum, so after a step of `rel`
            // it differs from the value at the new point in second order only
            if (rel < 1.0e-3 && (rel < 1.0e-9 || d2 <= kFitPolishSigma * kFitPolishSigma * chi2 / dof)) break;
        }
        if (status != 2) {
            // one fp64 pass for the normal matrix of the errors (its gradient and chi2 are not used: they would come
            // from the float copies)
            grp_accumulate<double, float, K, MODE, BG>(sp, sw, pl, lane, GrpPoint<K, MODE, BG, double>(vd, s0), snf);
            serr = snf;
        }
    } else {
        chi2 = (double)grp_chi2<RE, K, MODE, BG>(sp, sw, pl, lane, Point(v, s0));
        serr = (const double*)sa;
    }
    if (lane != 0) return;
    // Outputs.  The amplitudes leave the normalisation: F_k and their errors by 2^(kx - kp), b and its error by 2^kx,
    // chi2 by 2^(2 kx - kv).  The covariance is the inverse of the normal matrix times chi2 / (n_used - NP), which no
    // scale of the weights changes.
    const GrpPoint<K, MODE, BG, double> pf(vd, s0);
    const double upf = ldexp(1.0, kx - kp), up = ldexp(1.0, kx);
    double* o = orow;
#pragma unroll
    for (int k = 0; k < NFIT_GROUP; ++k) o[k] = 0.0;
    if constexpr (BG) o[0] = pf.bk * up;
    o[2] = ldexp(chi2, 2 * kx - kv);
    o[3] = (double)it;
    o[5] = (double)nused;
    o[6] = (double)K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double* os = o + 8 + 8 * k;
        os[0] = pf.F[k] * upf;
        os[1] = pf.py[k];
        os[2] = pf.px[k];
        os[6] = os[0] * psum;
    }
    // the covariance: one factorisation, then column after column through LDS (fit_spd_inverse unrolls its NP
    // back-substitutions side by side, which at NP = 13 in fp64 overflows the register file)
    bool spd = false;
    if (status != 2) {
        FitNormEq<double, NP> nf;
        grp_load<false>(serr, nf);
        double L[NP][NP], Li[NP], id[NP];
        spd = fit_chol<NP, double, double>(nf, 0.0, L, Li, id);
#pragma unroll 1
        for (int c = 0; c < NP; ++c) {
            double b[NP], x[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) b[k] = (k == c) ? 1.0 : 0.0;
            fit_chol_solve<NP, double, double>(L, Li, id, b, x);
#pragma unroll
            for (int k = 0; k < NP; ++k) scov[c * NP + k] = x[k];
        }
    }
    auto cov = [&](int i, int j) { return scov[i * NP + j]; };
    if (spd) {
        const double s = chi2 / dof;
        if constexpr (BG) o[1] = sqrt(fmax(cov(D::IB, D::IB) * s, 0.0)) * up;
        double sf[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double* os = o + 8 + 8 * k;
            const double cff = cov(D::iF(k), D::iF(k));
            sf[k] = sqrt(fmax(cff, 0.0));
            os[3] = sqrt(fmax(cff * s, 0.0)) * upf;
            if constexpr (MODE == GRP_FREE) {
                os[4] = sqrt(fmax(cov(3 * k + 1, 3 * k + 1) * s, 0.0));
                os[5] = sqrt(fmax(cov(3 * k + 2, 3 * k + 2) * s, 0.0));
            } else if constexpr (MODE == GRP_COMMON) {
                os[4] = sqrt(fmax(cov(D::IC, D::IC) * s, 0.0));
                os[5] = sqrt(fmax(cov(D::IC + 1, D::IC + 1) * s, 0.0));
            }
            os[7] = os[3] * fabs(psum);
        }
        // the correlation coefficients of (F_i, F_j): (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = i + 1; j < K; ++j)
                o[40 + i * (7 - i) / 2 + (j - i - 1)] = cov(D::iF(i), D::iF(j)) / (sf[i] * sf[j]);
    } else {
        if (status == 0) status = 2;
    }
    // a row that claims a minimum holds finite numbers only; a row that is not fitted holds zeros
    bool finite = true;
#pragma unroll
    for (int k = 0; k < NFIT_GROUP; ++k) finite = finite && fabs(o[k]) < __builtin_inf();
    if (!finite && (status & 3) == 0) status = 2;
    if (status == 2) {
#pragma unroll
        for (int k = 0; k < NFIT_GROUP; ++k) o[k] = 0.0;
        o[5] = (double)nused;
        o[6] = (double)K;
    }
    o[4] = (double)status;
}

template <typename RE, int K, int MODE>
void launch_fit_group_bg(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                         const double* d_psf, const int32_t* d_index, const double* d_shift, bool bg, double* d_fit) {
    const dim3 grid(nstamp), block(64);
    if (bg)
        hipLaunchKernelGGL((k_fit_group<RE, K, MODE, true>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
    else
        hipLaunchKernelGGL((k_fit_group<RE, K, MODE, false>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
}

// grid(nstamp), block(64): one wavefront (and workgroup) per stamp, as launch_fit_psf
template <typename RE, int K>
void launch_fit_group_mode(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                           const double* d_psf, const int32_t* d_index, const double* d_shift, int flags,
                           double* d_fit) {
    const bool bg = (flags & FLAG_BACKGROUND) != 0;
    if (flags & FLAG_FIXED_SHIFT)
        launch_fit_group_bg<RE, K, GRP_FIXED>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, bg, d_fit);
    else if (flags & FLAG_COMMON_SHIFT)
        launch_fit_group_bg<RE, K, GRP_COMMON>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, bg, d_fit);
    else
        launch_fit_group_bg<RE, K, GRP_FREE>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, bg, d_fit);
}

}  // namespace

}  // namespace mpsfr
