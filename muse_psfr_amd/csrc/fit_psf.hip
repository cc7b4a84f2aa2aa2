// HIP kernel of the PSF-model fit of observed stars, written for gfx950 (MI355X, wave64).  See DESIGN.md section 18.
//
// K_FIT_PSF: per star the minimum of
//     sum_used w (m - d)^2,   w = 1 / var,   m(p, q) = F P~(p - dp, q - dq) + b
// over (F, [dp, dq,] [b]), where P~ is the model stamp P ([40][40], zero outside) resampled by cubic convolution
// (Keys, a = -1/2):  P~(y, x) = sum_kl c(y - k) c(x - l) P[k][l].  The fractional parts of (dp, dq) are the same for
// every pixel of a star, so the 4 + 4 tap weights and their derivatives are wave-uniform and a model pass is a 4 x 4
// FIR over the model stamp in LDS; d m / d dp = -F sum c'(y - k) c(x - l) P[k][l] comes from the same 16 taps.
// The structure is k_fit_obs's: one wave per star, 25 pixels per lane in the 8 x 8-block pixel map, wave-wide sums on
// the DPP path (wave_total), the shared Levenberg-Marquardt descent and polish (fit_lm_descend, fit_polish over PsfModel); the used
// pixels, the weight plane and the power-of-two normalisation of data and weights are the shared intake's
// (fit_common.h, fit_psf_common.h).  The normal equations, their factorisation, solve and inverse are fit_common.h's, for NP = 1 to 4.
// New here: the model stamp in LDS with a zero apron of 10 pixels (|dp|, |dq| <= 8 and taps -1 .. +2: no bounds test
// inside the domain), rows of 72 elements -- 72 = 8 mod 32, so the 4 rows x 8 columns of a 32-lane half fall on 32
// different banks (ds_read_b32; 16 bank pairs twice for ds_read_b64), as the 40-element rows of the star do; the model
// stamp normalised by a power of two (max |P| into [1, 2)); the start from the closed-form linear solve for (F, b).
// With the shift held fixed the problem is linear: that solve, and one more from its solution, are the whole fit.
// Mixed mode: float iterations, then the fp64-residual polish (model from the fp64 stamp in memory, the float normal
// matrix of the last iteration) until the step is below 1e-6 of the formal error, then one fp64 normal matrix for the
// covariance.  f64 mode: fp64 throughout, star, weights and model stamp as doubles in LDS (60 KB).
#include "device_common.h"
#include "fit_common.h"
#include "fit_psf_common.h"

namespace mpsfr {

namespace {

// variables of a variant: F, [dp, dq,] [b]
template <bool SHIFT, bool BG>
struct PsfDim {
    static constexpr int NP = 1 + (SHIFT ? 2 : 0) + (BG ? 1 : 0);
    static constexpr int NA = NP * (NP + 1) / 2;
    static constexpr int IB = SHIFT ? 3 : 1;             // (only with BG)
};

// Weighted normal equations over the lane's 25 pixels, summed over the wave (every lane ends up with the totals).
// pix / wt / pl: the star, its weights and the apron model stamp in LDS (LT), the arithmetic runs in RE; (dp, dq): the
// shift (v[1], v[2] of the caller when it is fitted).  J = (P~, -F dP~/dy, -F dP~/dx, 1).
template <typename RE, typename LT, bool SHIFT, bool BG>
__device__ __forceinline__ void psf_accumulate(const LT* pix, const LT* wt, const LT* pl, int lane, const RE* v, RE dp,
                                               RE dq, FitNormEq<RE, PsfDim<SHIFT, BG>::NP>& ne) {
    using D = PsfDim<SHIFT, BG>;
    constexpr int NP = D::NP, NA = D::NA;
    const KeysTaps<RE> ty(dp), tx(dq);
    const LdsStamp<LT> st(pl, ty.f, tx.f);
    const RE F = v[0];
    RE bk = (RE)0;
    if constexpr (BG) bk = v[D::IB];
    RE a[NA], g[NP], chi2 = (RE)0;
#pragma unroll
    for (int k = 0; k < NA; ++k) a[k] = (RE)0;
#pragma unroll
    for (int k = 0; k < NP; ++k) g[k] = (RE)0;
    const int lr = lane >> 3, lc = lane & 7;
    static_assert(NS == 40, "5 x 5 blocks of 8 x 8 pixels");
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            RE val, gy, gx;
            psf_interp<RE, SHIFT>(st, p * kPsfStride + q, p, q, ty, tx, val, gy, gx);
            const RE w = (RE)wt[o];
            const RE r = (F * val + bk) - (RE)pix[o];
            RE J[NP];
            J[0] = val;
            if constexpr (SHIFT) {
                J[1] = -F * gy;
                J[2] = -F * gx;
            }
            if constexpr (BG) J[D::IB] = (RE)1;
            const RE wr = w * r;
            chi2 += wr * r;
            int k = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                g[i] += J[i] * wr;
                const RE wj = w * J[i];
#pragma unroll
                for (int j = i; j < NP; ++j) a[k++] += wj * J[j];
            }
        }
    }
    ne.chi2 = wave_total(chi2);
#pragma unroll
    for (int k = 0; k < NA; ++k) ne.a[k] = wave_total(a[k]);
#pragma unroll
    for (int k = 0; k < NP; ++k) ne.g[k] = wave_total(g[k]);
}

// weighted chi2 alone at (F, dp, dq, b)
template <typename RE>
__device__ __forceinline__ RE psf_chi2(const RE* pix, const RE* wt, const RE* pl, int lane, RE F, RE dp, RE dq,
                                       RE bk) {
    const KeysTaps<RE> ty(dp), tx(dq);
    const LdsStamp<RE> st(pl, ty.f, tx.f);
    RE cs[5] = {(RE)0, (RE)0, (RE)0, (RE)0, (RE)0};
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            RE val, gy, gx;
            psf_interp<RE, false>(st, p * kPsfStride + q, p, q, ty, tx, val, gy, gx);
            const RE r = (F * val + bk) - pix[o];
            cs[mi] += wt[o] * r * r;
        }
    }
    return wave_total(((cs[0] + cs[1]) + (cs[2] + cs[3])) + cs[4]);
}

// fp64-residual gradient J^T W r and chi2 for the polish of the mixed mode (obs_gradient of fit_obs.hip): the model
// from the fp64 model stamp in memory and the residual against the fp64 star in memory (each times the power of two of
// its normalisation) are formed in fp64; the weight and the Jacobian, which multiply a noise-sized residual, and the
// per-lane partial sums run in float.  A pixel of weight 0 is excluded: its stored value is never used.
template <bool SHIFT, bool BG>
__device__ __forceinline__ void psf_gradient(const double* __restrict__ src, double scale,
                                             const double* __restrict__ psrc, double pscale, const float* wt, int lane,
                                             const double* v, double dp, double dq, double* gout, double* chi2out) {
    using D = PsfDim<SHIFT, BG>;
    constexpr int NP = D::NP;
    const KeysTaps<double> ty(dp), tx(dq);
    const GlobalStamp st{psrc, pscale, ty.f, tx.f};
    const double F = sgpr(v[0]);
    double bk = 0.0;
    if constexpr (BG) bk = sgpr(v[D::IB]);
    const float Ff = (float)F;
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
            double val, gy, gx;
            psf_interp<double, SHIFT>(st, 0, p, q, ty, tx, val, gy, gx);
            const float w = wt[o];
            const double dd = src[o];
            const float r = w > 0.f ? (float)((F * val + bk) - dd * scale) : 0.f;
            const float wr = w * r;
            c2sum += wr * r;
            g[0] += (float)val * wr;
            if constexpr (SHIFT) {
                g[1] -= Ff * (float)gy * wr;
                g[2] -= Ff * (float)gx * wr;
            }
            if constexpr (BG) g[D::IB] += wr;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) gout[k] = wave_total((double)g[k]);
    *chi2out = (double)wave_total(c2sum);
}

// size of a step dx towards vn: relative to the scale F for F and b, absolute (pixels) for the shift
template <bool SHIFT, bool BG, typename S>
__device__ __forceinline__ S psf_step_size(const S* dx, const S* vn) {
    using D = PsfDim<SHIFT, BG>;
    const S iden = fit_rcp<S>(fabs(vn[0]) + (S)1.0e-30);
    S rel = fabs(dx[0]) * iden;
    if constexpr (SHIFT) rel = fmax(rel, fmax(fabs(dx[1]), fabs(dx[2])));
    if constexpr (BG) rel = fmax(rel, fabs(dx[D::IB]) * iden);
    return rel;
}

// what fit_lm_descend and fit_polish need of this fit (fit_common.h); (dp0, dq0): the shift where it is held fixed
template <typename RE, bool SHIFT, bool BG>
struct PsfModel {
    using D = PsfDim<SHIFT, BG>;
    static constexpr int NP = D::NP, IETA = -1;
    static constexpr bool ROW_FIRST = false, BOUNDED = true;
    const RE *sp, *sw, *pl;     // the star, its weights and the apron model stamp in LDS
    const double *src, *psrc;   // the star and the model stamp in memory, and the powers of two of their normalisation
    double scale, pscale, dp0, dq0;
    int lane;
    __device__ __forceinline__ void accumulate(const RE* v, FitNormEq<RE, NP>& ne) const {
        if constexpr (SHIFT) psf_accumulate<RE, RE, true, BG>(sp, sw, pl, lane, v, v[1], v[2], ne);
        else psf_accumulate<RE, RE, false, BG>(sp, sw, pl, lane, v, (RE)dp0, (RE)dq0, ne);
    }
    __device__ __forceinline__ void gradient(const double* v, double* g, double* chi2) const {
        static_assert(sizeof(RE) == 4, "the fp64-residual gradient belongs to the mixed mode");
        psf_gradient<SHIFT, BG>(src, scale, psrc, pscale, sw, lane, v, SHIFT ? v[1] : dp0, SHIFT ? v[2] : dq0, g, chi2);
    }
    template <typename S>
    __device__ __forceinline__ S step_size(const S* dx, const S* vn) const { return psf_step_size<SHIFT, BG, S>(dx, vn); }
    template <typename S>
    __device__ __forceinline__ bool inside(const S* vn) const {
        if constexpr (SHIFT) return psf_inside<S>(vn[1], vn[2]);
        else return true;
    }
};

// one wave per star; RE = float: mixed mode (float iterations + fp64 polish), RE = double: f64 mode
template <typename RE, bool SHIFT, bool BG>
__global__ void __launch_bounds__(64)
k_fit_psf(int nstamp, const double* __restrict__ stamps, const double* __restrict__ var, int npsf,
          const double* __restrict__ psf, const int32_t* __restrict__ psf_index, const double* __restrict__ shift,
          double* __restrict__ fit) {
    using D = PsfDim<SHIFT, BG>;
    using DL = PsfDim<false, BG>;                  // the linear problem in (F, [b])
    constexpr int NP = D::NP, NA = D::NA, NPL = DL::NP;
    using S = RE;
    const int lane = threadIdx.x & 63;
    const int st = (int)blockIdx.x;
    if (st >= nstamp) return;
    const double* src = stamps + (size_t)st * NS * NS;
    const bool has_var = var != nullptr;
    const double* vsrc = has_var ? var + (size_t)st * NS * NS : src;
    __shared__ RE sp[NS * NS];
    __shared__ RE sw[NS * NS];
    __shared__ RE pl[kPsfSide * kPsfStride];
    double* orow = fit + (size_t)st * NFIT_PSF;
    FitStarScan<true> star;
    auto refuse = [&]() {                   // a row that is not fitted: zeros, status 2, the number of used pixels
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NFIT_PSF; ++k) orow[k] = 0.0;
            orow[10] = 2.0;
            orow[11] = (double)star.nused;
        }
    };
    // the model stamp of this star and the given shift (the device form has not seen either on the host)
    const int ip = psf_index ? psf_index[st] : st;
    double dp0 = 0.0, dq0 = 0.0;
    if (shift) { dp0 = shift[2 * (size_t)st]; dq0 = shift[2 * (size_t)st + 1]; }
    const bool args_ok = ip >= 0 && ip < npsf && psf_inside<double>(dp0, dq0);
    const double* psrc = psf + (size_t)(args_ok ? ip : 0) * NS * NS;
    // first pass over the star and over the model stamp (the shared intake)
    PsfStampScan<true> mod;
    psf_scan(star, mod, src, vsrc, has_var, psrc, lane);
    // rows that are not fitted: a model index or a given shift outside its range, and the rules of the intake for the
    // star and for the model stamp
    if (!args_ok || fit_star_refused(star, NP) || mod.refused()) {
        refuse();
        return;
    }
    const FitNorm norm(star.best, star.vmin, has_var);
    const double scale = norm.scale;
    const int kx = norm.kx, kv = norm.kv, nused = star.nused, besto = star.besto, pbesto = mod.pbesto;
    const int kp = ilogb(mod.pamax);
    const double pscale = ldexp(1.0, -kp);
    psf_stamp_clear(pl, lane);
    __syncthreads();
    const PsfStarPlanes<RE> planes{norm, src, vsrc, has_var, sp, sw};
    const double psum = wave_total(psf_stamp_load(psrc, kp, pl, lane, planes));
    __syncthreads();                 // (one wave: the passes read pixels other lanes wrote)
    // Start values: the given shift, or the brightest used pixel of the star minus the first maximum of the model
    // stamp, brought into the domain; F and b from the closed-form weighted linear solve at that shift.
    if (!shift) {
        dp0 = fmin(fmax((double)(besto / NS - pbesto / NS), -kPsfMaxShift), kPsfMaxShift);
        dq0 = fmin(fmax((double)(besto % NS - pbesto % NS), -kPsfMaxShift), kPsfMaxShift);
    }
    S v[NP];
    {
        S vl[NPL], dl[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) vl[k] = (S)0;
        FitNormEq<RE, NPL> nl;
        psf_accumulate<RE, RE, false, BG>(sp, sw, pl, lane, vl, (RE)dp0, (RE)dq0, nl);
        if (!fit_lm_solve<NPL, S, RE>(nl, (S)0, dl)) {           // a singular normal matrix
            refuse();
            return;
        }
        v[0] = dl[0];
        if constexpr (SHIFT) { v[1] = (S)dp0; v[2] = (S)dq0; }
        if constexpr (BG) v[D::IB] = dl[DL::IB];
    }
    const PsfModel<RE, SHIFT, BG> model{sp, sw, pl, src, psrc, scale, pscale, dp0, dq0, lane};
    FitNormEq<RE, NP> ne;
    int it = 0, status = 1;
    if constexpr (!SHIFT) {
        // the linear problem: one more solve from the solution (the rounding of the first one); the normal matrix
        // does not depend on the variables
        model.accumulate(v, ne);
        S dx[NP];
        if (fit_lm_solve<NP, S, RE>(ne, (S)0, dx)) {
#pragma unroll
            for (int k = 0; k < NP; ++k) v[k] += dx[k];
            status = 0;
        } else {
            status = 2;
        }
        it = 1;
    } else {
        model.accumulate(v, ne);
        const S tol = sizeof(RE) == 4 ? (S)1.0e-3 : (S)1.0e-12;
        status = fit_lm_descend<PsfModel<RE, SHIFT, BG>, S, RE>(model, tol, kFitMaxIt, 1, v, ne, it);
        // a fit that rests on the bound of the shift has not found a minimum (a damped step too small to leave the
        // bound in this arithmetic passes the convergence test)
        if (status == 0 && !(fabs(v[1]) < (S)kPsfMaxShift && fabs(v[2]) < (S)kPsfMaxShift)) status = 1;
    }
    const double dof = (double)(nused - NP);
    double vd[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) vd[k] = (double)v[k];
    double dpf = dp0, dqf = dq0;       // the shift of the model: the fitted one, or the fixed one
    if constexpr (SHIFT) { dpf = vd[1]; dqf = vd[2]; }
    double chi2 = -1.0;
    // the normal matrix of the covariance, fp64; only nf.a is read after the fit
    FitNormEq<double, NP> nf;
    if constexpr (sizeof(RE) == 4) {
        // the fp64 polish with the float normal matrix of the last iteration; it ends once a step is below
        // kFitPolishSigma of the formal error (or below 1e-9 on a star the model fits exactly)
#pragma unroll
        for (int k = 0; k < NA; ++k) nf.a[k] = (double)ne.a[k];
        chi2 = fit_polish<NP, SHIFT>(model, FitPolishEnd{kFitPolishMax, 1.0e-9, kFitPolishSigma, dof}, nf, vd, status, it);
        if constexpr (SHIFT) { dpf = vd[1]; dqf = vd[2]; }
        if (chi2 < 0.0) {              // the residuals at the final point
            double gtmp[NP];
            model.gradient(vd, gtmp, &chi2);
        }
        if (status != 2) {
            // one fp64 pass for the normal matrix of the errors (its gradient and chi2 are not used: they would come
            // from the float copies)
            psf_accumulate<double, float, SHIFT, BG>(sp, sw, pl, lane, vd, dpf, dqf, nf);
        }
    } else {
        RE bk = (RE)0;
        if constexpr (BG) bk = v[D::IB];
        chi2 = (double)psf_chi2<RE>(sp, sw, pl, lane, v[0], (RE)dpf, (RE)dqf, bk);
#pragma unroll
        for (int k = 0; k < NA; ++k) nf.a[k] = (double)ne.a[k];
    }
    if (lane != 0) return;
    // Outputs.  The amplitudes leave the normalisation: F and its error by 2^(kx - kp), b and its error by 2^kx, chi2
    // by 2^(2 kx - kv).  The covariance is the inverse of the normal matrix times chi2 / (n_used - NP), which no scale
    // of the weights changes.
    const double upf = ldexp(1.0, kx - kp), up = ldexp(1.0, kx);
    double* o = orow;
#pragma unroll
    for (int k = 0; k < NFIT_PSF; ++k) o[k] = 0.0;
    o[0] = vd[0] * upf;
    o[1] = dpf;
    o[2] = dqf;
    if constexpr (BG) o[3] = vd[D::IB] * up;
    o[4] = ldexp(chi2, 2 * kx - kv);
    o[5] = (double)it;
    o[11] = (double)nused;
    o[12] = o[0] * psum;
    double cov[NP][NP];
    if (status != 2 && fit_spd_inverse<NP, double>(nf, cov)) {
        const double s = chi2 / dof;
        o[6] = sqrt(fmax(cov[0][0] * s, 0.0)) * upf;
        if constexpr (SHIFT) {
            o[7] = sqrt(fmax(cov[1][1] * s, 0.0));
            o[8] = sqrt(fmax(cov[2][2] * s, 0.0));
        }
        if constexpr (BG) o[9] = sqrt(fmax(cov[D::IB][D::IB] * s, 0.0)) * up;
        o[13] = o[6] * fabs(psum);
    } else {
        if (status == 0) status = 2;
    }
    // a row that claims a minimum holds finite numbers only
    bool finite = true;
#pragma unroll
    for (int k = 0; k < NFIT_PSF; ++k) finite = finite && fabs(o[k]) < __builtin_inf();
    if (!finite && (status & 3) == 0) status = 2;
    o[10] = (double)status;
}

template <typename RE>
void launch_fit_psf_variant(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                            const double* d_psf, const int32_t* d_index, const double* d_shift, int flags,
                            double* d_fit) {
    const dim3 grid(nstamp), block(64);
    switch (flags & (FLAG_BACKGROUND | FLAG_FIXED_SHIFT)) {
    case 0:
        hipLaunchKernelGGL((k_fit_psf<RE, true, false>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
        break;
    case FLAG_BACKGROUND:
        hipLaunchKernelGGL((k_fit_psf<RE, true, true>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
        break;
    case FLAG_FIXED_SHIFT:
        hipLaunchKernelGGL((k_fit_psf<RE, false, false>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
        break;
    default:
        hipLaunchKernelGGL((k_fit_psf<RE, false, true>), grid, block, 0, s, nstamp, d_stamps, d_var, npsf, d_psf,
                           d_index, d_shift, d_fit);
        break;
    }
}

}  // namespace

void launch_fit_psf(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                    const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit,
                    bool f64) {
    if (nstamp <= 0) return;
    // one wavefront (and workgroup) per star, as k_fit_obs
    if (f64) launch_fit_psf_variant<double>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
    else launch_fit_psf_variant<float>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
}

}  // namespace mpsfr
