// HIP kernel of the weighted Moffat fit of observed stars, written for gfx950 (MI355X, wave64).  See DESIGN.md
// section 17.
//
// K_FIT_OBS: mpdaf's Image.moffat_fit(weight=True, fit_back=..., circular=...) per stamp: the minimum of
//     sum_used w (model - data)^2,   w = 1 / var,   model = I (1 + Q)^-n + b
// with Q of fit_ell.hip (circular: e1 = e2 = 0 and no columns for them), over the USED pixels: data finite and,
// when a variance plane is given, variance finite and > 0.  Every other pixel carries weight 0 and data 0 from the
// load on, so its stored value reaches no sum.
// The structure is k_fit_ell's: one wave per stamp, 25 pixels per lane in the 8 x 8-block pixel map, wave-wide sums
// on the DPP path (wave_total), wave-uniform Levenberg-Marquardt state (Marquardt scaling, Nielsen's damping) in the
// variables (I, p0, q0, w, [e1, e2,] eta = 1/n, [b]): 5 to 8 of them, chosen at compile time.  The normal equations,
// their factorisation, solve and inverse, the model factors (MoffatPar) and the constants are fit_common.h's, shared
// by the fit kernels, as are the descent loop and the polish (fit_lm_descend, fit_polish over ObsModel) and the error
// columns of the row (fit_ell_errors).  New here: the weight
// plane beside the stamp in LDS, the start values from used pixels only, and the normalisation of data and weights by
// powers of two (brightest used pixel into [1, 2), largest weight into (1/2, 1]), which is exact and makes a constant
// factor on the variance plane change no bit of the parameters and errors.
// Mixed mode: float iterations, then the fp64-residual polish (float Jacobian, the float normal matrix of the last
// iteration) until the step is below 1e-6 of the formal error, then one fp64 normal matrix for the covariance.
// f64 mode: fp64 throughout, stamp and weights as doubles in LDS.
#include "device_common.h"
#include "fit_common.h"

namespace mpsfr {

namespace {

constexpr int FLAG_BACKGROUND = 1, FLAG_ELLIPTICAL = 2;      // MPSFR_FIT_BACKGROUND / MPSFR_FIT_ELLIPTICAL

// variables of a variant: I, p0, q0, w, [e1, e2,] eta, [b]
template <bool ELL, bool BG>
struct ObsDim {
    static constexpr int NP = 5 + (ELL ? 2 : 0) + (BG ? 1 : 0);
    static constexpr int NA = NP * (NP + 1) / 2;
    static constexpr int IETA = ELL ? 6 : 4;
    static constexpr int IB = IETA + 1;              // (only with BG)
};

// Weighted normal equations over the lane's 25 pixels, summed over the wave (every lane ends up with the totals).
// pix / wt: the stamp and its weights in LDS (LT), the arithmetic runs in RE.  Derivatives as in fit_ell.hip, with
// d/db = 1; c = n I (1+Q)^-n / (1 + Q) is taken from the Moffat term alone.
template <typename RE, typename LT, bool ELL, bool BG>
__device__ __forceinline__ void obs_accumulate(const LT* pix, const LT* wt, int lane, const RE* v,
                                               FitNormEq<RE, ObsDim<ELL, BG>::NP>& ne) {
    using D = ObsDim<ELL, BG>;
    constexpr int NP = D::NP, NA = D::NA;
    const MoffatPar<RE, ELL> P(v, D::IETA);
    RE bk = (RE)0;
    if constexpr (BG) bk = v[D::IB];
    RE a[NA], g[NP], chi2 = (RE)0;
#pragma unroll
    for (int k = 0; k < NA; ++k) a[k] = (RE)0;
#pragma unroll
    for (int k = 0; k < NP; ++k) g[k] = (RE)0;
    const RE lrf = (RE)(lane >> 3) - P.p0, lcf = (RE)(lane & 7) - P.q0;
    const int lo = (lane >> 3) * NS + (lane & 7);
    static_assert(NS == 40, "5 x 5 blocks of 8 x 8 pixels");
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const RE y = (RE)(8 * mo) + lrf;
        const RE yy = y * y;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const RE x = (RE)(8 * mi) + lcf;
            const RE xx = x * x;
            RE Q;
            if constexpr (ELL) Q = P.A * xx - (RE)2 * P.B * (x * y) + P.C * yy;
            else Q = P.A * (xx + yy);
            const RE gg = (RE)1 + Q;
            const RE lg2 = fit_log2<RE>(gg);
            const RE e = fit_exp2<RE>(-P.n * lg2);
            const RE m = P.I * e;
            const int o = lo + mo * 8 * NS + mi * 8;
            const RE w = (RE)wt[o];
            const RE r = (m + bk) - (RE)pix[o];
            const RE c = m * P.n * fit_rcp<RE>(gg);
            const RE c2 = (RE)2 * c;
            RE J[NP];
            J[0] = e;
            if constexpr (ELL) {
                const RE xy = x * y;
                J[1] = c2 * (P.C * y - P.B * x);
                J[2] = c2 * (P.A * x - P.B * y);
                J[4] = c * (P.gK * (xx - yy) - P.e1g2 * Q);
                J[5] = c * ((RE)2 * P.gK * xy - P.e2g2 * Q);
            } else {
                J[1] = c2 * P.A * y;
                J[2] = c2 * P.A * x;
            }
            J[3] = c * Q * P.w2;
            J[D::IETA] = m * (P.nsq2 * lg2) - c * Q * P.dKn;
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

// weighted chi2 alone at v (the residual pass without the Jacobian)
template <typename RE, bool ELL, bool BG>
__device__ __forceinline__ RE obs_chi2(const RE* pix, const RE* wt, int lane, const RE* v) {
    using D = ObsDim<ELL, BG>;
    const MoffatPar<RE, ELL> P(v, D::IETA);
    RE bk = (RE)0;
    if constexpr (BG) bk = v[D::IB];
    RE cs[5] = {(RE)0, (RE)0, (RE)0, (RE)0, (RE)0};
    const RE lrf = (RE)(lane >> 3) - P.p0, lcf = (RE)(lane & 7) - P.q0;
    const int lo = (lane >> 3) * NS + (lane & 7);
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const RE y = (RE)(8 * mo) + lrf;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const RE x = (RE)(8 * mi) + lcf;
            RE Q;
            if constexpr (ELL) Q = P.A * x * x - (RE)2 * P.B * x * y + P.C * y * y;
            else Q = P.A * (x * x + y * y);
            const int o = lo + mo * 8 * NS + mi * 8;
            const RE r = (P.I * fit_exp2<RE>(-P.n * fit_log2<RE>((RE)1 + Q)) + bk) - pix[o];
            cs[mi] += wt[o] * r * r;
        }
    }
    return wave_total(((cs[0] + cs[1]) + (cs[2] + cs[3])) + cs[4]);
}

// fp64-residual gradient J^T W r and chi2 for the polish of the mixed mode (ell_gradient of fit_ell.hip): the residual
// against the fp64 stamp in memory (times `scale`, the power of two of the normalisation) is formed in fp64; the
// Jacobian, the weight -- which multiply a noise-sized residual -- and the per-lane partial sums run in float.  A
// pixel of weight 0 is excluded: its stored value is never used.
template <bool ELL, bool BG>
__device__ __forceinline__ void obs_gradient(const double* __restrict__ src, double scale, const float* wt, int lane,
                                             const double* v, double* gout, double* chi2out) {
    using D = ObsDim<ELL, BG>;
    constexpr int NP = D::NP;
    const double eta = v[D::IETA];
    const double n = sgpr(1.0 / eta);
    const double s = lean_exp(0.69314718055994530942 * eta) - 1.0;
    const double K = 4.0 * s / (v[3] * v[3]);
    double e1 = 0.0, e2 = 0.0;
    if constexpr (ELL) { e1 = v[4]; e2 = v[5]; }
    const double q = 1.0 - e1 * e1 - e2 * e2;
    const double gK = sgpr(ELL ? K / sqrt(q) : K);
    const double A = sgpr(gK * (1.0 - e1)), B = sgpr(gK * e2), C = sgpr(gK * (1.0 + e1));
    const double I = sgpr(v[0]), p0 = sgpr(v[1]), q0 = sgpr(v[2]);
    double bk = 0.0;
    if constexpr (BG) bk = sgpr(v[D::IB]);
    const float nf = (float)n, nsq = (float)(n * n), dKn = (float)sgpr((s + 1.0) * 0.69314718055994530942 / s);
    const float w2 = (float)sgpr(2.0 / v[3]), gKf = (float)gK, Af = (float)A, Bf = (float)B, Cf = (float)C;
    const float e1g2 = (float)sgpr(e1 / q), e2g2 = (float)sgpr(e2 / q);
    float g[NP], c2sum = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) g[k] = 0.f;
    const double lrd = (double)(lane >> 3) - p0, lcd = (double)(lane & 7) - q0;
    const int lo = (lane >> 3) * NS + (lane & 7);
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const double y = (double)(8 * mo) + lrd;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const double x = (double)(8 * mi) + lcd;
            double Q;
            if constexpr (ELL) Q = fma(A * x, x, fma(C * y, y, -2.0 * B * x * y));
            else Q = A * fma(x, x, y * y);
            const double gg = 1.0 + Q;
            const double lg = lean_log(gg);
            const double e = lean_exp(-n * lg);
            const double m = I * e;
            const int o = lo + mo * 8 * NS + mi * 8;
            const float w = wt[o];
            const double dd = src[o];
            const float r = w > 0.f ? (float)((m + bk) - dd * scale) : 0.f;
            const float wr = w * r;
            c2sum += wr * r;
            const float xf = (float)x, yf = (float)y, Qf = (float)Q, mf = (float)m;
            const float c = mf * nf * __builtin_amdgcn_rcpf((float)gg);
            const float cr = c * wr;
            g[0] += (float)e * wr;
            if constexpr (ELL) {
                g[1] += 2.f * cr * (Cf * yf - Bf * xf);
                g[2] += 2.f * cr * (Af * xf - Bf * yf);
                g[4] += cr * (gKf * (xf * xf - yf * yf) - e1g2 * Qf);
                g[5] += cr * (2.f * gKf * xf * yf - e2g2 * Qf);
            } else {
                g[1] += 2.f * cr * Af * yf;
                g[2] += 2.f * cr * Af * xf;
            }
            g[3] += cr * Qf * w2;
            g[D::IETA] += (nsq * mf * (float)lg - c * Qf * dKn) * wr;
            if constexpr (BG) g[D::IB] += wr;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) gout[k] = wave_total((double)g[k]);
    *chi2out = (double)wave_total(c2sum);
}

// size of a step dx towards vn: relative for I, p0, q0, w, eta (k_fit's rule), absolute for e1, e2, and relative to
// the amplitude for the background (which may be zero)
template <bool ELL, bool BG, typename S>
__device__ __forceinline__ S obs_step_size(const S* dx, const S* vn) {
    using D = ObsDim<ELL, BG>;
    S rel = (S)0;
#pragma unroll
    for (int k = 0; k < D::NP; ++k) {
        S den = fabs(vn[k]) + (S)1.0e-30;
        if (ELL && (k == 4 || k == 5)) den = (S)1;
        if (BG && k == D::IB) den = fabs(vn[0]) + (S)1.0e-30;
        rel = fmax(rel, fabs(dx[k]) * fit_rcp<S>(den));
    }
    return rel;
}

template <bool ELL, bool BG, typename S>
__device__ __forceinline__ bool obs_inside(const S* vn) {
    using D = ObsDim<ELL, BG>;
    bool in = vn[3] > (S)1.0e-3 && vn[D::IETA] > (S)1.0e-3 && vn[D::IETA] < (S)1.0e2;
    if constexpr (ELL) in = in && vn[4] * vn[4] + vn[5] * vn[5] <= (S)(kFitMaxE * kFitMaxE);
    return in;
}

// what fit_lm_descend and fit_polish need of this fit (fit_common.h)
template <typename RE, bool ELL, bool BG>
struct ObsModel {
    using D = ObsDim<ELL, BG>;
    static constexpr int NP = D::NP, IETA = D::IETA;
    static constexpr bool ROW_FIRST = false, BOUNDED = false;
    const RE *sp, *sw;          // the stamp and its weights in LDS
    const double* src;          // the stamp in memory, and the power of two of its normalisation
    double scale;
    int lane;
    __device__ __forceinline__ void accumulate(const RE* v, FitNormEq<RE, NP>& ne) const {
        obs_accumulate<RE, RE, ELL, BG>(sp, sw, lane, v, ne);
    }
    __device__ __forceinline__ void gradient(const double* v, double* g, double* chi2) const {
        static_assert(sizeof(RE) == 4, "the fp64-residual gradient belongs to the mixed mode");
        obs_gradient<ELL, BG>(src, scale, sw, lane, v, g, chi2);
    }
    template <typename S>
    __device__ __forceinline__ S step_size(const S* dx, const S* vn) const { return obs_step_size<ELL, BG, S>(dx, vn); }
    template <typename S>
    __device__ __forceinline__ bool inside(const S* vn) const { return obs_inside<ELL, BG, S>(vn); }
};

// one wave per stamp; RE = float: mixed mode (float iterations + fp64 polish), RE = double: f64 mode
template <typename RE, bool ELL, bool BG>
__global__ void __launch_bounds__(64)
k_fit_obs(int nstamp, const double* __restrict__ stamps, const double* __restrict__ var, double* __restrict__ fit) {
    using D = ObsDim<ELL, BG>;
    constexpr int NP = D::NP, NA = D::NA;
    using S = RE;
    const int lane = threadIdx.x & 63;
    const int st = (int)blockIdx.x;
    if (st >= nstamp) return;
    const double* src = stamps + (size_t)st * NS * NS;
    const bool has_var = var != nullptr;
    const double* vsrc = has_var ? var + (size_t)st * NS * NS : src;
    __shared__ RE sp[NS * NS];
    __shared__ RE sw[NS * NS];
    // The intake of this kernel is written out, over the shared pixel rule, argmax step and weight (fit_pixel,
    // wave_first_max_step, fit_weight): through FitStarScan, the shared refusal predicates or FitNorm the compiler
    // allocates the registers of the whole kernel differently, and the elliptical instantiations with a background ran
    // 2 % slower (profiles/fit_intake_shared.md).  The rules are those of the shared intake.
    // First pass over the stamp: the brightest used pixel, the smallest valid variance, the number of used pixels.
    double best = -3.0e38, vmin = 3.0e38, amax = 0.0;
    int besto = 0, nused = 0, nbad = 0;
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
            if (d > best) { best = d; besto = o; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wave_first_max_step(best, besto, o);
        vmin = fmin(vmin, __shfl_xor(vmin, o, 64));
        amax = fmax(amax, __shfl_xor(amax, o, 64));
        nused += __shfl_xor(nused, o, 64);
        nbad += __shfl_xor(nbad, o, 64);
    }
    double* orow = fit + (size_t)st * NFIT_ELL;
    // rows that are not fitted: an infinite pixel, too few used pixels, a brightest used pixel outside [2^-40, 2^40],
    // a used pixel beyond 2^60 times the brightest one in modulus (fit_star_refused, written out)
    const double ab = fabs(best);
    if (nbad > 0 || nused < NP + 1 || !(ab >= 0x1p-40 && ab <= 0x1p40) || amax > 0x1p60 * ab) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NFIT_ELL; ++k) orow[k] = 0.0;
            orow[0] = (nused > 0 && ab <= 0x1p40) ? best : 0.0;
            orow[18] = 2.0;
            orow[23] = (double)nused;
        }
        return;
    }
    // normalisation by powers of two (FitNorm, written out): the brightest used pixel into [1, 2), the largest weight
    // into (1/2, 1]; the normalised stamp and its weights into LDS, and in the same pass the sums of the outer ring
    const int kx = ilogb(ab);
    const double scale = ldexp(1.0, -kx);
    const int kv = has_var ? ilogb(vmin) : 0;
    double ringsum = 0.0;
    int ringcnt = 0;
#pragma unroll 5
    for (int m = 0; m < kFitPix; ++m) {
        const int o = lane + m * 64;
        const double d = src[o];
        const double v = has_var ? vsrc[o] : 1.0;
        const bool used = fit_pixel(d, v, has_var).used;
        const double dn = used ? d * scale : 0.0;
        const double wn = used ? fit_weight(v, kv) : 0.0;
        sp[o] = (RE)dn;
        sw[o] = (RE)wn;
        if constexpr (BG) {
            const int p = o / NS, q = o - p * NS;
            const bool ring = used && (p == 0 || p == NS - 1 || q == 0 || q == NS - 1);
            ringsum += ring ? dn : 0.0;
            ringcnt += ring ? 1 : 0;
        }
    }
    __syncthreads();                 // (one wave: the passes read pixels other lanes wrote)
    // Start values, from used pixels only: the background is the mean of the used pixels of the outer ring, the
    // amplitude the brightest used pixel above it, the centre its position, the FWHM that of the disc whose area is
    // the number of used pixels above half maximum divided by the used fraction of the stamp; e = 0, n = 2.5.
    const double bestn = best * scale;
    double b0 = 0.0;
    if constexpr (BG) {
        ringsum = wave_total(ringsum);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ringcnt += __shfl_xor(ringcnt, o, 64);
        if (ringcnt > 0) b0 = ringsum / (double)ringcnt;
    }
    if (!(bestn > b0)) {             // no used pixel above the start background
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NFIT_ELL; ++k) orow[k] = 0.0;
            orow[0] = best;
            orow[18] = 2.0;
            orow[21] = BG ? b0 * ldexp(1.0, kx) : 0.0;
            orow[23] = (double)nused;
        }
        return;
    }
    int cnt = 0;
    {
        const RE half = (RE)(b0 + 0.5 * (bestn - b0));
        const int lo = (lane >> 3) * NS + (lane & 7);
#pragma unroll
        for (int mo = 0; mo < 5; ++mo)
#pragma unroll
            for (int mi = 0; mi < 5; ++mi) {
                const int o = lo + mo * 8 * NS + mi * 8;
                cnt += (sw[o] > (RE)0 && sp[o] > half) ? 1 : 0;
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    double fw0 = 2.0 * sqrt((double)cnt * (double)(NS * NS) / ((double)nused * kPi));
    fw0 = fmin(fmax(fw0, 1.5), (double)NS);
    S v[NP];
    v[0] = (S)(bestn - b0); v[1] = (S)(besto / NS); v[2] = (S)(besto % NS); v[3] = (S)fw0;
    if constexpr (ELL) { v[4] = (S)0; v[5] = (S)0; }
    v[D::IETA] = (S)0.4;
    if constexpr (BG) v[D::IB] = (S)b0;
    const S tol = sizeof(RE) == 4 ? (S)1.0e-3 : (S)1.0e-12;
    const ObsModel<RE, ELL, BG> model{sp, sw, src, scale, lane};
    FitNormEq<RE, NP> ne;
    model.accumulate(v, ne);
    int it = 0;
    int status = fit_lm_descend<ObsModel<RE, ELL, BG>, S, RE>(model, tol, kFitMaxIt, 1, v, ne, it);
    const double dof = (double)(nused - NP);
    double vd[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) vd[k] = (double)v[k];
    double chi2 = -1.0;
    // the normal matrix of the covariance, fp64; only nf.a is read after the fit (the f64 mode never writes nf.g and
    // nf.chi2, the mixed mode uses them inside its polish only)
    FitNormEq<double, NP> nf;
    if constexpr (sizeof(RE) == 4) {
        // the fp64 polish with the float normal matrix of the last iteration; it ends once a step is below
        // kFitPolishSigma of the formal error (or below 1e-9 relative on a stamp the model fits exactly)
#pragma unroll
        for (int k = 0; k < NA; ++k) nf.a[k] = (double)ne.a[k];
        chi2 = fit_polish<NP, true>(model, FitPolishEnd{kFitPolishMax, 1.0e-9, kFitPolishSigma, dof}, nf, vd, status, it);
        if (chi2 < 0.0) {              // the residuals at the final point
            double gtmp[NP];
            model.gradient(vd, gtmp, &chi2);
        }
        if (status != 2) {
            // one fp64 pass for the normal matrix of the errors (its gradient and chi2 are not used: they would come
            // from the float stamp)
            obs_accumulate<double, float, ELL, BG>(sp, sw, lane, vd, nf);
        }
    } else {
        chi2 = (double)obs_chi2<RE, ELL, BG>(sp, sw, lane, v);
#pragma unroll
        for (int k = 0; k < NA; ++k) nf.a[k] = (double)ne.a[k];
    }
    if (lane != 0) return;
    // Outputs, in the layout of k_fit_ell.  The amplitudes leave the normalisation: I, b and their errors by 2^kx,
    // chi2 by 2^(2 kx - kv).  The covariance is the inverse of the normal matrix times chi2 / (n_used - NP), which
    // no scale of the weights changes; the errors of derived values are propagated to first order.
    const double up = ldexp(1.0, kx);
    const FitEllRow<ELL> r(vd, D::IETA);
    double* o = orow;
    o[0] = r.I * up; o[1] = vd[1]; o[2] = vd[2];
    r.write(o, up);
    o[9] = ldexp(chi2, 2 * kx - kv);
    o[10] = (double)it;
    o[21] = 0.0; o[22] = 0.0;
    if constexpr (BG) o[21] = vd[D::IB] * up;
    o[23] = (double)nused;
    double cov[NP][NP];
    bool finite = true;
    if (status != 2 && fit_spd_inverse<NP, double>(nf, cov)) {
        const double s = chi2 / dof;
        fit_ell_errors<NP, D::IETA, ELL>(r, cov, s, up, o);
        if constexpr (BG) o[22] = sqrt(fmax(cov[D::IB][D::IB] * s, 0.0)) * up;
    } else {
        for (int k = 11; k <= 17; ++k) o[k] = 0.0;
        o[20] = 0.0;
        if (status == 0) status = 2;
    }
    // a row that claims a minimum holds finite numbers only
#pragma unroll
    for (int k = 0; k < NFIT_ELL; ++k)
        if (k != 18) finite = finite && fabs(o[k]) < __builtin_inf();
    if (!finite && (status & 3) == 0) status = 2;
    o[18] = (double)status;
}

template <typename RE>
void launch_fit_obs_variant(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int flags,
                            double* d_fit) {
    const dim3 grid(nstamp), block(64);
    switch (flags & (FLAG_BACKGROUND | FLAG_ELLIPTICAL)) {
    case 0:
        hipLaunchKernelGGL((k_fit_obs<RE, false, false>), grid, block, 0, s, nstamp, d_stamps, d_var, d_fit);
        break;
    case FLAG_BACKGROUND:
        hipLaunchKernelGGL((k_fit_obs<RE, false, true>), grid, block, 0, s, nstamp, d_stamps, d_var, d_fit);
        break;
    case FLAG_ELLIPTICAL:
        hipLaunchKernelGGL((k_fit_obs<RE, true, false>), grid, block, 0, s, nstamp, d_stamps, d_var, d_fit);
        break;
    default:
        hipLaunchKernelGGL((k_fit_obs<RE, true, true>), grid, block, 0, s, nstamp, d_stamps, d_var, d_fit);
        break;
    }
}

}  // namespace

void launch_fit_obs(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int flags, double* d_fit,
                    bool f64) {
    if (nstamp <= 0) return;
    // one wavefront (and workgroup) per stamp, as k_fit_ell
    if (f64) launch_fit_obs_variant<double>(s, nstamp, d_stamps, d_var, flags, d_fit);
    else launch_fit_obs_variant<float>(s, nstamp, d_stamps, d_var, flags, d_fit);
}

}  // namespace mpsfr
