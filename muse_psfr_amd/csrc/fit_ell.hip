// HIP kernel of the elliptical Moffat fit, written for gfx950 (MI355X, wave64).  See DESIGN.md section 13.
//
// K_FIT (elliptical): 7-parameter Moffat least-squares fit per stamp -- mpdaf's Image.moffat_fit(circular=False,
// fit_back=False), which the reference does not call (fit_psf_cube, psfrec.py:861-871, fits circularly):
//     I (1 + Q)^-n,   Q = (g / a^2) [ (1 - e1) x^2 - 2 e2 x y + (1 + e1) y^2 ],   g = 1 / sqrt(1 - e1^2 - e2^2)
// with x = q - q0 (column), y = p - p0 (row); a is the geometric mean of the semi-axes (the quadratic form has
// determinant 1 / a^4).  (e1, e2) is smooth through the round case e = 0, where an (a, b, theta) parametrisation
// has a singular normal matrix, and at e1 = e2 = 0 the model is k_fit's (stamps.hip).
// The structure is k_fit's: one wave per stamp with the stamp in LDS, wave-wide sums on the DPP path, wave-uniform
// Levenberg-Marquardt state (Marquardt scaling, Nielsen's damping update) in the variables
// (I, p0, q0, w = geometric-mean FWHM, e1, e2, eta = 1/n).  The normal equations, their factorisation, solve and
// inverse, the descent loop and the polish (fit_lm_descend, fit_polish over EllModel), the model factors (MoffatPar),
// the moment start, the error columns of the row (fit_ell_errors) and the constants are fit_common.h's, shared by the
// fit kernels.  Mixed mode: float iterations, then the fp64 gradient
// polish with the last normal matrix; f64 mode: fp64 iterations throughout.
#include "device_common.h"
#include "fit_common.h"

namespace mpsfr {

namespace {

constexpr int NPE = 7;                       // LM variables
constexpr int NAE = NPE * (NPE + 1) / 2;     // upper triangle of the normal matrix
constexpr int kEllPolishMax = 8;

// Normal equations of the elliptical model over the lane's 25 pixels, summed over the wave (every lane ends up
// with the totals).  Pixel map of k_fit's passes: the lane is a cell (lr, lc) of an 8 x 8 block and the 25 blocks
// of the stamp are walked as 5 x 5, pixel (8 mo + lr, 8 mi + lc).  With c = n model / (1 + Q):
//   d/dI = (1+Q)^-n            d/dp0 = 2c (C y - B x)         d/dq0 = 2c (A x - B y)         d/dw = 2c Q / w
//   d/de1 = c (gK (x^2 - y^2) - e1 g^2 Q)      d/de2 = c (2 gK x y - e2 g^2 Q)
//   d/deta = model n^2 ln(1+Q) - c Q (dK/deta)/K
template <typename RE>
__device__ __forceinline__ void ell_accumulate(const RE* pix, int lane, const RE* v, FitNormEq<RE, NPE>& ne) {
    const MoffatPar<RE, true> P(v, 6);
    RE a[NAE], g[NPE], chi2 = (RE)0;
#pragma unroll
    for (int k = 0; k < NAE; ++k) a[k] = (RE)0;
#pragma unroll
    for (int k = 0; k < NPE; ++k) g[k] = (RE)0;
    const RE lrf = (RE)(lane >> 3) - P.p0, lcf = (RE)(lane & 7) - P.q0;
    const RE* pl = pix + (lane >> 3) * NS + (lane & 7);
    static_assert(NS == 40, "5 x 5 blocks of 8 x 8 pixels");
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const RE y = (RE)(8 * mo) + lrf;
        const RE yy = y * y;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const RE x = (RE)(8 * mi) + lcf;
            const RE xx = x * x, xy = x * y;
            const RE Q = P.A * xx - (RE)2 * P.B * xy + P.C * yy;
            const RE gg = (RE)1 + Q;
            const RE lg2 = fit_log2<RE>(gg);
            const RE e = fit_exp2<RE>(-P.n * lg2);
            const RE m = P.I * e;
            const RE r = m - pl[mo * 8 * NS + mi * 8];
            const RE c = m * P.n * fit_rcp<RE>(gg);
            const RE c2 = (RE)2 * c;
            RE J[NPE];
            J[0] = e;
            J[1] = c2 * (P.C * y - P.B * x);
            J[2] = c2 * (P.A * x - P.B * y);
            J[3] = c2 * Q * P.w2 * (RE)0.5;
            J[4] = c * (P.gK * (xx - yy) - P.e1g2 * Q);
            J[5] = c * ((RE)2 * P.gK * xy - P.e2g2 * Q);
            J[6] = m * (P.nsq2 * lg2) - c * Q * P.dKn;
            chi2 += r * r;
            int k = 0;
#pragma unroll
            for (int i = 0; i < NPE; ++i) {
                g[i] += J[i] * r;
#pragma unroll
                for (int j = i; j < NPE; ++j) a[k++] += J[i] * J[j];
            }
        }
    }
    ne.chi2 = wave_total(chi2);
#pragma unroll
    for (int k = 0; k < NAE; ++k) ne.a[k] = wave_total(a[k]);
#pragma unroll
    for (int k = 0; k < NPE; ++k) ne.g[k] = wave_total(g[k]);
}

// chi2 alone at v (the residual pass without the Jacobian)
template <typename RE>
__device__ __forceinline__ RE ell_chi2(const RE* pix, int lane, const RE* v) {
    const MoffatPar<RE, true> P(v, 6);
    RE cs[5] = {(RE)0, (RE)0, (RE)0, (RE)0, (RE)0};
    const RE lrf = (RE)(lane >> 3) - P.p0, lcf = (RE)(lane & 7) - P.q0;
    const RE* pl = pix + (lane >> 3) * NS + (lane & 7);
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const RE y = (RE)(8 * mo) + lrf;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const RE x = (RE)(8 * mi) + lcf;
            const RE Q = P.A * x * x - (RE)2 * P.B * x * y + P.C * y * y;
            const RE r = P.I * fit_exp2<RE>(-P.n * fit_log2<RE>((RE)1 + Q)) - pl[mo * 8 * NS + mi * 8];
            cs[mi] += r * r;
        }
    }
    return wave_total(((cs[0] + cs[1]) + (cs[2] + cs[3])) + cs[4]);
}

// fp64 gradient J^T r over the fp64 stamp in memory, for the polish of the mixed mode (moffat_gradient of k_fit):
// only the residual needs fp64; the Jacobian, which multiplies a residual of ~1e-3 of the peak at the solution,
// and the per-lane partial sums run in float.
__device__ __forceinline__ void ell_gradient(const double* __restrict__ src, int lane, const double* v, double* gout,
                                             double* chi2out) {
    const double n = sgpr(1.0 / v[6]);
    const double s = lean_exp(0.69314718055994530942 * v[6]) - 1.0;
    const double K = 4.0 * s / (v[3] * v[3]);
    const double e1 = v[4], e2 = v[5], q = 1.0 - e1 * e1 - e2 * e2;
    const double gK = sgpr(K / sqrt(q));
    const double A = sgpr(gK * (1.0 - e1)), B = sgpr(gK * e2), C = sgpr(gK * (1.0 + e1));
    const double I = sgpr(v[0]), p0 = sgpr(v[1]), q0 = sgpr(v[2]);
    const float nf = (float)n, nsq = (float)(n * n), dKn = (float)sgpr((s + 1.0) * 0.69314718055994530942 / s);
    const float w2 = (float)sgpr(2.0 / v[3]), gKf = (float)gK, Af = (float)A, Bf = (float)B, Cf = (float)C;
    const float e1g2 = (float)sgpr(e1 / q), e2g2 = (float)sgpr(e2 / q);
    float g[NPE] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c2sum = 0.f;
    const double lrd = (double)(lane >> 3) - p0, lcd = (double)(lane & 7) - q0;
    const double* pl = src + (lane >> 3) * NS + (lane & 7);
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
        const double y = (double)(8 * mo) + lrd;
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const double x = (double)(8 * mi) + lcd;
            const double Q = fma(A * x, x, fma(C * y, y, -2.0 * B * x * y));
            const double gg = 1.0 + Q;
            const double lg = lean_log(gg);
            const double e = lean_exp(-n * lg);
            const double m = I * e;
            const float r = (float)(m - pl[mo * 8 * NS + mi * 8]);
            c2sum += r * r;
            const float xf = (float)x, yf = (float)y, Qf = (float)Q, mf = (float)m;
            const float c = mf * nf * __builtin_amdgcn_rcpf((float)gg);
            const float cr = c * r;
            g[0] += (float)e * r;
            g[1] += 2.f * cr * (Cf * yf - Bf * xf);
            g[2] += 2.f * cr * (Af * xf - Bf * yf);
            g[3] += cr * Qf * w2;
            g[4] += cr * (gKf * (xf * xf - yf * yf) - e1g2 * Qf);
            g[5] += cr * (2.f * gKf * xf * yf - e2g2 * Qf);
            g[6] += (nsq * mf * (float)lg - c * Qf * dKn) * r;
        }
    }
#pragma unroll
    for (int k = 0; k < NPE; ++k) gout[k] = wave_total((double)g[k]);
    *chi2out = (double)wave_total(c2sum);
}

// size of a step dx towards vn: relative for I, p0, q0, w, eta (k_fit's rule), absolute for e1, e2 (|e| < 1, and
// e = 0 is the round stamp)
template <typename S>
__device__ __forceinline__ S ell_step_size(const S* dx, const S* vn) {
    S rel = (S)0;
#pragma unroll
    for (int k = 0; k < NPE; ++k) {
        const S den = (k == 4 || k == 5) ? (S)1 : fabs(vn[k]) + (S)1.0e-30;
        rel = fmax(rel, fabs(dx[k]) * fit_rcp<S>(den));
    }
    return rel;
}

template <typename S>
__device__ __forceinline__ bool ell_inside(const S* vn) {
    return vn[3] > (S)1.0e-3 && vn[6] > (S)1.0e-3 && vn[6] < (S)1.0e2 &&
           vn[4] * vn[4] + vn[5] * vn[5] <= (S)(kFitMaxE * kFitMaxE);
}

// what fit_lm_descend and fit_polish need of this fit (fit_common.h)
template <typename RE>
struct EllModel {
    static constexpr int NP = NPE, IETA = 6;
    static constexpr bool ROW_FIRST = false, BOUNDED = false;
    const RE* sp;               // the stamp in LDS
    const double* src;          // and in memory
    int lane;
    __device__ __forceinline__ void accumulate(const RE* v, FitNormEq<RE, NPE>& ne) const {
        ell_accumulate<RE>(sp, lane, v, ne);
    }
    __device__ __forceinline__ void gradient(const double* v, double* g, double* chi2) const {
        ell_gradient(src, lane, v, g, chi2);
    }
    template <typename S>
    __device__ __forceinline__ S step_size(const S* dx, const S* vn) const { return ell_step_size<S>(dx, vn); }
    template <typename S>
    __device__ __forceinline__ bool inside(const S* vn) const { return ell_inside<S>(vn); }
};

// one wave per stamp; RE = float: mixed mode (float iterations + fp64 polish), RE = double: f64 mode
template <typename RE>
__global__ void __launch_bounds__(64)
k_fit_ell(int nstamp, const double* __restrict__ stamps, double* __restrict__ fit, double polish_tol) {
    constexpr int NPX = NS * NS / 64;
    static_assert(NPX * 64 == NS * NS, "the lane map assumes 1600 pixels");
    using S = RE;
    const int lane = threadIdx.x & 63;
    const int st = (int)blockIdx.x;
    if (st >= nstamp) return;
    const double* src = stamps + (size_t)st * NS * NS;
    __shared__ RE sp[NS * NS];
    double best = -3.0e38;
    int besto = 0;
#pragma unroll
    for (int m = 0; m < NPX; ++m) {
        const int o = lane + m * 64;
        const double d = src[o];
        sp[o] = (RE)d;
        if (d > best) { best = d; besto = o; }
    }
    __syncthreads();                 // (one wave: the LM passes read pixels other lanes wrote)
    // argmax (first maximum in C order, as np.argmax); the ladder stands here and not in wave_first_max, through which
    // this kernel got another register allocation and its fp64 form ran 0.9 % slower
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_first_max_step(best, besto, o);
    // Start values: k_fit's moment start for (I, p0, q0, w, eta) -- moments over the largest disc around the
    // brightest pixel that fits the stamp, truncation factors by fixed-point iteration -- and the second moments
    // over the same disc for (e1, e2) = ((Mxx - Myy), 2 Mxy) / (Mxx + Myy), exact for an untruncated profile with
    // elliptical isophotes.
    const int p0i = besto / NS, q0i = besto % NS;
    const int rm = min(min(p0i, NS - 1 - p0i), min(q0i, NS - 1 - q0i));
    // Amplitude range (include/mpsfr.h): k_fit's.  The sums of the float iterations and of the polish scale with the
    // square of the peak, and the moment start squares the pixels in float in both modes; a stamp whose brightest
    // pixel lies outside [2^-40, 2^40] in modulus is refused (status 2) rather than fitted wrongly.  Zero, NaN and
    // infinite brightest pixels fail the comparison too.
    const float abest = fabsf((float)best);
    const bool amp_ok = abest >= 0x1p-40f && abest <= 0x1p40f;
    int cnt = 0;
    const double half = 0.5 * best;
    float ms1 = 0.f, ms2 = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
    {
        const float r2 = ((float)rm + 0.5f) * ((float)rm + 0.5f);
        const float lrf = (float)((lane >> 3) - p0i), lcf = (float)((lane & 7) - q0i);
        const double* pl = src + (lane >> 3) * NS + (lane & 7);
#pragma unroll
        for (int mo = 0; mo < 5; ++mo) {
            const float dp = (float)(8 * mo) + lrf, dp2 = dp * dp;
#pragma unroll
            for (int mi = 0; mi < 5; ++mi) {
                const float dq = (float)(8 * mi) + lcf;
                const double dd = pl[mo * 8 * NS + mi * 8];
                cnt += dd > half ? 1 : 0;
                const float din = fmaf(dq, dq, dp2) <= r2 ? (float)dd : 0.f;
                ms1 += din;
                ms2 = fmaf(din, din, ms2);
                mxx = fmaf(din * dq, dq, mxx);
                myy = fmaf(din * dp, dp, myy);
                mxy = fmaf(din * dq, dp, mxy);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    ms1 = wave_total(ms1);
    ms2 = wave_total(ms2);
    mxx = wave_total(mxx);
    myy = wave_total(myy);
    mxy = wave_total(mxy);
    double fw0 = 2.0 * sqrt((double)cnt / kPi);
    fw0 = fmin(fmax(fw0, 1.5), (double)NS);
    float eta0 = 0.4f, e10 = 0.f, e20 = 0.f;
    if (fit_moment_start(ms1, ms2, (float)best, rm, &eta0, &fw0)) {
        const float tr = mxx + myy;
        if (tr > 0.f) {
            e10 = (mxx - myy) / tr;
            e20 = 2.f * mxy / tr;
            const float e = sqrtf(e10 * e10 + e20 * e20);
            if (!(e <= 0.9f)) {                 // (NaN included)
                const float sc = e == e ? 0.9f / e : 0.f;
                e10 *= sc;
                e20 *= sc;
            }
        }
    }
    S v[NPE] = {(S)best, (S)p0i, (S)q0i, (S)fw0, (S)e10, (S)e20, (S)eta0};
    const S tol = sizeof(RE) == 4 ? (S)1.0e-3 : (S)1.0e-10;
    const EllModel<RE> model{sp, src, lane};
    FitNormEq<RE, NPE> ne;
    model.accumulate(v, ne);
    int it = 0;
    int status = fit_lm_descend<EllModel<RE>, S, RE>(model, tol, amp_ok ? kFitMaxIt : 0, amp_ok ? 1 : 2, v, ne, it);
    double vd[NPE];
#pragma unroll
    for (int k = 0; k < NPE; ++k) vd[k] = (double)v[k];
    double chi2 = -1.0;
    if constexpr (sizeof(RE) == 4) {
        // the fp64 polish of k_fit: the float normal matrix of the last iteration, steps until one is below polish_tol
        FitNormEq<double, NPE> np;
#pragma unroll
        for (int k = 0; k < NAE; ++k) np.a[k] = (double)ne.a[k];
        chi2 = fit_polish<NPE, true>(model, FitPolishEnd{kEllPolishMax, polish_tol}, np, vd, status, it);
        if (chi2 < 0.0) {              // a residual pass at the final point, in fp64
            double cs = 0.0;
            {
                const MoffatPar<double, true> P(vd, 6);
                const double lrd = (double)(lane >> 3) - P.p0, lcd = (double)(lane & 7) - P.q0;
                const double* pl = src + (lane >> 3) * NS + (lane & 7);
#pragma unroll 1
                for (int mo = 0; mo < 5; ++mo) {
                    const double y = (double)(8 * mo) + lrd;
#pragma unroll
                    for (int mi = 0; mi < 5; ++mi) {
                        const double x = (double)(8 * mi) + lcd;
                        const double Q = fma(P.A * x, x, fma(P.C * y, y, -2.0 * P.B * x * y));
                        const double r = P.I * lean_exp(-P.n * lean_log(1.0 + Q)) - pl[mo * 8 * NS + mi * 8];
                        cs = fma(r, r, cs);
                    }
                }
            }
            chi2 = wave_total(cs);
        }
    } else {
        chi2 = (double)ell_chi2<RE>(sp, lane, v);
    }
    if (lane != 0) return;
    // Outputs.  n = 1/eta, alpha = w / (2 sqrt(2^eta - 1)); with e = |(e1, e2)| and f = ((1 + e)/(1 - e))^(1/4) the
    // semi-axes are alpha f and alpha / f, the FWHMs w f and w / f, the major axis at rot = atan2(e2, e1) / 2.
    // The covariance is the inverse of the normal matrix of the last iteration times chi2 / (npix - 7); the
    // errors of derived values are propagated to first order.
    const FitEllRow<true> r(vd, 6);
    double o[NFIT_ELL];                 // the row, in registers until the status is known
    o[0] = vd[0]; o[1] = vd[1]; o[2] = vd[2];
    r.write(o, 1.0);
    o[9] = chi2;
    o[10] = (double)it;
#pragma unroll
    for (int k = 21; k < NFIT_ELL; ++k) o[k] = 0.0;
    double cov[NPE][NPE];
    if (fit_spd_inverse<NPE, RE>(ne, cov)) {
        fit_ell_errors<NPE, 6, true>(r, cov, chi2 / (double)(NS * NS - NPE), 1.0, o);
        if (r.n * r.n * sqrt(fmax(cov[6][6], 0.0)) * fabs(r.I) >= kFitIllCond) status |= 4;
    } else {
#pragma unroll
        for (int k = 11; k <= 17; ++k) o[k] = 0.0;
        o[20] = 0.0;
        if (status == 0) status = 2;
    }
    // A row that claims a minimum holds finite numbers only and lies inside the search domain (k_fit's rule).  A NaN
    // or -inf pixel enters the gradient and chi2 but not the normal matrix: every step is NaN, is rejected, and the
    // damping runs out as it does at a minimum -- singular (2), not converged.  A stamp without a maximum (constant,
    // all negative) sends the iteration to the bound eta = 100 of the domain, and one more elongated than the domain
    // allows to the bound |e| = kFitMaxE, where steps are cut until they pass the convergence test: not converged (1)
    // from eta > 90 (n < 1/90) and from |e| > kFitMaxE - 0.01 on.
    bool finite = true;
#pragma unroll
    for (int k = 0; k < NFIT_ELL; ++k)
        if (k != 18) finite = finite && fabs(o[k]) < __builtin_inf();
    if ((status & 3) == 0 && !finite) status = (status & 4) | 2;
    if ((status & 3) == 0 && (vd[6] > 90.0 || r.esq > (kFitMaxE - 0.01) * (kFitMaxE - 0.01))) status = (status & 4) | 1;
    o[18] = (double)status;
    double* row = fit + (size_t)st * NFIT_ELL;
#pragma unroll
    for (int k = 0; k < NFIT_ELL; ++k) row[k] = o[k];
}

}  // namespace

void launch_fit_ell(hipStream_t s, int nstamp, const double* d_stamps, double* d_fit, bool f64) {
    if (nstamp <= 0) return;
    // one wavefront (and workgroup) per stamp, as k_fit
    if (f64)
        hipLaunchKernelGGL(k_fit_ell<double>, dim3(nstamp), dim3(64), 0, s, nstamp, d_stamps, d_fit, 0.0);
    else
        hipLaunchKernelGGL(k_fit_ell<float>, dim3(nstamp), dim3(64), 0, s, nstamp, d_stamps, d_fit, 1.0e-4);
}

}  // namespace mpsfr
