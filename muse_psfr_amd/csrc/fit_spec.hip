// HIP kernel of the PSF-model fit of star cubes, written for gfx950 (MI355X, wave64).  See DESIGN.md section 20.
//
// K_FIT_SPEC: per star, over the used pixels of all fitted layers l, the minimum of
//     sum_l sum_pq w_l (m_l - d_l)^2,   w = 1 / var,   m_l(p, q) = F_l P~_l(p - dp - sp x_l, q - dq - sq x_l) + b_l
// over theta = (dp, dq[, sp, sq]) and (F_l[, b_l]) of every layer; P~ is the Keys resampling of k_fit_psf
// (fit_psf_common.h, unchanged).  Variable projection: at a given theta the (F_l, b_l) of a layer are the closed-form
// weighted linear solve, and the layer contributes the Schur complement of its normal matrix over (F, [b], dp, dq),
//     S_l = A_tt - A_tl A_ll^-1 A_lt,   g_l = J_t^T W r,   chi2_l,
// to the normal equations in theta: with X_l = [I, x_l I] (drift) or I, S = sum X_l^T S_l X_l, g = sum X_l^T g_l.  The
// descent in theta is the shared fit_lm_descend (fit_common.h) over SpecModel.
// One workgroup of kSpecWaves waves per star; wave w takes the layers w, w + W, ...  A layer pass is k_fit_psf's: 25
// pixels per lane in the 8 x 8-block map, the 4 x 4 FIR with wave-uniform taps over the layer's model stamp in LDS
// (apron 10, rows of 72), wave-wide sums with wave_total.  A layer's data and variance are read once per pass, straight
// from memory into registers.  A layer takes two passes per evaluation: the sums of the linear solve (no derivatives),
// then, with (F, b) known, the residuals and the blocks that hold the derivatives -- chi2 and the gradient come from
// residuals, never from differences of large sums.  The per-wave sums of (S, g, chi2) over a wave's layers, taken in
// the order of the layers, are combined through LDS in the order of the waves: a star's row depends on the star alone.
// Every wave then runs the same descent on the same totals, so the control flow is uniform over the workgroup.
// Normalisation by powers of two: one for the data of a star (the brightest used pixel of its fitted layers into
// [1, 2)), one for its weights, one per layer for the model stamp: the sums of the layers add on one scale, exactly.
// The arithmetic is fp64 in both precision modes of a context (the mixed mode has no float path of its own yet).
#include "device_common.h"
#include "fit_common.h"
#include "fit_psf_common.h"

namespace mpsfr {

namespace {

constexpr int kSpecWaves = 4;                        // W: four model stamps of 34560 bytes in the 160 KiB of a CU
constexpr int kSpecMaxLayers = 4096;                 // MPSFR_MAX_SPEC_LAYERS
constexpr int kSpecHead = 16, kSpecLayer = 10;       // MPSFR_NFIT_SPEC, MPSFR_NFIT_SPEC_LAYER
constexpr int FLAG_DRIFT = 16;                       // MPSFR_FIT_DRIFT
constexpr int kSpecStamp = kPsfSide * kPsfStride;    // elements of a model stamp with its apron
constexpr short kSpecLeftOut = -32768;               // lkp of a layer that is not fitted
constexpr int kSpecRed = 16;                         // values a wave hands to the combination
static_assert(2 * NS * NS <= kSpecStamp, "the collapsed images of the start fit into a wave's stamp");

// what a wave needs of its star to read a layer
struct SpecStar {
    const double *src, *vsrc, *psrc, *x;     // cube, variance (or the cube), model cube of the star; x [nl] or nullptr
    bool has_var;
    int nl;
    FitNorm norm;                            // one normalisation of data and weights for all layers of the star
};

// The linear problem of a layer at the shift (dpl, dql): the normal matrix over (F, [b]), its right-hand side, the
// solution and the inverse.  ok: the matrix is positive definite.
template <bool BG>
struct SpecLin {
    double app, ap1, a11, rp, r1;            // sum w P~^2, sum w P~, sum w, sum w P~ d, sum w d
    double ipp, ip1, i11;                    // A_ll^-1
    double F, b;
    int nused;
    bool ok;
};
template <bool BG>
__device__ __forceinline__ void spec_linear(const SpecStar& s, const double* src, const double* vsrc, const double* pl,
                                            int lane, double dpl, double dql, SpecLin<BG>& L) {
    const KeysTaps<double> ty(dpl), tx(dql);
    const LdsStamp<double> st(pl, ty.f, tx.f);
    double app = 0.0, ap1 = 0.0, a11 = 0.0, rp = 0.0, r1 = 0.0;
    int nu = 0;
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            double val, gy, gx, dn, wn;
            psf_interp<double, false>(st, p * kPsfStride + q, p, q, ty, tx, val, gy, gx);
            s.norm.pixel(src, vsrc, s.has_var, o, dn, wn);
            nu += wn > 0.0 ? 1 : 0;
            const double wp = wn * val;
            app += wp * val;
            rp += wp * dn;
            if constexpr (BG) {
                ap1 += wp;
                a11 += wn;
                r1 += wn * dn;
            }
        }
    }
    L.app = wave_total(app);
    L.rp = wave_total(rp);
    L.nused = (int)wave_total((double)nu);
    if constexpr (BG) {
        L.ap1 = wave_total(ap1);
        L.a11 = wave_total(a11);
        L.r1 = wave_total(r1);
        // positive definite as fit_chol tests it: the diagonal, and the pivot of the unit-diagonal form
        const double c2 = (L.ap1 * L.ap1) / (L.app * L.a11);
        L.ok = L.app > 0.0 && L.a11 > 0.0 && (1.0 - c2) > 0.0;
        const double idet = 1.0 / (L.app * L.a11 - L.ap1 * L.ap1);
        L.ipp = L.a11 * idet;
        L.ip1 = -L.ap1 * idet;
        L.i11 = L.app * idet;
        L.F = L.ipp * L.rp + L.ip1 * L.r1;
        L.b = L.ip1 * L.rp + L.i11 * L.r1;
    } else {
        L.ap1 = 0.0; L.a11 = 0.0; L.r1 = 0.0;
        L.ok = L.app > 0.0;
        L.ipp = 1.0 / L.app;
        L.ip1 = 0.0; L.i11 = 0.0;
        L.F = L.ipp * L.rp;
        L.b = 0.0;
    }
    L.ok = L.ok && fabs(L.F) < __builtin_inf() && fabs(L.b) < __builtin_inf();
}

// The blocks of a layer that hold the derivatives, at its linear optimum (F, b): J_t = -F (dP~/dy, dP~/dx);
// apt, a1t: the rows of A_lt; att: A_tt (00, 01, 11); gt: J_t^T W r; chi2.
struct SpecBlocks {
    double apt[2], a1t[2], att[3], gt[2], chi2;
};
template <bool BG>
__device__ __forceinline__ void spec_blocks(const SpecStar& s, const double* src, const double* vsrc, const double* pl,
                                            int lane, double dpl, double dql, double F, double b, SpecBlocks& B) {
    const KeysTaps<double> ty(dpl), tx(dql);
    const LdsStamp<double> st(pl, ty.f, tx.f);
    double apt0 = 0.0, apt1 = 0.0, a1t0 = 0.0, a1t1 = 0.0, t00 = 0.0, t01 = 0.0, t11 = 0.0, g0 = 0.0, g1 = 0.0,
           chi2 = 0.0;
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll 1
    for (int mo = 0; mo < 5; ++mo) {
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
            const int p = 8 * mo + lr, q = 8 * mi + lc;
            const int o = p * NS + q;
            double val, gy, gx, dn, wn;
            psf_interp<double, true>(st, p * kPsfStride + q, p, q, ty, tx, val, gy, gx);
            s.norm.pixel(src, vsrc, s.has_var, o, dn, wn);
            const double r = (F * val + b) - dn;
            const double j0 = -F * gy, j1 = -F * gx;
            const double wr = wn * r;
            chi2 += wr * r;
            g0 += j0 * wr;
            g1 += j1 * wr;
            const double w0 = wn * j0, w1 = wn * j1;
            apt0 += w0 * val;
            apt1 += w1 * val;
            if constexpr (BG) {
                a1t0 += w0;
                a1t1 += w1;
            }
            t00 += w0 * j0;
            t01 += w0 * j1;
            t11 += w1 * j1;
        }
    }
    B.chi2 = wave_total(chi2);
    B.gt[0] = wave_total(g0);
    B.gt[1] = wave_total(g1);
    B.apt[0] = wave_total(apt0);
    B.apt[1] = wave_total(apt1);
    if constexpr (BG) {
        B.a1t[0] = wave_total(a1t0);
        B.a1t[1] = wave_total(a1t1);
    } else {
        B.a1t[0] = 0.0; B.a1t[1] = 0.0;
    }
    B.att[0] = wave_total(t00);
    B.att[1] = wave_total(t01);
    B.att[2] = wave_total(t11);
}

// U = A_ll^-1 A_lt (rows F, b; columns dp, dq)
template <bool BG>
__device__ __forceinline__ void spec_lt(const SpecLin<BG>& L, const SpecBlocks& B, double (&uf)[2], double (&ub)[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        uf[k] = L.ipp * B.apt[k] + L.ip1 * B.a1t[k];
        ub[k] = L.ip1 * B.apt[k] + L.i11 * B.a1t[k];
    }
}

// the shift of layer l at theta
template <bool DRIFT, typename S>
__device__ __forceinline__ void spec_shift(const S* v, double xl, double& dpl, double& dql) {
    dpl = (double)v[0];
    dql = (double)v[1];
    if constexpr (DRIFT) {
        dpl += (double)v[2] * xl;
        dql += (double)v[3] * xl;
    }
}

// the sums of the waves (red[w][0 .. n)) added in the order of the waves; every thread gets the totals
template <int N>
__device__ __forceinline__ void spec_combine(double (*red)[kSpecRed], int wave, int lane, const double (&part)[N],
                                             double (&tot)[N]) {
    static_assert(N <= kSpecRed, "room of a wave");
    __syncthreads();                          // (the values of the combination before this one have been read)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave][k] = part[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < kSpecWaves; ++w) t += red[w][k];
        tot[k] = sgpr(t);
    }
}

// what fit_lm_descend needs of this fit (fit_common.h)
template <bool DRIFT, bool BG>
struct SpecModel {
    static constexpr int NP = DRIFT ? 4 : 2, IETA = -1;
    static constexpr bool ROW_FIRST = false, BOUNDED = true;
    SpecStar s;
    double* pl;                  // the wave's model stamp in LDS
    const short* lkp;            // [nl] the power of two of a layer's model stamp, or kSpecLeftOut
    double (*red)[kSpecRed];
    int wave, lane;
    double xmin, xmax;           // over the fitted layers
    mutable bool sing;           // the last evaluation met a layer whose linear solve is singular

    __device__ __forceinline__ void accumulate(const double* v, FitNormEq<double, NP>& ne) const {
        constexpr int NA = NP * (NP + 1) / 2, NT = NA + NP + 2;
        double part[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) part[k] = 0.0;
        for (int l0 = 0; l0 < s.nl; l0 += kSpecWaves) {
            const int l = l0 + wave;
            const int kp = l < s.nl ? __builtin_amdgcn_readfirstlane((int)lkp[l]) : (int)kSpecLeftOut;
            const bool act = kp != (int)kSpecLeftOut;
            const size_t off = (size_t)(act ? l : 0) * NS * NS;
            if (act) psf_stamp_load(s.psrc + off, kp, pl, lane);
            __syncthreads();
            if (act) {
                const double xl = DRIFT ? sgpr(s.x[l]) : 0.0;
                double dpl, dql;
                spec_shift<DRIFT, double>(v, xl, dpl, dql);
                SpecLin<BG> L;
                spec_linear<BG>(s, s.src + off, s.vsrc + off, pl, lane, dpl, dql, L);
                SpecBlocks B;
                spec_blocks<BG>(s, s.src + off, s.vsrc + off, pl, lane, dpl, dql, L.F, L.b, B);
                double uf[2], ub[2];
                spec_lt<BG>(L, B, uf, ub);
                // S_l = A_tt - A_tl U
                const double s00 = B.att[0] - (B.apt[0] * uf[0] + B.a1t[0] * ub[0]);
                const double s01 = B.att[1] - (B.apt[0] * uf[1] + B.a1t[0] * ub[1]);
                const double s11 = B.att[2] - (B.apt[1] * uf[1] + B.a1t[1] * ub[1]);
                if constexpr (DRIFT) {
                    const double x2 = xl * xl;
                    part[0] += s00; part[1] += s01; part[2] += xl * s00; part[3] += xl * s01;
                    part[4] += s11; part[5] += xl * s01; part[6] += xl * s11;
                    part[7] += x2 * s00; part[8] += x2 * s01;
                    part[9] += x2 * s11;
                    part[NA + 0] += B.gt[0]; part[NA + 1] += B.gt[1];
                    part[NA + 2] += xl * B.gt[0]; part[NA + 3] += xl * B.gt[1];
                } else {
                    part[0] += s00; part[1] += s01; part[2] += s11;
                    part[NA + 0] += B.gt[0]; part[NA + 1] += B.gt[1];
                }
                part[NA + NP] += B.chi2;
                if (!L.ok) part[NA + NP + 1] += 1.0;
            }
            __syncthreads();
        }
        double tot[NT];
        spec_combine<NT>(red, wave, lane, part, tot);
#pragma unroll
        for (int k = 0; k < NA; ++k) ne.a[k] = tot[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) ne.g[k] = tot[NA + k];
        sing = tot[NA + NP + 1] > 0.0;
        ne.chi2 = sing ? __builtin_nan("") : tot[NA + NP];         // (a NaN is refused by the descent)
    }
    template <typename S>
    __device__ __forceinline__ S step_size(const S* dx, const S*) const {      // pixels (|x| <= 1)
        S rel = fmax(fabs(dx[0]), fabs(dx[1]));
        if constexpr (DRIFT) rel = fmax(rel, fmax(fabs(dx[2]), fabs(dx[3])));
        return rel;
    }
    // every fitted layer inside the domain: the shift is linear in x, so the two ends decide
    template <typename S>
    __device__ __forceinline__ bool inside(const S* vn) const {
        double p0, q0, p1, q1;
        spec_shift<DRIFT, S>(vn, xmin, p0, q0);
        spec_shift<DRIFT, S>(vn, xmax, p1, q1);
        return psf_inside<double>(p0, q0) && psf_inside<double>(p1, q1);
    }
};

template <typename RE, bool DRIFT, bool BG>
__global__ void __launch_bounds__(64 * kSpecWaves)
k_fit_spec(int nstar, int nl, const double* __restrict__ cubes, const double* __restrict__ var, int npsf,
           const double* __restrict__ psf, const int32_t* __restrict__ psf_index, const double* __restrict__ shift,
           const double* __restrict__ x, double* __restrict__ fit) {
    static_assert(sizeof(RE) == 8, "fp64 only");
    using Model = SpecModel<DRIFT, BG>;
    constexpr int NP = Model::NP, NLIN = BG ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int st = (int)blockIdx.x;
    if (st >= nstar) return;
    __shared__ double pls[kSpecWaves][kSpecStamp];
    __shared__ double red[kSpecWaves][kSpecRed];
    __shared__ short lkp[kSpecMaxLayers];
    double* pl = pls[wave];
    const size_t cube = (size_t)nl * NS * NS;
    const size_t nrow = (size_t)kSpecHead + (size_t)kSpecLayer * nl;
    double* orow = fit + (size_t)st * nrow;
    const bool has_var = var != nullptr;
    const int ip = psf_index ? psf_index[st] : st;
    double dp0 = 0.0, dq0 = 0.0;
    if (shift) { dp0 = shift[2 * (size_t)st]; dq0 = shift[2 * (size_t)st + 1]; }
    const bool args_ok = ip >= 0 && ip < npsf && psf_inside<double>(dp0, dq0);
    SpecStar s;
    s.src = cubes + (size_t)st * cube;
    s.vsrc = has_var ? var + (size_t)st * cube : s.src;
    s.psrc = psf + (size_t)(args_ok ? ip : 0) * cube;
    s.x = x;
    s.has_var = has_var;
    s.nl = nl;

    // First pass over the wave's layers: which are fitted, and over the fitted ones the brightest used pixel, the
    // smallest valid variance, the largest used modulus, the used pixels, the range of x.  The layer blocks get their
    // n_used and status here, and zeros.
    double wbest = -3.0e38, wvmin = 3.0e38, wamax = 0.0, wxmin = 3.0e38, wxmax = -3.0e38;
    int wused = 0, wfit = 0;
    for (int l = wave; l < nl; l += kSpecWaves) {
        const size_t off = (size_t)l * NS * NS;
        FitStarScan<false> ls;
        PsfStampScan<false> lm;
        psf_scan(ls, lm, s.src + off, s.vsrc + off, has_var, s.psrc + off, lane);
        const int nused = ls.nused;
        // a layer is fitted if its pixels suffice for its linear variables and its model stamp is fit to use
        const bool fitted = !fit_pixels_refused(nused, ls.nbad, NLIN) && !lm.refused();
        if (fitted) {
            wbest = fmax(wbest, ls.best);
            wvmin = fmin(wvmin, ls.vmin);
            wamax = fmax(wamax, ls.amax);
            wused += nused;
            wfit += 1;
            if constexpr (DRIFT) {
                const double xl = x[l];
                wxmin = fmin(wxmin, xl);
                wxmax = fmax(wxmax, xl);
            }
        }
        if (lane == 0) {
            lkp[l] = fitted ? (short)ilogb(lm.pamax) : kSpecLeftOut;
            double* ol = orow + kSpecHead + (size_t)kSpecLayer * l;
#pragma unroll
            for (int k = 0; k < kSpecLayer; ++k) ol[k] = 0.0;
            ol[7] = (double)nused;
            ol[8] = fitted ? 0.0 : 2.0;
        }
    }
    // the star's values: maxima, minima and counts of the waves (no order matters)
    if (lane == 0) {
        red[wave][0] = wbest; red[wave][1] = wvmin; red[wave][2] = wamax; red[wave][3] = wxmin;
        red[wave][4] = wxmax; red[wave][5] = (double)wused; red[wave][6] = (double)wfit;
    }
    __syncthreads();
    double best = red[0][0], vmin = red[0][1], amax = red[0][2], xmin = red[0][3], xmax = red[0][4];
    int nused = (int)red[0][5], nfit = (int)red[0][6];
#pragma unroll
    for (int w = 1; w < kSpecWaves; ++w) {
        best = fmax(best, red[w][0]); vmin = fmin(vmin, red[w][1]); amax = fmax(amax, red[w][2]);
        xmin = fmin(xmin, red[w][3]); xmax = fmax(xmax, red[w][4]);
        nused += (int)red[w][5]; nfit += (int)red[w][6];
    }
    best = sgpr(best); vmin = sgpr(vmin); amax = sgpr(amax); xmin = sgpr(xmin); xmax = sgpr(xmax);
    nused = __builtin_amdgcn_readfirstlane(nused);
    nfit = __builtin_amdgcn_readfirstlane(nfit);
    if constexpr (!DRIFT) { xmin = 0.0; xmax = 0.0; }
    const int dofi = nused - (NP + NLIN * nfit);
    auto head = [&](int status) {            // the head of a row that is not fitted
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < kSpecHead; ++k) orow[k] = 0.0;
            orow[10] = (double)status;
            orow[11] = (double)nused;
            orow[12] = (double)nfit;
        }
    };
    // Rows that are not fitted: a model index or a given start outside its range, no fitted layer, too few used pixels
    // for the variables, with the drift fewer than two distinct x among the fitted layers, and the range rule of the
    // intake over the used pixels of the fitted layers.
    if (!args_ok || nfit < 1 || dofi < 1 || (DRIFT && !(xmax > xmin)) || fit_range_refused(best, amax)) {
        head(2);
        return;
    }
    s.norm = FitNorm(best, vmin, has_var);
    const int kx = s.norm.kx;

    // the wave's stamp: zero, apron included (the layers are loaded into its interior, one after the other)
    psf_stamp_clear(pl, lane);
    __syncthreads();
    if (!shift) {
        // The start: the first maximum of sum_l w_l d_l over the used pixels of the fitted layers minus the first
        // maximum of sum_l P_l, brought into the domain.  The two images of a wave's layers grow in its stamp; they are
        // added in the order of the waves.
        for (int l = wave; l < nl; l += kSpecWaves) {
            if (__builtin_amdgcn_readfirstlane((int)lkp[l]) == (int)kSpecLeftOut) continue;
            const size_t off = (size_t)l * NS * NS;
#pragma unroll 5
            for (int m = 0; m < kFitPix; ++m) {
                const int o = lane + m * 64;
                double dn, wn;
                s.norm.pixel(s.src + off, s.vsrc + off, has_var, o, dn, wn);
                pl[o] += wn * dn;
                pl[NS * NS + o] += s.psrc[off + o];
            }
        }
        __syncthreads();
        double cb = -3.0e38, pb = -3.0e38;
        int cbo = 0, pbo = 0;
#pragma unroll 5
        for (int m = 0; m < kFitPix; ++m) {
            const int o = lane + m * 64;
            double c = pls[0][o], p = pls[0][NS * NS + o];
#pragma unroll
            for (int w = 1; w < kSpecWaves; ++w) { c += pls[w][o]; p += pls[w][NS * NS + o]; }
            if (c > cb) { cb = c; cbo = o; }
            if (p > pb) { pb = p; pbo = o; }
        }
        wave_first_max(cb, cbo);
        wave_first_max(pb, pbo);
        cbo = __builtin_amdgcn_readfirstlane(cbo);
        pbo = __builtin_amdgcn_readfirstlane(pbo);
        dp0 = fmin(fmax((double)(cbo / NS - pbo / NS), -kPsfMaxShift), kPsfMaxShift);
        dq0 = fmin(fmax((double)(cbo % NS - pbo % NS), -kPsfMaxShift), kPsfMaxShift);
        __syncthreads();
        for (int o = lane; o < 2 * NS * NS; o += 64) pl[o] = 0.0;
        __syncthreads();
    }
    const Model model{s, pl, lkp, red, wave, lane, xmin, xmax, false};
    double v[NP];
    v[0] = dp0;
    v[1] = dq0;
    if constexpr (DRIFT) { v[2] = 0.0; v[3] = 0.0; }
    FitNormEq<double, NP> ne;
    model.accumulate(v, ne);
    if (model.sing) {                        // a singular start
        head(2);
        return;
    }
    int it = 0;
    int status = fit_lm_descend<Model, double, double>(model, 1.0e-12, kFitMaxIt, 1, v, ne, it);
    // a descent that ended on a refused point (the domain, or a singular layer) has not found a minimum; nor has a fit
    // that rests on the bound of the domain
    if (status == 0 && model.sing) status = 1;
    {
        double p0, q0, p1, q1;
        spec_shift<DRIFT, double>(v, xmin, p0, q0);
        spec_shift<DRIFT, double>(v, xmax, p1, q1);
        const double far = fmax(fmax(fabs(p0), fabs(q0)), fmax(fabs(p1), fabs(q1)));
        if (status == 0 && !(far < kPsfMaxShift)) status = 1;
    }
    // the normal equations and chi2 at the final point, the covariance of theta
    FitNormEq<double, NP> nf;
    model.accumulate(v, nf);
    if (model.sing) status = 2;
    const double dof = (double)dofi;
    const double chi2 = nf.chi2;
    const double sc = chi2 / dof;
    double cov[NP][NP];
    if (status != 2 && !fit_spd_inverse<NP, double>(nf, cov)) status = 2;
    if (status == 2) {
        head(2);
        return;
    }
    // Last pass: the layer blocks.  The amplitudes leave the normalisation: F and its error by 2^(kx - kp), b and its
    // error by 2^kx, chi2 by 2^(2 kx - kv).  cov(F, b) = (A_ll^-1 + B cov(theta) B^T) chi2 / dof, B = A_ll^-1 A_lt X_l.
    const double up = ldexp(1.0, kx), upc = ldexp(1.0, 2 * kx - s.norm.kv);
    double notfinite = 0.0;
    for (int l0 = 0; l0 < nl; l0 += kSpecWaves) {
        const int l = l0 + wave;
        const int kp = l < nl ? __builtin_amdgcn_readfirstlane((int)lkp[l]) : (int)kSpecLeftOut;
        const bool act = kp != (int)kSpecLeftOut;
        const size_t off = (size_t)(act ? l : 0) * NS * NS;
        double psum = 0.0;
        if (act) psum = psf_stamp_load(s.psrc + off, kp, pl, lane);
        __syncthreads();
        if (act) {
            psum = wave_total(psum);
            const double xl = DRIFT ? sgpr(x[l]) : 0.0;
            double dpl, dql;
            spec_shift<DRIFT, double>(v, xl, dpl, dql);
            SpecLin<BG> L;
            spec_linear<BG>(s, s.src + off, s.vsrc + off, pl, lane, dpl, dql, L);
            SpecBlocks B;
            spec_blocks<BG>(s, s.src + off, s.vsrc + off, pl, lane, dpl, dql, L.F, L.b, B);
            double uf[2], ub[2];
            spec_lt<BG>(L, B, uf, ub);
            double bf[NP], bb[NP];
            bf[0] = uf[0]; bf[1] = uf[1]; bb[0] = ub[0]; bb[1] = ub[1];
            if constexpr (DRIFT) { bf[2] = xl * uf[0]; bf[3] = xl * uf[1]; bb[2] = xl * ub[0]; bb[3] = xl * ub[1]; }
            double qf = 0.0, qb = 0.0;
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    qf += bf[i] * cov[i][j] * bf[j];
                    qb += bb[i] * cov[i][j] * bb[j];
                }
            const double upf = ldexp(1.0, kx - kp);
            double o[kSpecLayer];
            o[0] = L.F * upf;
            o[1] = BG ? L.b * up : 0.0;
            o[2] = sqrt(fmax((L.ipp + qf) * sc, 0.0)) * upf;
            o[3] = BG ? sqrt(fmax((L.i11 + qb) * sc, 0.0)) * up : 0.0;
            o[4] = o[0] * psum;
            o[5] = o[2] * fabs(psum);
            o[6] = B.chi2 * upc;
            o[7] = (double)L.nused;
            o[8] = 0.0;
            o[9] = 0.0;
            bool finite = true;
#pragma unroll
            for (int k = 0; k < kSpecLayer; ++k) finite = finite && fabs(o[k]) < __builtin_inf();
            if (!finite) notfinite += 1.0;
            if (lane == 0) {
                double* ol = orow + kSpecHead + (size_t)kSpecLayer * l;
#pragma unroll
                for (int k = 0; k < kSpecLayer; ++k) ol[k] = o[k];
            }
        }
        __syncthreads();
    }
    double nfp[1] = {notfinite}, nft[1];
    spec_combine<1>(red, wave, lane, nfp, nft);
    if (threadIdx.x != 0) return;
    double* o = orow;
#pragma unroll
    for (int k = 0; k < kSpecHead; ++k) o[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        o[k] = v[k];
        o[4 + k] = sqrt(fmax(cov[k][k] * sc, 0.0));
    }
    o[8] = chi2 * upc;
    o[9] = (double)it;
    o[11] = (double)nused;
    o[12] = (double)nfit;
    o[13] = dof;
    // a row that claims a minimum holds finite numbers only
    bool finite = nft[0] == 0.0;
#pragma unroll
    for (int k = 0; k < kSpecHead; ++k) finite = finite && fabs(o[k]) < __builtin_inf();
    if (!finite && (status & 3) == 0) status = 2;
    o[10] = (double)status;
}

}  // namespace

void launch_fit_spec(hipStream_t s, int nstar, int nl, const double* d_cubes, const double* d_var, int npsf,
                     const double* d_psf, const int32_t* d_index, const double* d_shift, const double* d_x, int flags,
                     double* d_fit, bool f64) {
    if (nstar <= 0 || nl <= 0 || nl > kSpecMaxLayers) return;
    (void)f64;                  // both modes run the fp64 kernel
    const dim3 grid(nstar), block(64 * kSpecWaves);
    switch (flags & (FLAG_BACKGROUND | FLAG_DRIFT)) {
    case 0:
        hipLaunchKernelGGL((k_fit_spec<double, false, false>), grid, block, 0, s, nstar, nl, d_cubes, d_var, npsf,
                           d_psf, d_index, d_shift, d_x, d_fit);
        break;
    case FLAG_BACKGROUND:
        hipLaunchKernelGGL((k_fit_spec<double, false, true>), grid, block, 0, s, nstar, nl, d_cubes, d_var, npsf, d_psf,
                           d_index, d_shift, d_x, d_fit);
        break;
    case FLAG_DRIFT:
        hipLaunchKernelGGL((k_fit_spec<double, true, false>), grid, block, 0, s, nstar, nl, d_cubes, d_var, npsf, d_psf,
                           d_index, d_shift, d_x, d_fit);
        break;
    default:
        hipLaunchKernelGGL((k_fit_spec<double, true, true>), grid, block, 0, s, nstar, nl, d_cubes, d_var, npsf, d_psf,
                           d_index, d_shift, d_x, d_fit);
        break;
    }
}

}  // namespace mpsfr
