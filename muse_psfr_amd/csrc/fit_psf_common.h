// Device code shared by the kernels that resample a PSF model stamp (k_fit_psf in fit_psf.hip, k_fit_group in
// fit_group_impl.h, k_fit_spec in fit_spec.hip and, through frame_common.h, k_render_tiles in render.hip and k_ff_star
// in frame_fit_impl.h): the constants of the model stamp in LDS, the Keys tap weights of one axis (KeysTaps), the model
// stamp with its apron in LDS and the fp64 one in memory (LdsStamp, GlobalStamp), the 4 x 4 FIR with its
// derivatives (psf_interp), the domain of the shift (psf_inside) and
// the intake of a model stamp (k_fit_psf, k_fit_spec): its first pass, taken with the star's (PsfStampScan,
// psf_scan), its refusal rule and its load into the apron layout (psf_stamp_clear, psf_stamp_load).  The intake of the
// star is fit_common.h's.  See DESIGN.md sections 13, 18 and 19.  Everything here has internal linkage.
#pragma once
#include "device_common.h"
#include "fit_common.h"

namespace mpsfr {
namespace {

constexpr int kPsfApron = 10;
constexpr int kPsfSide = NS + 2 * kPsfApron;       // 60 rows
constexpr int kPsfStride = 72;                     // elements per row (the last 12 are never read)
constexpr double kPsfMaxShift = 8.0;               // |dp|, |dq| bound
constexpr int FLAG_BACKGROUND = 1, FLAG_FIXED_SHIFT = 4;     // MPSFR_FIT_BACKGROUND / MPSFR_FIT_FIXED_SHIFT
static_assert(kPsfApron >= (int)kPsfMaxShift + 2 && kPsfStride >= kPsfSide, "the taps stay inside the apron");

__device__ __forceinline__ float psf_floor(float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double psf_floor(double x) { return __builtin_floor(x); }

// The tap weights of one axis at the shift d: the sample position of pixel p is y = p - d = (p + f) + t with
// f = floor(-d), t in [0, 1); the taps are the stamp's rows p + f - 1 .. p + f + 2 with the weights w = c(t + 1),
// c(t), c(t - 1), c(t - 2) and the derivatives dw = c' at the same places (d/dy).
template <typename RE>
struct KeysTaps {
    RE w[4], dw[4];
    int f;
    __device__ __forceinline__ explicit KeysTaps(RE d) {
        const RE s = -d;
        const RE fl = psf_floor(s);
        const RE t = s - fl, t2 = t * t, t3 = t2 * t;
        f = (int)fl;
        w[0] = (RE)0.5 * (-t3 + (RE)2 * t2 - t);
        w[1] = (RE)0.5 * ((RE)3 * t3 - (RE)5 * t2 + (RE)2);
        w[2] = (RE)0.5 * ((RE)-3 * t3 + (RE)4 * t2 + t);
        w[3] = (RE)0.5 * (t3 - t2);
        dw[0] = (RE)0.5 * ((RE)-3 * t2 + (RE)4 * t - (RE)1);
        dw[1] = (RE)0.5 * ((RE)9 * t2 - (RE)10 * t);
        dw[2] = (RE)0.5 * ((RE)-9 * t2 + (RE)8 * t + (RE)1);
        dw[3] = (RE)0.5 * ((RE)3 * t2 - (RE)2 * t);
    }
};

// the model stamp in LDS, with its apron: tap (a, b) of pixel (p, q) without a bounds test
template <typename LT>
struct LdsStamp {
    const LT* base;
    __device__ __forceinline__ LdsStamp(const LT* pl, int fy, int fx)
        : base(pl + (fy - 1 + kPsfApron) * kPsfStride + (fx - 1 + kPsfApron)) {}
    template <typename RE>
    __device__ __forceinline__ RE at(int o, int, int, int a, int b) const {
        return (RE)base[o + a * kPsfStride + b];
    }
};
// the fp64 model stamp in memory (times `scale`, the power of two of its normalisation), zero outside
struct GlobalStamp {
    const double* P;
    double scale;
    int fy, fx;
    template <typename RE>
    __device__ __forceinline__ RE at(int, int p, int q, int a, int b) const {
        const int r = p + fy - 1 + a, c = q + fx - 1 + b;
        const bool in = (unsigned)r < (unsigned)NS && (unsigned)c < (unsigned)NS;
        const double v = P[in ? r * NS + c : 0];
        return in ? (RE)(v * scale) : (RE)0;
    }
};

// P~ at pixel (p, q) (o: its offset in the apron stamp) and, with DERIV, its derivatives along y and x
template <typename RE, bool DERIV, typename ST>
__device__ __forceinline__ void psf_interp(const ST& st, int o, int p, int q, const KeysTaps<RE>& ty,
                                           const KeysTaps<RE>& tx, RE& val, RE& gy, RE& gx) {
    val = (RE)0; gy = (RE)0; gx = (RE)0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        RE h = (RE)0, hd = (RE)0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const RE t = st.template at<RE>(o, p, q, a, b);
            h += tx.w[b] * t;
            if constexpr (DERIV) hd += tx.dw[b] * t;
        }
        val += ty.w[a] * h;
        if constexpr (DERIV) {
            gy += ty.dw[a] * h;
            gx += ty.w[a] * hd;
        }
    }
}

template <typename S>
__device__ __forceinline__ bool psf_inside(S dp, S dq) {          // (NaN fails)
    return fabs(dp) <= (S)kPsfMaxShift && fabs(dq) <= (S)kPsfMaxShift;
}

// The first pass over a model stamp: max |P|, the pixels that are not finite and, with ARGMAX, its first maximum in C
// order; add() takes one pixel, reduce_step() is one step of the ladder over the wave.
template <bool ARGMAX>
struct PsfStampScan {
    double pbest = -3.0e38, pamax = 0.0;
    int pbesto = 0, pbad = 0;
    __device__ __forceinline__ void add(int o, double pv) {
        pbad += fabs(pv) < __builtin_inf() ? 0 : 1;
        pamax = fmax(pamax, fabs(pv));
        if constexpr (ARGMAX) {
            if (pv > pbest) { pbest = pv; pbesto = o; }
        }
    }
    __device__ __forceinline__ void reduce_step(int o) {
        if constexpr (ARGMAX) wave_first_max_step(pbest, pbesto, o);
        pamax = fmax(pamax, __shfl_xor(pamax, o, 64));
        pbad += __shfl_xor(pbad, o, 64);
    }
    // a model stamp that is not fitted: not finite, or its brightest pixel outside [2^-40, 2^40] in modulus (an
    // all-zero stamp included)
    __device__ __forceinline__ bool refused() const { return pbad > 0 || !fit_amplitude_ok(pamax); }
};

// the first pass over a star and its model stamp: one loop over a lane's pixels (o = lane + 64 m), one ladder
template <bool AS, bool AM>
__device__ __forceinline__ void psf_scan(FitStarScan<AS>& star, PsfStampScan<AM>& mod, const double* src,
                                         const double* vsrc, bool has_var, const double* psrc, int lane) {
#pragma unroll 5
    for (int m = 0; m < kFitPix; ++m) {
        const int o = lane + m * 64;
        star.add(o, src[o], has_var ? vsrc[o] : 1.0, has_var);
        mod.add(o, psrc[o]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        star.reduce_step(o);
        mod.reduce_step(o);
    }
}

// the apron stamp, all of it, to zero (the caller synchronises before the interior is written)
template <typename LT>
__device__ __forceinline__ void psf_stamp_clear(LT* pl, int lane) {
    for (int o = lane; o < kPsfSide * kPsfStride; o += 64) pl[o] = (LT)0;
}
// The planes of a star in LDS and what fills them: the normalised values into sp, the weights into sw
template <typename LT>
struct PsfStarPlanes {
    const FitNorm& norm;
    const double *src, *vsrc;
    bool has_var;
    LT *sp, *sw;
};
// The model stamp times 2^-kp (its brightest pixel in modulus into [1, 2)) into the interior of the apron stamp and,
// with STAR, the normalised star and its weights into their planes in the same loop.  Returns the lane's share of
// sum P, its pixels added in ascending m: wave_total of it is the sum the flux columns use.
template <bool STAR, typename LT>
__device__ __forceinline__ double psf_stamp_load_loop(const double* __restrict__ psrc, int kp, LT* pl, int lane,
                                                      const PsfStarPlanes<LT>* star) {
    const double pscale = ldexp(1.0, -kp);
    double ps = 0.0;
#pragma unroll 5
    for (int m = 0; m < kFitPix; ++m) {
        const int o = lane + m * 64;
        if constexpr (STAR) {
            double dn, wn;
            star->norm.pixel(star->src, star->vsrc, star->has_var, o, dn, wn);
            star->sp[o] = (LT)dn;
            star->sw[o] = (LT)wn;
        }
        const double pv = psrc[o];
        ps += pv;
        const int p = o / NS, q = o - p * NS;
        pl[(p + kPsfApron) * kPsfStride + q + kPsfApron] = (LT)(pv * pscale);
    }
    return ps;
}
// the model stamp alone (k_fit_spec, which reads the layers of its star from memory at every pass)
template <typename LT>
__device__ __forceinline__ double psf_stamp_load(const double* __restrict__ psrc, int kp, LT* pl, int lane) {
    return psf_stamp_load_loop<false, LT>(psrc, kp, pl, lane, nullptr);
}
// the model stamp and the star (k_fit_psf)
template <typename LT>
__device__ __forceinline__ double psf_stamp_load(const double* __restrict__ psrc, int kp, LT* pl, int lane,
                                                 const PsfStarPlanes<LT>& star) {
    return psf_stamp_load_loop<true, LT>(psrc, kp, pl, lane, &star);
}

}  // namespace
}  // namespace mpsfr
