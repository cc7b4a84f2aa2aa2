// Device code shared by the PSF-model fits (k_fit_psf in fit_psf.hip, k_fit_group in fit_group_impl.h): the constants
// of the model stamp in LDS, the Keys tap weights of one axis (KeysTaps), the model stamp with its
// apron in LDS and the fp64 one in memory (LdsStamp, GlobalStamp), the 4 x 4 FIR with its derivatives (psf_interp),
// the domain of the shift (psf_inside) and the validity of a pixel (psf_pixel).  See DESIGN.md sections 18 and 19.
// Everything here has internal linkage.
#pragma once
#include "device_common.h"
#include "fit_common.h"

namespace mpsfr {
namespace {

constexpr int kPsfApron = 10;
constexpr int kPsfSide = NS + 2 * kPsfApron;       // 60 rows
constexpr int kPsfStride = 72;                     // elements per row (the last 12 are never read)
constexpr double kPsfMaxShift = 8.0;               // |dp|, |dq| bound
constexpr double kPsfMinWeight = 0x1p-100;         // a used pixel keeps a weight > 0 (relative to the largest one)
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

// the validity of a pixel (obs_pixel of fit_obs.hip)
struct PsfPixel {
    bool used, bad;       // bad: an infinite value under a valid variance (the row gets status 2)
};
__device__ __forceinline__ PsfPixel psf_pixel(double d, double v, bool has_var) {
    const bool vok = !has_var || (v > 0.0 && v < __builtin_inf());       // (NaN fails both)
    const bool fin = fabs(d) < __builtin_inf();
    PsfPixel p;
    p.used = vok && fin;
    p.bad = vok && !fin && d == d;
    return p;
}

}  // namespace
}  // namespace mpsfr
