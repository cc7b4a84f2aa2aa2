// HIP kernel of the band-integrated PSFs (mpsfr_reconstruct_band), written for gfx950 (MI355X, wave64).  See DESIGN.md
// section 14.
//
// K_BAND_REDUCE: the final stamps of one chunk S [tb][nl][40][40] (float in mixed mode, double in f64 mode) reduced
// over wavelength with the normalised weights of up to MPSFR_MAX_BANDS bands:
//     out[g][b][p] = sum_l w[b][l] S[g][l][p]        (fp64, one FMA chain per (g, b, p) in wavelength order)
// No atomics and no split over wavelengths: the result does not depend on the chunking, and a band that holds one
// wavelength at weight 1 is that stamp exactly (1 x S + 0; the zero weights add exact zeros).
// Memory-bound: S is read once, whole 40 x 40 planes by consecutive lanes.  A workgroup is 320 threads (five waves),
// one pixel each, and five workgroups cover a stamp group, so no lane idles.  A thread keeps NB accumulators in
// registers and eight planes of loads in flight (as k_stamp_sum keeps eight tasks).  The weights are wave-uniform
// ([nl][NB], zero beyond nband): they come through the scalar cache.
#include "kernels.h"

namespace mpsfr {

namespace {

constexpr int kBandThreads = 320;
constexpr int kBandPlane = NS * NS;                 // 1600 = 5 x 320
static_assert(kBandPlane % kBandThreads == 0, "whole workgroups per stamp");
constexpr int kBandInFlight = 8;

template <typename TF, int NB>
__global__ void __launch_bounds__(kBandThreads) k_band_reduce(int nl, int nband, const TF* __restrict__ fin,
                                                              const double* __restrict__ w, double* __restrict__ out) {
    const int g = blockIdx.y;
    const int p = blockIdx.x * kBandThreads + threadIdx.x;
    const TF* src = fin + (size_t)g * nl * kBandPlane + p;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    int l = 0;
    for (; l + kBandInFlight <= nl; l += kBandInFlight) {
        TF v[kBandInFlight];
#pragma unroll
        for (int k = 0; k < kBandInFlight; ++k) v[k] = src[(size_t)(l + k) * kBandPlane];
#pragma unroll
        for (int k = 0; k < kBandInFlight; ++k) {
            const double x = (double)v[k];
            const double* wl = w + (size_t)(l + k) * NB;
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_fma(wl[b], x, acc[b]);
        }
    }
    for (; l < nl; ++l) {
        const double x = (double)src[(size_t)l * kBandPlane];
        const double* wl = w + (size_t)l * NB;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_fma(wl[b], x, acc[b]);
    }
    double* dst = out + (size_t)g * nband * kBandPlane + p;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b < nband) dst[(size_t)b * kBandPlane] = acc[b];
}

template <typename TF, int NB>
void launch_nb(hipStream_t s, int ntb, int nl, int nband, const void* d_fin, const double* d_w, double* d_out) {
    const dim3 grid(kBandPlane / kBandThreads, ntb);
    hipLaunchKernelGGL((k_band_reduce<TF, NB>), grid, dim3(kBandThreads), 0, s, nl, nband, (const TF*)d_fin, d_w,
                       d_out);
}

template <typename TF>
void launch_tf(hipStream_t s, int ntb, int nl, int nband, const void* d_fin, const double* d_w, double* d_out) {
    switch (band_stride(nband)) {
    case 1: launch_nb<TF, 1>(s, ntb, nl, nband, d_fin, d_w, d_out); break;
    case 2: launch_nb<TF, 2>(s, ntb, nl, nband, d_fin, d_w, d_out); break;
    case 4: launch_nb<TF, 4>(s, ntb, nl, nband, d_fin, d_w, d_out); break;
    case 8: launch_nb<TF, 8>(s, ntb, nl, nband, d_fin, d_w, d_out); break;
    default: launch_nb<TF, 16>(s, ntb, nl, nband, d_fin, d_w, d_out); break;
    }
}

}  // namespace

int band_stride(int nband) {
    int nb = 1;
    while (nb < nband) nb *= 2;
    return nb;
}

void launch_band_reduce(hipStream_t s, int ntb, int nl, int nband, const void* d_fin, bool fin_f32,
                        const double* d_w, double* d_out) {
    if (ntb <= 0 || nband <= 0 || nband > MAX_BANDS) return;
    if (fin_f32) launch_tf<float>(s, ntb, nl, nband, d_fin, d_w, d_out);
    else launch_tf<double>(s, ntb, nl, nband, d_fin, d_w, d_out);
}

}  // namespace mpsfr
