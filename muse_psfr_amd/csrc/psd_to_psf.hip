// HIP kernels of the public psd_to_psf (psfrec.py:689-807): the full-field PSF of a caller's PSD,
// pupil and static phase.  Everything is fp64 in both precision modes.  See DESIGN.md, "psd_to_psf".
//
// Notation: M = dimnum (transform length), P = npup, N = dim (the PSD grid).  The structure function
// comes from launch_dphi_from_psd (stage_a.hip) as the transposed half plane D0t[y][x], y in [0, N/2].
//
// The reference's chain  sysFTO = fftshift(Dphi2 dlFTO),  PSF = Re fftshift(ifft2(sysFTO)) / sum  is
// evaluated in FFT layout: with sk, sl the signed indices of (k, l) (sk = k - M for k >= M/2),
//   S[k][l] = exp(c_lambda Dphi0[sk][sl]) |A[k][l]| / (M^4 sum(pup)),
//   A = fft2(|fft2(tab)|^2)   (|A| is even, so it equals |fft2(|ifft2(tab)|^2)| M^4 of psfrec.py:788),
//   PSF_u = Re fft2(S)        (S is real and even: Re fft2 = Re ifft2 M^2),
// and PSF[i][j] = PSF_u[(i + M/2) % M][(j + M/2) % M] / (M^2 S[0][0]) -- the sum of a transform over
// every frequency is M^2 times its DC input, so the normalisation needs no reduction pass and does
// not depend on how the planes are batched.
//
// Layouts (all line-major, one line per FFT slot):
//   T1 [P][M]            complex  rows of fft2(tab) after the row pass (only the P rows of the pupil)
//   Q  [M][M/2+1]        complex  Q[b][u] = sum_a |T[a][b]|^2 W^(a u)   (real input: u <= M/2 suffices)
//   OTFt [M/2+1][M]      double   OTFt[v][u] = |A[u][v]| / (M^4 sum(pup))   (even: half plane)
//   G  [M/2+1][M/2+1]    complex  G[l][a] = sum_k S[k][l] W^(k a), l, a in [0, M/2]
#include "device_common.h"

namespace mpsfr {

namespace {

template <int N>
constexpr size_t p2p_smem() { return (size_t)(1 + 2 * LineCfg<N>::SLOTS) * LineCfg<N>::NPAD * sizeof(cx<double>); }

// S[k][l] for l in [0, M/2]: the one expression both kernels of the PSF pair evaluate (same bits)
template <int M>
__device__ __forceinline__ double sys_otf(const double* __restrict__ D0t, int N, const double* __restrict__ otft,
                                          double c, int k, int l) {
    int sk = k < M / 2 ? k : k - M, sl = l < M / 2 ? l : l - M;
    if (sl < 0) { sk = -sk; sl = -sl; }          // l = M/2: Dphi0[sk][-M/2] = Dphi0[-sk][M/2]
    const int x = sk < 0 ? sk + N : sk;
    return exp(c * D0t[(size_t)sl * N + x]) * otft[(size_t)l * M + k];
}

// ------------------------------------------------------------------------------------------
// K_P2P_OTF_ROWS: row pass of the telescope OTF (psfrec.py:784-788).  Line k < P of tab: the pupil
// field pup exp(i 2 pi phase / lambda_m) (zero-padded to M), forward FFT -> T1[z][k][0..M).
// ------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__((LineCfg<M>::THREADS))
k_p2p_otf_rows(int P, const double* __restrict__ pup, const double* __restrict__ phase,
               const double* __restrict__ lbda_m, cx<double>* __restrict__ T1, const cx<double>* __restrict__ twg) {
    using L = LineCfg<M>;
    constexpr int TPR = L::TPR, SLOTS = L::SLOTS, THREADS = L::THREADS, NPAD = L::NPAD, EPT = M / TPR;
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
    cx<double>* bufA = tw + NPAD;
    cx<double>* bufB = bufA + SLOTS * NPAD;
    const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR, z = blockIdx.y;
    const int k = blockIdx.x * SLOTS + slot;
    const bool on = k < P;
    for (int i = threadIdx.x; i < M; i += THREADS) tw[lds_pad(i)] = twg[i];
    const double w = phase ? 2.0 * kPi / lbda_m[z] : 0.0;
    cx<double> x[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int l = t + e * TPR;
        x[e] = {0.0, 0.0};
        if (on && l < P) {
            const double a = pup[(size_t)k * P + l];
            if (phase) {
                double s, co;
                sincos(w * phase[(size_t)k * P + l], &s, &co);
                x[e] = {a * co, a * s};
            } else {
                x[e] = {a, 0.0};
            }
        }
    }
    __syncthreads();
    const cx<double>* res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
    if (on) {
        cx<double>* dst = T1 + ((size_t)z * P + k) * M;
        for (int b = t; b < M; b += TPR) dst[b] = res[lds_out<M, 16>(b)];
    }
}

// ------------------------------------------------------------------------------------------
// K_P2P_OTF_COLS: column b of tab: FFT over the P pupil rows (zero-padded) -> T[.][b], then |T|^2,
// then the first pass of the second transform, over the same index: Q[z][b][u], u in [0, M/2].
// ------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__((LineCfg<M>::THREADS))
k_p2p_otf_cols(int P, const cx<double>* __restrict__ T1, cx<double>* __restrict__ Q, const cx<double>* __restrict__ twg) {
    using L = LineCfg<M>;
    constexpr int TPR = L::TPR, SLOTS = L::SLOTS, THREADS = L::THREADS, NPAD = L::NPAD, EPT = M / TPR, H1 = M / 2 + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
    cx<double>* bufA = tw + NPAD;
    cx<double>* bufB = bufA + SLOTS * NPAD;
    const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR, z = blockIdx.y;
    const int b = blockIdx.x * SLOTS + slot;     // M is a multiple of SLOTS
    for (int i = threadIdx.x; i < M; i += THREADS) tw[lds_pad(i)] = twg[i];
    const cx<double>* src = T1 + (size_t)z * P * M;
    cx<double> x[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int k = t + e * TPR;
        x[e] = k < P ? src[(size_t)k * M + b] : cx<double>{0.0, 0.0};
    }
    __syncthreads();
    const cx<double>* res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const cx<double> v = res[lds_out<M, 16>(t + e * TPR)];
        x[e] = {v.x * v.x + v.y * v.y, 0.0};
    }
    __syncthreads();                             // every slot has read its result before the buffers are reused
    res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
    cx<double>* dst = Q + ((size_t)z * M + b) * H1;
    for (int u = t; u < H1; u += TPR) dst[u] = res[lds_out<M, 16>(u)];
}

// ------------------------------------------------------------------------------------------
// K_P2P_OTF_FIN: line u in [0, M/2] of the second pass: A[u][v] = sum_b Q[b][u] W^(b v), and
// OTFt[v][u] = |A[u][v]| scale for v <= M/2.  |A[M-u][M-v]| = |A[u][v]| (A is the transform of a real
// array), so line u also fills column M - u (0 < u < M/2): every element is written exactly once.
// ------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__((LineCfg<M>::THREADS))
k_p2p_otf_fin(const cx<double>* __restrict__ Q, double scale, double* __restrict__ otft,
              const cx<double>* __restrict__ twg) {
    using L = LineCfg<M>;
    constexpr int TPR = L::TPR, SLOTS = L::SLOTS, THREADS = L::THREADS, NPAD = L::NPAD, EPT = M / TPR, H1 = M / 2 + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
    cx<double>* bufA = tw + NPAD;
    cx<double>* bufB = bufA + SLOTS * NPAD;
    const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR, z = blockIdx.y;
    const int u = blockIdx.x * SLOTS + slot;
    const bool on = u < H1;
    for (int i = threadIdx.x; i < M; i += THREADS) tw[lds_pad(i)] = twg[i];
    const cx<double>* src = Q + (size_t)z * M * H1;
    cx<double> x[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) x[e] = on ? src[(size_t)(t + e * TPR) * H1 + u] : cx<double>{0.0, 0.0};
    __syncthreads();
    const cx<double>* res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
    if (on) {
        double* o = otft + (size_t)z * H1 * M;
        for (int v = t; v < M; v += TPR) {
            const cx<double> a = res[lds_out<M, 16>(v)];
            const double val = sqrt(a.x * a.x + a.y * a.y) * scale;
            if (v < H1) o[(size_t)v * M + u] = val;
            const int vm = (M - v) % M;
            if (u > 0 && u < M / 2 && vm < H1) o[(size_t)vm * M + (M - u)] = val;
        }
    }
}

// ------------------------------------------------------------------------------------------
// K_P2P_PSF_LINES: first pass of the PSF transform, the product formed while the lines load
// (psfrec.py:793-797).  Line l in [0, M/2] (S real and even: the lines l > M/2 are conjugates),
// elements k: G[z][l][a] = sum_k S[k][l] W^(k a), a in [0, M/2].
// otft advances by otf_stride per plane (0: one OTF for every wavelength).
// ------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__((LineCfg<M>::THREADS))
k_p2p_psf_lines(int N, const double* __restrict__ D0t, const double* __restrict__ otft, size_t otf_stride,
                const double* __restrict__ cl, cx<double>* __restrict__ G, const cx<double>* __restrict__ twg) {
    using L = LineCfg<M>;
    constexpr int TPR = L::TPR, SLOTS = L::SLOTS, THREADS = L::THREADS, NPAD = L::NPAD, EPT = M / TPR, H1 = M / 2 + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
    cx<double>* bufA = tw + NPAD;
    cx<double>* bufB = bufA + SLOTS * NPAD;
    const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR, z = blockIdx.y;
    const int l = blockIdx.x * SLOTS + slot;
    const bool on = l < H1;
    for (int i = threadIdx.x; i < M; i += THREADS) tw[lds_pad(i)] = twg[i];
    const double* ot = otft + z * otf_stride;
    const double c = cl[z];
    cx<double> x[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) x[e] = {on ? sys_otf<M>(D0t, N, ot, c, t + e * TPR, l) : 0.0, 0.0};
    __syncthreads();
    const cx<double>* res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
    if (on) {
        cx<double>* dst = G + ((size_t)z * H1 + l) * H1;
        for (int a = t; a < H1; a += TPR) dst[a] = res[lds_out<M, 16>(a)];
    }
}

// ------------------------------------------------------------------------------------------
// K_P2P_PSF_OUT: second pass, line a in [0, M/2] over l (G[l][a] = conj G[M-l][a] for l > M/2):
// PSF_u[a][b] = Re sum_l G[l][a] W^(l b), stored centred and normalised (psfrec.py:797-801) into
// row (a + M/2) % M, and, since PSF_u[M-a][M-b] = PSF_u[a][b], row (M/2 - a) % M for 0 < a < M/2.
// ------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__((LineCfg<M>::THREADS))
k_p2p_psf_out(int N, const double* __restrict__ D0t, const double* __restrict__ otft, size_t otf_stride,
              const double* __restrict__ cl, const cx<double>* __restrict__ G, double* __restrict__ psf,
              const cx<double>* __restrict__ twg) {
    using L = LineCfg<M>;
    constexpr int TPR = L::TPR, SLOTS = L::SLOTS, THREADS = L::THREADS, NPAD = L::NPAD, EPT = M / TPR, H1 = M / 2 + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
    cx<double>* bufA = tw + NPAD;
    cx<double>* bufB = bufA + SLOTS * NPAD;
    const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR, z = blockIdx.y;
    const int a = blockIdx.x * SLOTS + slot;
    const bool on = a < H1;
    for (int i = threadIdx.x; i < M; i += THREADS) tw[lds_pad(i)] = twg[i];
    const cx<double>* src = G + (size_t)z * H1 * H1;
    cx<double> x[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int l = t + e * TPR;
        cx<double> v = {0.0, 0.0};
        if (on) {
            if (l < H1) {
                v = src[(size_t)l * H1 + a];
            } else {
                v = src[(size_t)(M - l) * H1 + a];
                v.y = -v.y;
            }
        }
        x[e] = v;
    }
    // sum of PSF_u over the plane = M^2 S[0][0]
    const double inv = 1.0 / ((double)M * (double)M * sys_otf<M>(D0t, N, otft + z * otf_stride, cl[z], 0, 0));
    __syncthreads();
    const cx<double>* res = fft_forward_regs<double, M, false>(x, bufA + slot * NPAD, bufB + slot * NPAD, tw, t);
    if (on) {
        double* o = psf + (size_t)z * M * M;
        double* r0 = o + (size_t)((a + M / 2) % M) * M;
        double* r1 = o + (size_t)((M / 2 - a + M) % M) * M;
        const bool mirror = a > 0 && a < M / 2;
        for (int b = t; b < M; b += TPR) {
            const double v = res[lds_out<M, 16>(b)].x * inv;
            r0[(b + M / 2) % M] = v;
            if (mirror) r1[(M / 2 - b + M) % M] = v;
        }
    }
}

}  // namespace

bool p2p_supported(int M) { return M == 128 || M == 256 || M == 512 || M == 1024 || M == 1280; }

void launch_p2p_otf(hipStream_t s, int M, int P, int nz, const double* d_pup, const double* d_phase,
                    const double* d_lbda_m, double scale, void* d_T1, void* d_Q, double* d_otft, const void* d_twm) {
    DISPATCH_N(M, {
        constexpr size_t sm = p2p_smem<NN>();
        constexpr int SL = LineCfg<NN>::SLOTS;
        constexpr int TH = LineCfg<NN>::THREADS;
        allow_smem((k_p2p_otf_rows<NN>), sm);
        allow_smem((k_p2p_otf_cols<NN>), sm);
        allow_smem((k_p2p_otf_fin<NN>), sm);
        hipLaunchKernelGGL((k_p2p_otf_rows<NN>), dim3((P + SL - 1) / SL, nz), dim3(TH), sm, s, P, d_pup, d_phase,
                           d_lbda_m, (cx<double>*)d_T1, (const cx<double>*)d_twm);
        hipLaunchKernelGGL((k_p2p_otf_cols<NN>), dim3(NN / SL, nz), dim3(TH), sm, s, P, (const cx<double>*)d_T1,
                           (cx<double>*)d_Q, (const cx<double>*)d_twm);
        hipLaunchKernelGGL((k_p2p_otf_fin<NN>), dim3((NN / 2 + 1 + SL - 1) / SL, nz), dim3(TH), sm, s,
                           (const cx<double>*)d_Q, scale, d_otft, (const cx<double>*)d_twm);
    })
}

void launch_p2p_psf(hipStream_t s, int M, int N, int nz, const double* d_D0t, const double* d_otft, size_t otf_stride,
                    const double* d_cl, void* d_G, double* d_psf, const void* d_twm) {
    DISPATCH_N(M, {
        constexpr size_t sm = p2p_smem<NN>();
        constexpr int SL = LineCfg<NN>::SLOTS;
        constexpr int TH = LineCfg<NN>::THREADS;
        const dim3 grid((NN / 2 + 1 + SL - 1) / SL, nz);
        allow_smem((k_p2p_psf_lines<NN>), sm);
        allow_smem((k_p2p_psf_out<NN>), sm);
        hipLaunchKernelGGL((k_p2p_psf_lines<NN>), grid, dim3(TH), sm, s, N, d_D0t, d_otft, otf_stride, d_cl,
                           (cx<double>*)d_G, (const cx<double>*)d_twm);
        hipLaunchKernelGGL((k_p2p_psf_out<NN>), grid, dim3(TH), sm, s, N, d_D0t, d_otft, otf_stride, d_cl,
                           (const cx<double>*)d_G, d_psf, (const cx<double>*)d_twm);
    })
}

}  // namespace mpsfr
