// Crowded-field PSF photometry (mpsfr_fit_frame_psf, include/mpsfr.h): the fluxes of all stars of
// a frame, and one constant, as one weighted linear least-squares problem, solved by Jacobi-preconditioned conjugate
// gradients on the normal equations without ever forming them.  A x is the renderer's tile walk (render.hip) over lists
// built once per solve; what is new here:
//   k_ff_star<false>  one workgroup per star: judges it (FrameStar's rule and footprint, which are the renderer's; the
//                     valid pixels of its own disc, sum w P~^2 over them) and takes sum P of its model
//   k_ff_domain       one workgroup per frame tile: W = w [pixel in Omega], Omega the valid pixels in the disc of an
//                     accepted star, from the tile's star list
//   k_ff_star<true>   the projection, one workgroup per accepted star: g_k = sum W P~_k (V + c) over its footprint and,
//                     in the first pass, N_kk = sum W P~_k^2 -- the model stamp with the rows and columns its taps
//                     reach staged once in LDS, every thread a fixed set of footprint pixels, a fixed tree
//   k_ff_reduce       sum W (V + c), sum W, sum W (V + c)^2 and |Omega| over chunks of the frame, one partial per chunk
//   k_ff_step<phase>  one workgroup: the conjugate-gradient step over the unknowns, the stop test and the done word; the
//                     first residual; the rows of the result
// What the step kernels of the whole family (k_ff_step; k_fr_step, frame_free.hip; k_cf_step, cube_free.hip) have in
// common stands here once: block_reduce (block_sum, block_max), the conjugate-gradient step over a flat vector (cg_step)
// with its per-place updates (cg_advance, cg_direct) and its end (cg_alpha, cg_end, cg_beta), columns 0 to 7 of a star's
// row (star_row) and columns 0 to 6 of a head (solve_head).  What only the fits with free positions share is in
// frame_free_impl.h.
// Every sum has a fixed order (no floating-point atomics), all arithmetic is fp64, and nothing waits for the host: the
// scalars live in the work buffer, and once the done word is set the queued kernels of the later iterations return.
//
// Every kernel and the driver have a second form, LAYERS = true, for the layers of a cube (DESIGN.md section 25;
// mpsfr_fit_cube_psf; instantiated in cube_fit.hip): the layers of a batch are one more grid dimension, every array of
// the workspace and of the call holds the layers one behind the other at its own length (a frame ny nx, a vector of
// the unknowns nstar + 1, a per-star array nstar, the partials 4 chunks, the scalars), the lists hold every placed
// star, sorted once, and accept [layers][nstar] says which of them a layer sums.  The arithmetic of a layer, and the
// order of every sum, is that of the frame: the same code.  This header is the whole of both; frame_fit.hip and
// cube_fit.hip instantiate it.
#pragma once
#include <type_traits>

#include "frame_common.h"

namespace mpsfr {
namespace {

constexpr int kStarThreads = 256;
constexpr int kFootPix = kPsfSide * kPsfSide;                              // 3600 footprint pixels
constexpr int kFootShare = (kFootPix + kStarThreads - 1) / kStarThreads;    // per thread: e = tid + 256 m
constexpr int kFootBatch = 5;                                               // of them loaded at once (3, 15: slower)
static_assert(kFootShare % kFootBatch == 0, "whole batches");
constexpr int kFootSide = kPsfSide + 3;                                     // model rows / columns a footprint's taps touch
constexpr int kFootStride = kFootSide + 1;
constexpr int kChunk = 4096;                                                // frame pixels per partial of k_ff_reduce
constexpr int kStepThreads = 1024;
constexpr int kTile = kFrameTile;                                            // k_ff_domain walks the renderer's lists
constexpr int NROW = 8;                                                     // MPSFR_NFRAMEFIT

// the scalars of a solve: doubles, then ints
enum { S_RHO = 0, S_RHO0, S_REL, S_WSUM, S_NDOUBLE };
enum { I_DONE = 0, I_ITER, I_STATUS, I_NACC, I_NOMEGA, I_NINT };

// op over the v of the workgroup's T threads in a fixed tree -- the wave's ladder (wave_sum's: v = op(v, the lane 32,
// 16, ... 1 away)), then the waves in order from wave 0 --; every thread gets it.  `part`: T / 64 doubles of LDS, free
// again on return.  The tree, and the two barriers, are part of every result of this family: they do not change.
template <int T, class Op>
__device__ __forceinline__ double block_reduce(double v, double* part, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) s = op(s, part[w]);
    return s;
}
template <int T>
__device__ __forceinline__ double block_sum(double v, double* part) {
    return block_reduce<T>(v, part, [](double a, double b) { return a + b; });
}
template <int T>
__device__ __forceinline__ double block_max(double v, double* part) {
    return block_reduce<T>(v, part, [](double a, double b) { return fmax(a, b); });
}

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

// is the frame pixel (Y, X) in the disc of the star centred on (cy, cx)?  Each product rounded, then the sum.
__device__ __forceinline__ bool in_disc(int Y, int X, double cy, double cx, double r2) {
#pragma clang fp contract(off)
    const double dy = (double)Y - cy, dx = (double)X - cx;
    const double a = dy * dy, b = dx * dx;
    return a + b <= r2;
}

// What k_ff_star<false> reads beside the stars and writes: the verdict on every star, the sum over its own disc (diag)
// and its start (x)
struct StarJudging {
    const double *image, *var, *scale0;
    int32_t *accept, *stat;
    double *ndisc, *sump, *diag, *x;
    __device__ __forceinline__ void layer(int b, size_t npix, int nstar) {
        image += b * npix;
        if (var) var += b * npix;
        if (scale0) scale0 += (size_t)b * nstar;
        accept += (size_t)b * nstar;
        stat += (size_t)b * nstar;
        ndisc += (size_t)b * nstar;
        sump += (size_t)b * nstar;
        diag += (size_t)b * (nstar + 1);
        x += (size_t)b * (nstar + 1);
    }
};
// What k_ff_star<true> reads and writes: g[k] = sum W P~ (V + c) (c: nullptr for 0) and, with diag, diag[k] = sum W P~^2
// for an accepted star; nothing once *done is set
struct StarProjection {
    const double *W, *V, *c;
    const int32_t *accept, *done;
    double *g, *diag;
    __device__ __forceinline__ void layer(int b, size_t npix, int nstar) {
        W += b * npix;
        V += b * npix;
        if (c) c += (size_t)b * (nstar + 1);
        accept += (size_t)b * nstar;
        if (done) done += (size_t)b * I_NINT;
        g += (size_t)b * (nstar + 1);
        if (diag) diag += (size_t)b * (nstar + 1);
    }
};

// PROJECT = false: the star is judged.  PROJECT = true: the projection on an accepted star.  LAYERS: of layer blockIdx.y.
template <bool PROJECT, bool LAYERS>
__global__ __launch_bounds__(kStarThreads) void k_ff_star(
    int ny, int nx, StarList stars, double r2, std::conditional_t<PROJECT, StarProjection, StarJudging> io) {
    __shared__ double stage[kFootSide * kFootStride];
    __shared__ double part[kStarThreads / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    if constexpr (LAYERS) {
        io.layer(blockIdx.y, (size_t)ny * nx, stars.nstar);
        stars.layer = blockIdx.y;
    }
    if constexpr (PROJECT) {
        if ((io.done && *io.done) || !io.accept[k]) return;
    }
    const FrameStar star(stars, k);
    const int op = star.op, oq = star.oq;
    if constexpr (!PROJECT) {
        int y0, y1, x0, x1;
        const bool ok = star.valid(stars.npsf);
        const bool hit = ok && star.footprint(ny, nx, y0, y1, x0, x1);
        if (!hit) {                                   // (the same for all threads)
            if (tid == 0) {
                io.accept[k] = 0;
                io.stat[k] = ok ? 1 : 2;
                io.ndisc[k] = 0.0;
                io.sump[k] = 0.0;
                io.diag[k] = 0.0;
                io.x[k] = 0.0;
            }
            return;
        }
    }
    const double* P = star.model(stars);
    const KeysTaps<double> ty(star.dp), tx(star.dq);
    // stage[i][j] = model pixel (ty.f - 11 + i, tx.f - 11 + j): the taps of footprint pixel (p, q) = (pr - 10, qc - 10)
    // are the model rows p + f - 1 + a, that is the stage rows pr + a
    const int r0 = ty.f - 1 - kPsfApron, c0 = tx.f - 1 - kPsfApron;
    double ps = 0.0;
    for (int e = tid; e < kFootSide * kFootSide; e += kStarThreads) {
        const int i = e / kFootSide, j = e - i * kFootSide;
        stage[i * kFootStride + j] = model_pixel(P, r0 + i, c0 + j);
    }
    if constexpr (!PROJECT)
        for (int e = tid; e < NS * NS; e += kStarThreads) ps += P[e];
    __syncthreads();
    const StagedStamp<kFootStride> st{stage};
    const double cy = star.cy(), cx = star.cx();
    double cval = 0.0;
    if constexpr (PROJECT) cval = io.c ? *io.c : 0.0;
    double sg = 0.0, sn = 0.0;
    int cnt = 0;
    // the thread's pixels of the two frames a batch at a time, the loads of a batch in flight together, then its
    // arithmetic: a workgroup is short, and what it waits for is memory
#pragma unroll 1
    for (int m0 = 0; m0 < kFootShare; m0 += kFootBatch) {
        double fa[kFootBatch], fb[kFootBatch];        // W and V; or the variance and the datum
#pragma unroll
        for (int j = 0; j < kFootBatch; ++j) {
            const int e = tid + (m0 + j) * kStarThreads, pr = e / kPsfSide, qc = e - pr * kPsfSide;
            const int Y = op - kPsfApron + pr, X = oq - kPsfApron + qc;
            const bool on = e < kFootPix && Y >= 0 && Y < ny && X >= 0 && X < nx;
            const size_t src = on ? (size_t)Y * nx + (size_t)X : 0;
            if constexpr (PROJECT) {
                fa[j] = io.W[src];
                fb[j] = io.V[src];
            } else {
                fa[j] = io.var ? io.var[src] : 1.0;
                fb[j] = io.image[src];
            }
        }
#pragma unroll
        for (int j = 0; j < kFootBatch; ++j) {
            const int e = tid + (m0 + j) * kStarThreads, pr = e / kPsfSide, qc = e - pr * kPsfSide;
            const int Y = op - kPsfApron + pr, X = oq - kPsfApron + qc;
            const bool on = e < kFootPix && Y >= 0 && Y < ny && X >= 0 && X < nx;
            double w, v = 0.0;
            bool use;
            if constexpr (PROJECT) {
                w = fa[j];
                v = fb[j];
                use = on && w > 0.0;              // (W is 0 outside Omega; a masked datum may be NaN: selected out)
            } else {
                use = on && fit_pixel(fb[j], fa[j], io.var != nullptr).used && in_disc(Y, X, cy, cx, r2);
                w = 1.0 / fa[j];
            }
            if (use) {
                double val, gy, gx;
                psf_interp<double, false>(st, pr * kFootStride + qc, 0, 0, ty, tx, val, gy, gx);
                const double wv = w * val;
                sn += wv * val;
                if constexpr (PROJECT) sg += wv * (v + cval);
                ++cnt;
            }
        }
    }
    if constexpr (PROJECT) {
        const double tg = block_sum<kStarThreads>(sg, part);
        if (tid == 0) io.g[k] = tg;
        if (io.diag) {
            const double tn = block_sum<kStarThreads>(sn, part);
            if (tid == 0) io.diag[k] = tn;
        }
    } else {
        const double tn = block_sum<kStarThreads>(sn, part);
        const double tc = block_sum<kStarThreads>((double)cnt, part);
        const double tp = block_sum<kStarThreads>(ps, part);
        if (tid == 0) {
            const bool acc = tc > 0.0 && tn > 0.0 && tn < __builtin_inf();
            const double s0 = io.scale0 ? io.scale0[k] : 0.0;
            io.accept[k] = acc ? 1 : 0;
            io.stat[k] = acc ? 0 : 2;
            io.ndisc[k] = tc;
            io.sump[k] = tp;
            io.diag[k] = tn;
            io.x[k] = acc && fabs(s0) < __builtin_inf() ? s0 : 0.0;
        }
    }
}

// W of one frame tile from its star list: the centres of up to 256 stars at a time in LDS.  LAYERS: of layer
// blockIdx.z, whose accept [nstar] marks the stars of the list that count (the centre of any other is NaN: in no disc).
template <bool LAYERS>
__global__ __launch_bounds__(256) void k_ff_domain(int ny, int nx, const double* __restrict__ image,
                                                  const double* __restrict__ var, StarList stars, double r2,
                                                  const int* __restrict__ offset, const int* __restrict__ pairs,
                                                  const int32_t* __restrict__ accept, double* __restrict__ W) {
    __shared__ double scy[256], scx[256];
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly0 = tid / kTile;
    if constexpr (LAYERS) {
        const size_t o = (size_t)blockIdx.z * ny * nx;
        image += o;
        if (var) var += o;
        W += o;
        accept += (size_t)blockIdx.z * stars.nstar;
        stars.layer = blockIdx.z;
    }
    const int t = blockIdx.y * gridDim.x + blockIdx.x;
    const int Y0 = blockIdx.y * kTile, X = blockIdx.x * kTile + lx;
    const int first = offset[t], n = offset[t + 1] - first;
    bool in[4] = {false, false, false, false};
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if (tid < m) {
            const int k = pairs[first + base + tid];
            const FrameStar star(stars, k);
            bool counts = true;
            if constexpr (LAYERS) counts = accept[k] != 0;
            scy[tid] = counts ? star.cy() : __builtin_nan("");
            scx[tid] = star.cx();
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double cy = scy[i], cx = scx[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) in[j] = in[j] || in_disc(Y0 + ly0 + 8 * j, X, cy, cx, r2);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int Y = Y0 + ly0 + 8 * j;
        if (Y < ny && X < nx) {
            const size_t o = (size_t)Y * nx + X;
            const double vv = var ? var[o] : 1.0;
            const bool use = in[j] && fit_pixel(image[o], vv, var != nullptr).used;
            W[o] = use ? 1.0 / vv : 0.0;
        }
    }
}

// partial sums over chunk blockIdx.x of the frame: part[0][c] = sum W (V + csign c), [1] sum W, [2] sum W (V + ..)^2,
// [3] the pixels with W > 0.  LAYERS: of layer blockIdx.y; cptr at a pitch of cpitch.
template <bool LAYERS>
__global__ __launch_bounds__(256) void k_ff_reduce(size_t npix, int nchunk, const double* __restrict__ W,
                                                  const double* __restrict__ V, const double* __restrict__ cptr,
                                                  int cpitch, double csign, double* __restrict__ partial,
                                                  const int32_t* __restrict__ done) {
    __shared__ double part[256 / 64];
    if constexpr (LAYERS) {
        const int b = blockIdx.y;
        W += b * npix;
        V += b * npix;
        if (cptr) cptr += (size_t)b * cpitch;
        partial += (size_t)b * 4 * nchunk;
        if (done) done += (size_t)b * I_NINT;
    }
    if (done && *done) return;
    const int tid = threadIdx.x, c = blockIdx.x;
    const double cval = cptr ? csign * *cptr : 0.0;
    double s1 = 0.0, s0 = 0.0, s2 = 0.0, cnt = 0.0;
#pragma unroll 4
    for (int j = 0; j < kChunk / 256; ++j) {
        const size_t o = (size_t)c * kChunk + (size_t)j * 256 + tid;
        const double w = o < npix ? W[o] : 0.0;
        if (w > 0.0) {
            const double v = V[o] + cval, wv = w * v;
            s1 += wv;
            s0 += w;
            s2 += wv * v;
            cnt += 1.0;
        }
    }
    s1 = block_sum<256>(s1, part);
    s0 = block_sum<256>(s0, part);
    s2 = block_sum<256>(s2, part);
    cnt = block_sum<256>(cnt, part);
    if (tid == 0) {
        partial[c] = s1;
        partial[nchunk + c] = s0;
        partial[2 * (size_t)nchunk + c] = s2;
        partial[3 * (size_t)nchunk + c] = cnt;
    }
}

// the sum of a[0 .. n - 1] by the step kernel's workgroup: thread t takes t, t + 1024, ... in order, then the tree
__device__ __forceinline__ double step_sum(const double* __restrict__ a, int n, double* part) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kStepThreads) s += a[i];
    return block_sum<kStepThreads>(s, part);
}

// The pieces below are the step kernels' of all four fits (k_ff_step here, k_fr_step of frame_free.hip, k_cf_step of
// cube_free.hip).  What fixes the bits of those calls, and so holds for every change here: thread t of the step
// workgroup takes the places t, t + 1024, ... in order (lane j of a layer's wave in k_cf_step: j, j + 64, ...); the
// number and the order of the reductions of a phase stay; every expression keeps its shape down to the parentheses --
// ri * (ri / d) is not (ri * ri) / d, and the build contracts a product and a sum into one rounding wherever they
// stand next to each other, so a term that is split or re-associated rounds differently.

// One place of a conjugate-gradient step: x += alpha p, r -= alpha q; returns the place's term of rho1 = r . (r / diag)
__device__ __forceinline__ double cg_advance(double alpha, double qi, double* x, double* r, const double* p,
                                             const double* diag, size_t at) {
    x[at] += alpha * p[at];
    const double ri = r[at] - alpha * qi;
    r[at] = ri;
    return ri * (ri / diag[at]);
}
// ... and its new direction, p = r / diag + beta p
__device__ __forceinline__ void cg_direct(double beta, const double* r, const double* diag, double* p, size_t at) {
    p[at] = r[at] / diag[at] + beta * p[at];
}

struct CgEnd {
    double rho1;       // r . (r / diag) after the step
    bool stop, end;    // the stop test has passed; the solve ends (stop, or N singular along p, or rho1 not finite)
};
// How a step ends: from p . q whether it is taken at all (not so: N is singular along p, the solve ends), from rho1 the
// stop test against tol2 `ref`
__device__ __forceinline__ double cg_alpha(double rho, double pq) { return positive_finite(pq) ? rho / pq : 0.0; }
__device__ __forceinline__ CgEnd cg_end(double rho1, double pq, double tol2, double ref) {
    const bool stop = rho1 <= tol2 * ref;
    return {rho1, stop, stop || !positive_finite(pq) || !(rho1 < __builtin_inf())};
}
__device__ __forceinline__ double cg_beta(const CgEnd& e, double rho) { return e.end ? 0.0 : e.rho1 / rho; }

// One conjugate-gradient step of the step workgroup over the flat vectors x, r, p, q, diag [nu] from q = N p, on the
// places live(i) says.  With `back` the last place is the constant, whose q is the sum of the partials [nchunk] of
// k_ff_reduce.  rho = r . z before the step; the stop test is rho1 <= tol2 ref.  Three reductions in this order: the
// constant's q, p . q, rho1.
template <class Live>
__device__ __forceinline__ CgEnd cg_step(int nu, bool back, Live live, double* x, double* r, double* p, double* q,
                                         const double* diag, const double* partial, int nchunk, double rho, double ref,
                                         double tol2, double* part) {
    const int tid = threadIdx.x;
    if (back) {
        const double qb = step_sum(partial, nchunk, part);
        if (tid == 0) q[nu - 1] = qb;
        __syncthreads();
    }
    double s = 0.0;
    for (int i = tid; i < nu; i += kStepThreads)
        if (live(i)) s += p[i] * q[i];
    const double pq = block_sum<kStepThreads>(s, part);
    const double alpha = cg_alpha(rho, pq);
    double rz = 0.0;
    for (int i = tid; i < nu; i += kStepThreads)
        if (live(i)) rz += cg_advance(alpha, q[i], x, r, p, diag, i);
    const CgEnd e = cg_end(block_sum<kStepThreads>(rz, part), pq, tol2, ref);
    const double beta = cg_beta(e, rho);
    for (int i = tid; i < nu; i += kStepThreads)
        if (live(i)) cg_direct(beta, r, diag, p, i);
    return e;
}

// Columns 0 to 7 of a star's row (MPSFR_NFRAMEFIT; the first eight of the free fits' rows) from its places of the
// closing solve: x, diag, q = (N 1)_k.  `on`: the star was fitted.  Returns F.
__device__ __forceinline__ double star_row(double* o, bool on, double x, double diag, double q, double s2, double sump,
                                           double ndisc, int stat) {
    const double F = on ? x : 0.0, nkk = on ? diag : 0.0;
    const double eF = on ? sqrt(s2 / nkk) : 0.0;
    o[0] = F;
    o[1] = eF;
    o[2] = on ? F * sump : 0.0;
    o[3] = on ? eF * fabs(sump) : 0.0;
    o[4] = on ? (q - nkk) / nkk : 0.0;
    o[5] = on ? ndisc : 0.0;
    o[6] = nkk;
    o[7] = on ? 0.0 : (stat == 1 ? 1.0 : 2.0);
    return F;
}
// Columns 0 to 6 of the head of a solve.  `none`: nothing was fitted; b: the constant's place of x.
__device__ __forceinline__ void solve_head(double* h, bool back, bool none, double b, double s2, double wsum,
                                           double chi2, double nomega, double iter, double rel, double nacc) {
    const bool on = back && !none;
    h[0] = on ? b : 0.0;
    h[1] = on ? sqrt(s2 / wsum) : 0.0;
    h[2] = none ? 0.0 : chi2;
    h[3] = nomega;
    h[4] = iter;
    h[5] = none ? 0.0 : rel;
    h[6] = nacc;
}

enum { STEP_INIT = 0, STEP_ITER = 1, STEP_FINAL = 2 };

// One workgroup over the nu = nstar + 1 unknowns (the constant last; it takes part with `back` only).  x, r, p, q, diag:
// [nu].  STEP_INIT: the first residual from q (the projection of the data minus the start) and the partials.  STEP_ITER:
// one conjugate-gradient step from q = N p.  STEP_FINAL: the rows, from q = N 1 and the partials of the residual frame.
// LAYERS: one workgroup per layer, blockIdx.x.
template <int PHASE, bool LAYERS>
__global__ __launch_bounds__(kStepThreads) void k_ff_step(int nstar, int back, int nchunk, double tol2,
                                                         const int32_t* __restrict__ accept,
                                                         const int32_t* __restrict__ stat,
                                                         const double* __restrict__ ndisc,
                                                         const double* __restrict__ sump, double* __restrict__ x,
                                                         double* __restrict__ r, double* __restrict__ p,
                                                         double* __restrict__ q, double* __restrict__ diag,
                                                         const double* __restrict__ partial, double* __restrict__ sd,
                                                         int32_t* __restrict__ si, double* __restrict__ star_out,
                                                         double* __restrict__ head_out) {
    __shared__ double part[kStepThreads / 64];
    const int tid = threadIdx.x;
    const int nu = nstar + (back ? 1 : 0);
    if constexpr (LAYERS) {
        const size_t b = blockIdx.x, ov = b * ((size_t)nstar + 1), os = b * (size_t)nstar;
        accept += os, stat += os, ndisc += os, sump += os;
        x += ov, r += ov, p += ov, q += ov, diag += ov;
        partial += b * 4 * nchunk;
        sd += b * S_NDOUBLE;
        si += b * I_NINT;
        star_out += b * NROW * nstar;
        head_out += b * NROW;
    }
    // (an unknown that takes part: an accepted star, or the constant)
    auto live = [&](int i) { return i >= nstar || accept[i] != 0; };
    if constexpr (PHASE == STEP_INIT) {
        const double gb = step_sum(partial, nchunk, part);
        const double wsum = step_sum(partial + nchunk, nchunk, part);
        const double nomega = step_sum(partial + 3 * (size_t)nchunk, nchunk, part);
        double na = 0.0;
        for (int i = tid; i < nstar; i += kStepThreads) na += accept[i] ? 1.0 : 0.0;
        const double nacc = block_sum<kStepThreads>(na, part);
        const bool none = nacc < 1.0 || nomega < nacc + (back ? 1.0 : 0.0) + 1.0;
        double rz = 0.0;
        for (int i = tid; i <= nstar; i += kStepThreads) {
            if (i == nstar) {
                diag[i] = wsum;
                x[i] = 0.0;
            }
            const bool on = !none && i < nu && live(i);
            const double ri = on ? (i == nstar ? gb : q[i]) : 0.0;
            const double zi = on ? ri / diag[i] : 0.0;
            if (none) x[i] = 0.0;
            r[i] = ri;
            p[i] = zi;
            rz += ri * zi;
        }
        const double rho = block_sum<kStepThreads>(rz, part);
        if (tid == 0) {
            const bool more = !none && rho > 0.0 && rho < __builtin_inf();
            sd[S_RHO] = rho;
            sd[S_RHO0] = rho;
            sd[S_REL] = more ? 1.0 : 0.0;
            sd[S_WSUM] = wsum;
            si[I_DONE] = more ? 0 : 1;
            si[I_ITER] = 0;
            si[I_STATUS] = none ? 2 : (rho == 0.0 ? 0 : 1);  // 1 until the stop test passes
            si[I_NACC] = (int)nacc;
            si[I_NOMEGA] = (int)nomega;
        }
    } else if constexpr (PHASE == STEP_ITER) {
        if (si[I_DONE]) return;
        const double rho0 = sd[S_RHO0];
        const CgEnd e = cg_step(nu, back != 0, live, x, r, p, q, diag, partial, nchunk, sd[S_RHO], rho0, tol2, part);
        if (tid == 0) {
            sd[S_RHO] = e.rho1;
            sd[S_REL] = sqrt(e.rho1 / rho0);
            si[I_ITER] += 1;
            if (e.end) si[I_DONE] = 1;
            if (e.stop) si[I_STATUS] = 0;
        }
    } else {
        const int status = si[I_STATUS], nacc = si[I_NACC], nomega = si[I_NOMEGA];
        const bool none = status == 2;
        const double chi2 = step_sum(partial + 2 * (size_t)nchunk, nchunk, part);
        const double dof = (double)nomega - (double)nacc - (back ? 1.0 : 0.0);
        const double s2 = none ? 0.0 : chi2 / dof;
        for (int k = tid; k < nstar; k += kStepThreads)
            star_row(star_out + (size_t)NROW * k, !none && accept[k] != 0, x[k], diag[k], q[k], s2, sump[k], ndisc[k],
                     stat[k]);
        if (tid == 0) {
            solve_head(head_out, back != 0, none, x[nstar], s2, sd[S_WSUM], chi2, (double)nomega, (double)si[I_ITER],
                       sd[S_REL], (double)nacc);
            head_out[7] = (double)status;
        }
    }
}

// p[k] = 1 for every star (the renderer reads the accepted ones): the scales of the overlap's render
__global__ __launch_bounds__(256) void k_ff_ones(int n, double* __restrict__ p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 1.0;
}

// The workspace of a solve: the renderer's lists (at its start: launch_render_lists and the walks take d_ws); then, each
// for all the layers of the batch (1 for a frame), the frames W and M; x, r, p, q, diag [nstar + 1], ndisc, sump
// [nstar]; the partials [4][chunks]; the scalars; accept, stat [nstar]
struct FrameFitWork {
    RenderLists lists;
    size_t npix, nu, nb;
    int nchunk;
    double *W, *M, *x, *r, *p, *q, *diag, *ndisc, *sump, *partial, *sd;
    int32_t *si, *accept, *stat;
    FrameFitWork(WorkspaceCarver& ws, int ny, int nx, int nstar, int layers = 1)
        : lists(ws, ny, nx, nstar), npix((size_t)ny * nx), nu((size_t)nstar + 1), nb((size_t)layers),
          nchunk((int)((npix + kChunk - 1) / kChunk)), W(ws.take<double>(nb * npix)), M(ws.take<double>(nb * npix)),
          x(ws.take<double>(nb * nu)), r(ws.take<double>(nb * nu)), p(ws.take<double>(nb * nu)),
          q(ws.take<double>(nb * nu)), diag(ws.take<double>(nb * nu)), ndisc(ws.take<double>(nb * nstar)),
          sump(ws.take<double>(nb * nstar)), partial(ws.take<double>(nb * 4 * (size_t)nchunk)),
          sd(ws.take<double>(nb * S_NDOUBLE)), si(ws.take<int32_t>(nb * I_NINT)), accept(ws.take<int32_t>(nb * nstar)),
          stat(ws.take<int32_t>(nb * nstar)) {}
};

// The solve of a frame (LAYERS = false, layers = 1) or of `layers` layers side by side: d_image, d_var, d_resid_out
// [layers][ny][nx], d_scale0 [layers][nstar], d_star_out [layers][nstar][8], d_head_out [layers][8]; layer b of `stars`
// is its layer b (StarList::layer).  Everything is queued on s; nothing waits.
template <bool LAYERS>
void fit_layers(hipStream_t s, int ny, int nx, int layers, const double* d_image, const double* d_var, StarList stars,
                const double* d_scale0, double radius, bool background, int max_iter, double tol, double* d_star_out,
                double* d_head_out, double* d_resid_out, void* d_ws) {
    WorkspaceCarver ws(d_ws);
    const FrameFitWork w(ws, ny, nx, stars.nstar, layers);
    const int nstar = stars.nstar, back = background ? 1 : 0, nu = nstar + 1;
    const int32_t* done = w.si + I_DONE;
    const double r2 = radius * radius, tol2 = tol * tol;
    // out = in (nullptr: zeros) +- sum scale_k P~_k over the accepted stars: the renderer's tile walk
    auto walk = [&](const double* in, const double* scale, bool subtract, double* out, const int32_t* dn) {
        if constexpr (LAYERS)
            launch_render_walk_layers(s, ny, nx, layers, in, stars, scale, nu, w.accept, subtract, out, d_ws, dn, I_NINT);
        else
            launch_render_walk(s, ny, nx, in, stars, scale, subtract, out, d_ws, dn);
    };
    // g = A^T W (V + c) and, with dg, the diagonal of N
    auto project = [&](const double* V, const double* c, double* g, double* dg, const int32_t* dn) {
        hipLaunchKernelGGL((k_ff_star<true, LAYERS>), dim3(nstar, layers), dim3(kStarThreads), 0, s, ny, nx, stars, r2,
                           StarProjection{w.W, V, c, w.accept, dn, g, dg});
    };
    // the partials of sum W (V + csign c), sum W, sum W (V + csign c)^2 and |Omega|
    auto reduce = [&](const double* V, const double* c, double csign, const int32_t* dn) {
        hipLaunchKernelGGL(k_ff_reduce<LAYERS>, dim3(w.nchunk, layers), dim3(256), 0, s, w.npix, w.nchunk, w.W, V, c, nu,
                           csign, w.partial, dn);
    };
    auto step = [&](auto phase) {
        hipLaunchKernelGGL((k_ff_step<decltype(phase)::value, LAYERS>), dim3(layers), dim3(kStepThreads), 0, s, nstar,
                           back, w.nchunk, tol2, w.accept, w.stat, w.ndisc, w.sump, w.x, w.r, w.p, w.q, w.diag, w.partial,
                           w.sd, w.si, d_star_out, d_head_out);
    };
    const double* constant = w.p + nstar;             // the constant's component of the direction p
    // the stars judged and the lists -- of a frame: of the accepted stars; of layers: of every placed star, from the
    // geometry alone, sorted here once and for all --, then the weights on Omega
    if constexpr (LAYERS) {
        launch_render_lists(s, ny, nx, stars, nullptr, nullptr, nullptr, d_ws);
        launch_render_sort(s, ny, nx, nstar, d_ws);
    }
    hipLaunchKernelGGL((k_ff_star<false, LAYERS>), dim3(nstar, layers), dim3(kStarThreads), 0, s, ny, nx, stars, r2,
                       StarJudging{d_image, d_var, d_scale0, w.accept, w.stat, w.ndisc, w.sump, w.diag, w.x});
    if constexpr (!LAYERS) launch_render_lists(s, ny, nx, stars, nullptr, w.accept, nullptr, d_ws);
    hipLaunchKernelGGL(k_ff_domain<LAYERS>, dim3(w.lists.ntx, w.lists.nty, layers), dim3(256), 0, s, ny, nx, d_image,
                       d_var, stars, r2, w.lists.offset, w.lists.pairs, w.accept, w.W);
    // r0 = A^T W (D - A x0), and the diagonal of N
    walk(d_image, w.x, true, w.M, nullptr);
    project(w.M, nullptr, w.q, w.diag, nullptr);
    reduce(w.M, nullptr, 1.0, nullptr);
    step(std::integral_constant<int, STEP_INIT>{});
    for (int it = 0; it < max_iter; ++it) {           // q = N p: one tile walk, one projection, one frame reduction
        walk(nullptr, w.p, false, w.M, done);
        project(w.M, constant, w.q, nullptr, done);
        if (back) reduce(w.M, constant, 1.0, done);
        step(std::integral_constant<int, STEP_ITER>{});
    }
    // the residual frame by the renderer itself, chi2 from it, the overlap from N 1
    double* R = d_resid_out ? d_resid_out : w.M;
    walk(d_image, w.x, true, R, nullptr);
    reduce(R, w.x + nstar, -1.0, nullptr);
    const int nones = LAYERS ? layers * nu : nstar;   // (of layers: the whole of p, the constants' places with it)
    hipLaunchKernelGGL(k_ff_ones, dim3((nones + 255) / 256), dim3(256), 0, s, nones, w.p);
    walk(nullptr, w.p, false, w.M, nullptr);
    project(w.M, nullptr, w.q, nullptr, nullptr);
    step(std::integral_constant<int, STEP_FINAL>{});
}

}  // namespace
}  // namespace mpsfr
