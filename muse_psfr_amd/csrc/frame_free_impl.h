// The two frame kernels of the fits with free positions (DESIGN.md sections 26 and 27), each in two forms:
//   k_fr_walk      the three-column tile walk: sum_k (F_k P~_k + a_k d_y + c_k d_x) at every pixel, in star-index order,
//                  over the sorted tile lists; the LDS stage and the two-buffer pipeline of k_render_tiles, the
//                  derivative columns from the second tap vector of each axis (KeysTaps::dw) on the same staged pixels
//   k_fr_project   one workgroup per accepted star, the footprint batches of k_ff_star<true>: three sums per pass and,
//                  in the first pass of a solve, the three sums of the data (the stop rule's g) and the six sums of the
//                  star's 3 x 3 block of N
// LAYERS = false is the frame's (mpsfr_fit_frame_psf_free; frame_free.hip instantiates it).  LAYERS = true is that of
// the layers of a cube side by side (mpsfr_fit_cube_psf_free; cube_free.hip): the layer is one more grid dimension, the
// first statement of a kernel moves its pointers to its layer, the lists hold every placed star and accept
// [layers][nstar] says which of them a layer sums, and the two derivative scales of a star that its layer carries are
// a = F0[l][k] delta[k], c = F0[l][k] delta[n + k], one rounded product each, before three_terms.  The arithmetic of a
// layer, and the order of every sum, is that of the frame: the same code.
// And what the two step kernels k_fr_step and k_cf_step share beyond frame_fit_impl.h's pieces: the scalar words of a
// call, the carry rule (carries), a place of the first residual (first_place), the end of an inner step (free_iter_end),
// the move of a shift along one axis (move_shift) and the end of an outer step (outer_end).
#pragma once
#include "frame_fit_impl.h"

namespace mpsfr {
namespace {

// the tile layout of k_render_tiles (render.hip)
constexpr int kWThreads = 256;
constexpr int kWRows = kWThreads / kTile;
constexpr int kWPix = kTile / kWRows;                         // pixels per thread: adjacent rows of one column
constexpr int kWWaveRows = 64 / kTile * kWPix;
constexpr int kWSide = kTile + 3;
constexpr int kWStride = kWSide + 1;
constexpr int kWLoads = (kWSide * kWSide + kWThreads - 1) / kWThreads;
static_assert(kTile * kTile == kWThreads * kWPix && kWRows * kTile == kWThreads, "tile layout");

constexpr int FLAG_HELD = 1, FLAG_BOUND = 2, FLAG_CLIPPED = 4;
// the places of a star's block of N: the diagonal (the preconditioner) first
enum { B_FF = 0, B_AA, B_CC, B_FA, B_FC, B_AC, B_N };

// The scalars of a call that mean the same in both free fits, doubles and ints; each fit appends its own
enum { D_RHO = 0, D_RHOG, D_REL, D_MAXD, D_SHARED };
enum {
    J_DONE = 0,   // the solve under way has ended
    J_GN,         // ... or the outer loop has: what the kernels of a Gauss-Newton step's iterations look at
    J_OUTER,      // the outer loop has ended
    J_ITER, J_ITERSUM, J_STOP, J_NOUTER, J_NFREE, J_POSOK, J_SHARED
};

// The pieces of the step kernels k_fr_step and k_cf_step that are one text (the invariants: frame_fit_impl.h, above
// cg_advance).

// The carry rule: the positions of a star count in a solve when its flux stands min_snr conditional errors above zero
// and its block b of N has a usable diagonal
__device__ __forceinline__ bool carries(double F, const double* b, double s2, double min_snr) {
    return positive_finite(F) && positive_finite(b[B_AA]) && positive_finite(b[B_CC]) &&
           F > min_snr * sqrt(s2 / b[B_FF]);
}

// One place of the first residual of a solve: d its place of the preconditioner, ri of the residual, gi of the data's
// projection, all as if 0 unless `on`.  Writes diag, r and p = r / d at `at`; adds to rz (rho) and gz (the stop
// reference rhog).
__device__ __forceinline__ void first_place(bool on, double d, double ri, double gi, double* diag, double* r, double* p,
                                            size_t at, double& rz, double& gz) {
    ri = on ? ri : 0.0;
    gi = on ? gi : 0.0;
    const double zi = on ? ri / d : 0.0;
    diag[at] = d;
    r[at] = ri;
    p[at] = zi;
    rz += ri * zi;
    gz += on ? gi * (gi / d) : 0.0;
}

// The end of a conjugate-gradient step of a free fit, by thread 0: the scalars and the done words of the call
__device__ __forceinline__ void free_iter_end(const CgEnd& e, double rhog, double* sd, int32_t* si) {
    sd[D_RHO] = e.rho1;
    sd[D_REL] = sqrt(e.rho1 / rhog);
    si[J_ITER] += 1;
    si[J_ITERSUM] += 1;
    if (e.end) {
        si[J_DONE] = 1;
        si[J_GN] = 1;
    }
    if (e.stop) si[J_STOP] = 0;
}

// The move of one star's shift s along one axis by the step d: a step that is not finite is none, |d| is clipped to
// max_step (FLAG_CLIPPED), the new shift to within max_move of the start s0 and to [lo8, hi8], the +-8 px domain
// (FLAG_BOUND).  Returns the new shift; absd: |d| before the clips.
__device__ __forceinline__ double move_shift(double d, double s, double s0, double max_step, double max_move, double lo8,
                                             double hi8, int& flag, double& absd) {
    if (!(fabs(d) < __builtin_inf())) d = 0.0;
    absd = fabs(d);
    if (fabs(d) > max_step) {
        d = d > 0.0 ? max_step : -max_step;
        flag |= FLAG_CLIPPED;
    }
    const double lo = fmax(s0 - max_move, lo8), hi = fmin(s0 + max_move, hi8);
    s += d;
    if (s <= lo) {
        s = lo;
        flag |= FLAG_BOUND;
    } else if (s >= hi) {
        s = hi;
        flag |= FLAG_BOUND;
    }
    return s;
}
// The end of an outer step: the largest |d| of the workgroup (md: the thread's own) against pos_tol.  Returns whether
// the outer loop has ended; thread 0 writes the scalars.
__device__ __forceinline__ bool outer_end(double md, double pos_tol, double* sd, int32_t* si, double* part) {
    const double maxd = block_max<kStepThreads>(md, part);
    const bool over = maxd <= pos_tol;
    if (threadIdx.x == 0) {
        si[J_NOUTER] += 1;
        sd[D_MAXD] = maxd;
        if (over) {
            si[J_OUTER] = 1;
            si[J_GN] = 1;
            si[J_POSOK] = 1;
        }
    }
    return over;
}

// What the layered walk reads beside the frame's arguments: vec is [layers][nstar + 1] (the fluxes' places of the joint
// vector), freem [layers][nstar] marks the stars a layer carries, delta [2 nstar] the shifts' places, f0 [layers][nstar]
// the fluxes before the step, accept [layers][nstar]; the done word of layer l is done[l done_pitch]
struct NoFreeLayers {};
struct FreeLayers {
    const double *f0, *delta;
    const int32_t* accept;
    int done_pitch;
};

// One star as a tile sees it (TileStar of render.hip, with the three scales of the star)
struct WalkStar {
    int op, oq, r0, c0, three;
    double f, a, c;
    const double* P;
    KeysTaps<double> ty{0.0}, tx{0.0};
    template <bool LAYERS>
    __device__ __forceinline__ void load(int k, int Y0, int X0, const StarList& stars, const double* vec,
                                         const int32_t* freem, const std::conditional_t<LAYERS, FreeLayers, NoFreeLayers>& lay) {
        const FrameStar star(stars, k);
        const int n = stars.nstar;
        op = star.op;
        oq = star.oq;
        three = freem[k];
        f = vec[k];
        if constexpr (LAYERS) {
            const double f0 = three ? lay.f0[k] : 0.0;
            a = three ? f0 * lay.delta[k] : 0.0;
            c = three ? f0 * lay.delta[n + k] : 0.0;
        } else {
            a = three ? vec[n + k] : 0.0;
            c = three ? vec[2 * n + k] : 0.0;
        }
        ty = KeysTaps<double>(star.dp);
        tx = KeysTaps<double>(star.dq);
        P = star.model(stars);
        r0 = Y0 - op + ty.f - 1;
        c0 = X0 - oq + tx.f - 1;
    }
    __device__ __forceinline__ void fetch(int tid, double (&pre)[kWLoads]) const {
#pragma unroll
        for (int m = 0; m < kWLoads; ++m) {
            const int e = tid + m * kWThreads, si = e / kWSide, sj = e - si * kWSide;
            pre[m] = model_pixel(P, r0 + si, c0 + sj, e < kWSide * kWSide);
        }
    }
};

// f val + a py + c px, every product rounded, summed in this order
__device__ __forceinline__ double three_terms(double f, double val, double a, double py, double c, double px) {
#pragma clang fp contract(off)
    const double t0 = f * val, t1 = a * py, t2 = c * px;
    return (t0 + t1) + t2;
}

// out = sum_k (vec[k] P~_k + vec[n + k] dP~_k/ds_y + vec[2 n + k] dP~_k/ds_x), the derivative columns for the stars
// freem marks, over the tile lists of d_ws, which are sorted.  Nothing once *done is set.  LAYERS: of layer blockIdx.z,
// over the stars its accept marks, the derivative scales as FreeLayers says.
template <bool LAYERS>
__global__ __launch_bounds__(kWThreads) void k_fr_walk(int ny, int nx, StarList stars, const double* __restrict__ vec,
                                                       const int32_t* __restrict__ freem,
                                                       const int* __restrict__ offset, const int* __restrict__ pairs,
                                                       const int32_t* __restrict__ done, double* __restrict__ out,
                                                       std::conditional_t<LAYERS, FreeLayers, NoFreeLayers> lay) {
    __shared__ double stage[2 * kWSide * kWStride];
    if constexpr (LAYERS) {
        const size_t b = blockIdx.z;
        done += b * lay.done_pitch;
        out += b * ny * nx;
        vec += b * (stars.nstar + 1);
        freem += b * stars.nstar;
        lay.f0 += b * stars.nstar;
        lay.accept += b * stars.nstar;
        stars.layer = blockIdx.z;
    }
    if (*done) return;
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly0 = tid / kTile;
    const int t = blockIdx.y * gridDim.x + blockIdx.x;
    const int Y0 = blockIdx.y * kTile, X0 = blockIdx.x * kTile, X = X0 + lx;
    const int first = offset[t], n = offset[t + 1] - first;
    const int* list = pairs + first;
    double acc[kWPix];
    bool on[kWPix];
#pragma unroll
    for (int j = 0; j < kWPix; ++j) {
        on[j] = Y0 + kWPix * ly0 + j < ny && X < nx;
        acc[j] = 0.0;
    }
    // the first place of the list from i on whose star takes part
    auto next = [&](int i) {
        if constexpr (LAYERS)
            while (i < n && !lay.accept[list[i]]) ++i;
        return i;
    };
    // (the pipeline of k_render_tiles: star i + 1 fetched into registers while star i is evaluated, two buffers, one
    // barrier per star)
    WalkStar cur, nxt;
    double pre[kWLoads];
    int i = next(0);
    if (i < n) {
        cur.load<LAYERS>(list[i], Y0, X0, stars, vec, freem, lay);
        cur.fetch(tid, pre);
    }
    for (int turn = 0; i < n; ++turn) {
        double* buf = stage + (turn & 1) * (kWSide * kWStride);
#pragma unroll
        for (int m = 0; m < kWLoads; ++m) {
            const int e = tid + m * kWThreads;
            if (e < kWSide * kWSide) buf[(e / kWSide) * kWStride + e % kWSide] = pre[m];
        }
        i = next(i + 1);
        if (i < n) {
            nxt.load<LAYERS>(list[i], Y0, X0, stars, vec, freem, lay);
            nxt.fetch(tid, pre);
        }
        __syncthreads();
        const StagedStamp<kWStride> st{buf};
        const int q = X - cur.oq;
        const int pw = Y0 + (tid / 64) * kWWaveRows - cur.op;
        if (pw + kWWaveRows > -kPsfApron && pw < NS + kPsfApron) {
#pragma unroll
            for (int j = 0; j < kWPix; ++j) {
                const int ly = kWPix * ly0 + j, p = Y0 + ly - cur.op;
                double val, gy, gx, term;
                if (cur.three) {          // (the same for the whole workgroup)
                    psf_interp<double, true>(st, ly * kWStride + lx, p, q, cur.ty, cur.tx, val, gy, gx);
                    term = three_terms(cur.f, val, cur.a, -gy, cur.c, -gx);     // d/ds = -d/dy
                } else {
                    psf_interp<double, false>(st, ly * kWStride + lx, p, q, cur.ty, cur.tx, val, gy, gx);
                    term = three_terms(cur.f, val, 0.0, 0.0, 0.0, 0.0);
                }
                const bool inside = on[j] && p >= -kPsfApron && p < NS + kPsfApron && q >= -kPsfApron &&
                                    q < NS + kPsfApron;
                acc[j] = inside ? acc[j] + term : acc[j];
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (int j = 0; j < kWPix; ++j) {
        const int Y = Y0 + kWPix * ly0 + j;
        if (on[j]) out[(size_t)Y * nx + X] = acc[j];
    }
}

// What the projection reads and writes.  q[k], q[n + k], q[2 n + k] = sum W col (V + csign c) for the columns of star k
// (the derivative ones: of a star freem marks; FIRST: of every accepted star); FIRST: g the same of the data D, and
// blk[6 k ..] the star's block of N.  Of layers: the frames at ny nx, c at nstar + 1, q and g at 3 nstar, blk at 6 nstar,
// accept and freem at nstar, the done word at I_NINT.
struct FreeProjection {
    const double *W, *V, *D, *c;
    double csign;
    const int32_t *accept, *freem, *done;
    double *q, *g, *blk;
    __device__ __forceinline__ void layer(size_t b, size_t npix, size_t n) {
        W += b * npix;
        V += b * npix;
        D += b * npix;
        if (c) c += b * (n + 1);
        accept += b * n;
        freem += b * n;
        if (done) done += b * I_NINT;
        q += b * 3 * n;
        g += b * 3 * n;
        blk += b * B_N * n;
    }
};

template <bool FIRST, bool LAYERS>
__global__ __launch_bounds__(kStarThreads) void k_fr_project(int ny, int nx, StarList stars, FreeProjection io) {
    __shared__ double stage[kFootSide * kFootStride];
    __shared__ double part[kStarThreads / 64];
    const int k = blockIdx.x, tid = threadIdx.x, n = stars.nstar;
    if constexpr (LAYERS) {
        io.layer(blockIdx.y, (size_t)ny * nx, (size_t)n);
        stars.layer = blockIdx.y;
    }
    if ((io.done && *io.done) || !io.accept[k]) return;
    const bool three = FIRST || io.freem[k] != 0;
    const FrameStar star(stars, k);
    const int op = star.op, oq = star.oq;
    const double* P = star.model(stars);
    const KeysTaps<double> ty(star.dp), tx(star.dq);
    const int r0 = ty.f - 1 - kPsfApron, c0 = tx.f - 1 - kPsfApron;
    for (int e = tid; e < kFootSide * kFootSide; e += kStarThreads) {
        const int i = e / kFootSide, j = e - i * kFootSide;
        stage[i * kFootStride + j] = model_pixel(P, r0 + i, c0 + j);
    }
    __syncthreads();
    const StagedStamp<kFootStride> st{stage};
    const double cval = io.c ? io.csign * *io.c : 0.0;
    double sq[3] = {0.0, 0.0, 0.0}, sg[3] = {0.0, 0.0, 0.0}, sb[B_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int m0 = 0; m0 < kFootShare; m0 += kFootBatch) {
        double fa[kFootBatch], fb[kFootBatch], fd[kFootBatch];
#pragma unroll
        for (int j = 0; j < kFootBatch; ++j) {
            const int e = tid + (m0 + j) * kStarThreads, pr = e / kPsfSide, qc = e - pr * kPsfSide;
            const int Y = op - kPsfApron + pr, X = oq - kPsfApron + qc;
            const bool on = e < kFootPix && Y >= 0 && Y < ny && X >= 0 && X < nx;
            const size_t src = on ? (size_t)Y * nx + (size_t)X : 0;
            fa[j] = io.W[src];
            fb[j] = io.V[src];
            if constexpr (FIRST) fd[j] = io.D[src];
        }
#pragma unroll
        for (int j = 0; j < kFootBatch; ++j) {
            const int e = tid + (m0 + j) * kStarThreads, pr = e / kPsfSide, qc = e - pr * kPsfSide;
            const int Y = op - kPsfApron + pr, X = oq - kPsfApron + qc;
            const bool on = e < kFootPix && Y >= 0 && Y < ny && X >= 0 && X < nx;
            const double w = fa[j];
            if (on && w > 0.0) {                      // (W is 0 outside Omega; a masked datum may be NaN: selected out)
                double val, gy, gx;
                const double u = w * (fb[j] + cval);
                if (three) {
                    psf_interp<double, true>(st, pr * kFootStride + qc, 0, 0, ty, tx, val, gy, gx);
                    const double py = -gy, px = -gx;
                    sq[0] += u * val;
                    sq[1] += u * py;
                    sq[2] += u * px;
                    if constexpr (FIRST) {
                        const double ud = w * fd[j], wv = w * val, wy = w * py;
                        sg[0] += ud * val;
                        sg[1] += ud * py;
                        sg[2] += ud * px;
                        sb[B_FF] += wv * val;
                        sb[B_AA] += wy * py;
                        sb[B_CC] += (w * px) * px;
                        sb[B_FA] += wv * py;
                        sb[B_FC] += wv * px;
                        sb[B_AC] += wy * px;
                    }
                } else {
                    psf_interp<double, false>(st, pr * kFootStride + qc, 0, 0, ty, tx, val, gy, gx);
                    sq[0] += u * val;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j == 0 || three) {                        // (the same for the whole workgroup)
            const double tq = block_sum<kStarThreads>(sq[j], part);
            if (tid == 0) io.q[j * n + k] = tq;
        }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double tg = block_sum<kStarThreads>(sg[j], part);
            if (tid == 0) io.g[j * n + k] = tg;
        }
#pragma unroll
        for (int j = 0; j < B_N; ++j) {
            const double tb = block_sum<kStarThreads>(sb[j], part);
            if (tid == 0) io.blk[(size_t)B_N * k + j] = tb;
        }
    }
}

}  // namespace
}  // namespace mpsfr
