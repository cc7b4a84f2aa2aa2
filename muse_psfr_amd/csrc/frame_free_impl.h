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

template <int T>
__device__ __forceinline__ double block_max(double v, double* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) s = fmax(s, part[w]);
    return s;
}

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

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
