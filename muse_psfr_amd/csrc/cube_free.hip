// Crowded-field PSF photometry of a cube with free positions (mpsfr_fit_cube_psf_free,
// include/mpsfr.h): one shift per star from all layers jointly.  Per layer everything is section 25's -- the judging,
// Omega and the weights at the start shifts, once; the layers side by side in every launch --, the Gauss-Newton loop is
// section 26's on one joint vector
//     F, b of layer 0 | F, b of layer 1 | ... | delta_y [nstar] | delta_x [nstar]         (nl (nstar + 1) + 2 nstar places)
// with a live mask: the F of a star its layer accepted, the b of a live layer with the background on, the two delta of
// a free star.  The column of delta_y of star k is sum over the layers that carry k of F0_kl dP~_kl/ds_y:
//   k_fr_walk<true>     (frame_free_impl.h) takes a = F0 delta_y, c = F0 delta_x for a carried star
//   k_fr_project<true>  (the same) gives the three sums per (layer, star); the delta places of q are then
//                       sum_l F0_kl q_a,kl in layer order, formed by the step kernel
//   k_cf_begin          the working shifts, the counters, the scalars and the +-8 bounds across the layers
//   k_cf_step           ONE workgroup over the joint vector: CF_JUDGE (dead layers, who carries, who is free, F0, the
//                       delta places of the preconditioner and of the first residual), CF_INIT (the places of the
//                       layers, the first residual, the stop reference, the done words), CF_ITER (a conjugate-gradient
//                       step), CF_APPLY (delta, its clips, the new shifts, the outer done word), CF_FINAL (rows, heads,
//                       pos_out, call_out)
// k_ff_star<false, true>, k_ff_domain<true>, k_ff_reduce<true>, k_ff_ones and the renderer's layered walk are reused as
// they are: their done word is per layer at a pitch of I_NINT, so the step kernel keeps the call's three done words once
// (si) and a copy per layer (gate), a dead layer's copies always set.  The step kernel's loops and the order of its sums
// are its own (below); what it computes at one place, one row, one head or one shift is the frame's: cg_advance,
// cg_direct, cg_alpha, cg_end, cg_beta, star_row, solve_head (frame_fit_impl.h), carries, first_place, free_iter_end,
// move_shift, outer_end and the shared scalar words (frame_free_impl.h).
//
// The order of every sum (none depends on a grid):
//   over the places of ONE layer, and over the chunks of a layer's frame reductions: lane j of a wave takes the places
//     j, j + 64, ... in order, then the wave's ladder (wave_sum); which wave of the workgroup takes a layer has no
//     influence on the value;
//   over the layers: in layer order, a dead layer adding 0.0, by every thread alike (layers_sum);
//   over the delta places: thread t takes the stars t, t + 1024, ..., y before x, then block_sum's tree;
//   a joint scalar product is (the sum over the layers) + (the sum over the delta places);
//   inside a star's delta place (the preconditioner, q, g, the first residual): over the layers in layer order.
#include <algorithm>

#include "frame_free_impl.h"

namespace mpsfr {
namespace {

constexpr int NPOS = 8;                                       // MPSFR_NCUBEFREE_POS, MPSFR_NCUBEFREE_CALL
constexpr int kStepWaves = kStepThreads / 64;
constexpr int kMaxLayers = 4096;                              // MPSFR_CUBE_FIT_MAX_LAYERS

// the scalars of a call: the shared ones (frame_free_impl.h), then the cube's own
enum { D_RHO_D = D_SHARED, D_RHOG_D, D_LO8, D_HI8 = D_LO8 + 2, D_NDOUBLE = D_HI8 + 2 };
enum { J_ALLDEAD = J_SHARED, J_FREENOW, J_NINT };
// the words of a layer's gate (pitch I_NINT): copies of the first three, 1 for a dead layer; and whether it is dead
enum { G_DONE = J_DONE, G_GN = J_GN, G_OUTER = J_OUTER, G_DEAD };
static_assert(G_DEAD < I_NINT, "a layer's gate has the pitch of section 25's scalars");
// the scalars of a layer (lw[kind][layer])
enum { L_GB = 0, L_WSUM, L_CHI, L_GD, L_S2, L_RHO, L_RHOG, L_REL, L_QB, L_PQ, L_NOMEGA, L_NACC, L_DOF, L_N };

// the shifts, the counters, the scalars; wave 0 of workgroup 0: for each axis the interval of shifts s with
// |s + layer_shift[l]| <= 8 in every layer after rounding (without layer_shift: [-8, 8])
__global__ __launch_bounds__(256) void k_cf_begin(int n, int nl, const double* __restrict__ shift_in,
                                                  const double* __restrict__ lshift, double* __restrict__ shift0,
                                                  double* __restrict__ wshift, double* __restrict__ x, size_t nvec,
                                                  int32_t* __restrict__ star_i, int32_t* __restrict__ layer_i,
                                                  int32_t* __restrict__ gate, double* __restrict__ sd,
                                                  int32_t* __restrict__ si, int posok) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * (size_t)n) {
        const double v = shift_in ? shift_in[i] : 0.0;
        shift0[i] = v;
        wshift[i] = v;
    }
    if (i < nvec) x[i] = 0.0;
    if (i < 5 * (size_t)n) star_i[i] = 0;                     // freem, nfree, sflag, held, seen
    if (i < 2 * (size_t)nl * n) layer_i[i] = 0;               // carry, carryl
    if (i < (size_t)nl * I_NINT) gate[i] = 0;
    if (i < D_LO8) sd[i] = 0.0;
    if (i < J_NINT) si[i] = i == J_POSOK ? posok : 0;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        for (int ax = 0; ax < 2; ++ax) {
            double lo = -kPsfMaxShift, hi = kPsfMaxShift;
            if (lshift) {
                for (int l = lane; l < nl; l += 64) {
                    const double t = lshift[2 * l + ax];
                    lo = fmax(lo, -kPsfMaxShift - t);
                    hi = fmin(hi, kPsfMaxShift - t);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    lo = fmax(lo, __shfl_xor(lo, o, 64));
                    hi = fmin(hi, __shfl_xor(hi, o, 64));
                }
                for (int turn = 0; turn < 4; ++turn) {        // (a rounded sum may still pass the bound by an ulp)
                    bool low = false, high = false;
                    for (int l = lane; l < nl; l += 64) {
                        const double t = lshift[2 * l + ax];
                        low = low || lo + t < -kPsfMaxShift;
                        high = high || hi + t > kPsfMaxShift;
                    }
                    if (__any(low)) lo = nextafter(lo, __builtin_inf());
                    if (__any(high)) hi = nextafter(hi, -__builtin_inf());
                }
            }
            if (lane == 0) {
                sd[D_LO8 + ax] = lo;
                sd[D_HI8 + ax] = hi;
            }
        }
    }
}

enum { CF_JUDGE = 0, CF_INIT, CF_ITER, CF_APPLY, CF_FINAL };

struct CubeStep {
    int n, nl, back, nchunk, gn;              // gn: a Gauss-Newton step (else the positions are held)
    double tol2, min_snr, max_step, max_move, pos_tol;
    const int32_t *accept, *stat;             // [nl][n]
    const double *ndisc, *sump;               // [nl][n]
    const double* shift0;
    double *wshift, *x, *r, *p, *diag;        // the joint vectors
    double *q3, *g3, *blk, *blkl, *f0;        // [nl][3 n], [nl][3 n], [nl][6 n], [nl][6 n], [nl][n]
    double* qd;                               // the delta places of q [2 n]
    const double *partial, *partial_d;        // [nl][4][nchunk]
    double *lw, *sd;
    int32_t *si, *gate, *carry, *carryl, *freem, *nfree, *sflag, *held, *seen;
    const int32_t* word;                      // CF_ITER: the done word of its solve
    double *star_out, *head_out, *pos_out, *shift_out, *call_out;
};

template <int PHASE>
__global__ __launch_bounds__(kStepThreads) void k_cf_step(CubeStep a) {
    __shared__ double part[kStepWaves];
    __shared__ double lsh[kMaxLayers];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, nl = a.nl, nv = n + 1;
    const size_t NB = (size_t)nl * nv;
    double* const sd = a.sd;
    int32_t* const si = a.si;
    auto lw = [&](int kind, int l) -> double& { return a.lw[(size_t)kind * nl + l]; };
    auto dead = [&](int l) { return a.gate[(size_t)l * I_NINT + G_DEAD] != 0; };
    // the sum of a scalar of the layers over the live ones, in layer order
    auto layers_sum = [&](int kind) {
        __syncthreads();
        for (int l = tid; l < nl; l += kStepThreads) lsh[l] = dead(l) ? 0.0 : lw(kind, l);
        __syncthreads();
        double s = 0.0;
        for (int l = 0; l < nl; ++l) s += lsh[l];
        return s;
    };
    auto set_gates = [&](int done, int gn, int outer) {
        for (int l = tid; l < nl; l += kStepThreads) {
            int32_t* g = a.gate + (size_t)l * I_NINT;
            const int dd = g[G_DEAD];
            g[G_DONE] = dd | done;
            g[G_GN] = dd | gn;
            g[G_OUTER] = dd | outer;
        }
    };
    const int nb = n + (a.back ? 1 : 0);      // the places of a layer that can be live
    if constexpr (PHASE == CF_JUDGE) {
        if (a.gn && si[J_OUTER]) return;
        const double back = a.back ? 1.0 : 0.0;
        // the frame sums of every layer, its accepted stars, whether it is dead, its s2 at the current shifts
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            const double* pa = a.partial + (size_t)l * 4 * a.nchunk;
            const double* pd = a.partial_d + (size_t)l * 4 * a.nchunk;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, na = 0.0;
#pragma unroll 1
            for (int c = lane; c < a.nchunk; c += 64) {
                s0 += pa[c];
                s1 += pa[a.nchunk + c];
                s2 += pa[2 * (size_t)a.nchunk + c];
                s3 += pa[3 * (size_t)a.nchunk + c];
                s4 += pd[c];
            }
#pragma unroll 1
            for (int k = lane; k < n; k += 64) na += a.accept[(size_t)l * n + k] ? 1.0 : 0.0;
            s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3), s4 = wave_sum(s4);
            na = wave_sum(na);
            const bool dd = na < 1.0 || s3 < na + back + 1.0;
            if (lane == 0) {
                lw(L_GB, l) = s0;
                lw(L_WSUM, l) = s1;
                lw(L_CHI, l) = s2;
                lw(L_GD, l) = s4;
                lw(L_NOMEGA, l) = s3;
                lw(L_NACC, l) = na;
                lw(L_S2, l) = dd ? 0.0 : s2 / (s3 - na - back);
                lw(L_DOF, l) = 1.0;           // (here: a live layer counts one)
                a.gate[(size_t)l * I_NINT + G_DEAD] = dd ? 1 : 0;
            }
        }
        __syncthreads();
        // who carries (section 26's rule per layer), and the stars accepted in some live layer
        double cnt = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            bool anyacc = false, anycarry = false;
#pragma unroll 1
            for (int l = 0; l < nl; ++l) {
                const size_t o = (size_t)l * n + k;
                const bool acc = !dead(l) && a.accept[o] != 0;
                const bool cr = a.gn && acc &&
                                carries(a.x[(size_t)l * nv + k], a.blk + (size_t)B_N * o, lw(L_S2, l), a.min_snr);
                a.carry[o] = cr ? 1 : 0;
                anyacc = anyacc || acc;
                anycarry = anycarry || cr;
            }
            a.freem[k] = anycarry ? 1 : 0;
            a.seen[k] = anyacc ? 1 : 0;
            cnt += anyacc ? 1.0 : 0.0;
        }
        const double nseen = block_sum<kStepThreads>(cnt, part);
        const double somega = layers_sum(L_NOMEGA), sacc = layers_sum(L_NACC), nlive = layers_sum(L_DOF);
        const bool alldead = nlive < 1.0;
        // (no star moves unless the pixels outnumber the unknowns with every star free)
        const bool movable = a.gn && !alldead && somega >= sacc + back * nlive + 2.0 * nseen + 1.0;
        // who is free; F0, the blocks of this step, the delta places of the preconditioner, of r and of g
        double nf = 0.0, rz = 0.0, gz = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            const bool fr = movable && a.freem[k] != 0;
            a.freem[k] = fr ? 1 : 0;
            if (a.gn) {
                a.held[k] = a.seen[k] && !fr ? 1 : 0;
                if (fr) a.nfree[k] += 1;
            }
            double d[2] = {0.0, 0.0}, rr[2] = {0.0, 0.0}, gg[2] = {0.0, 0.0};
#pragma unroll 1
            for (int l = 0; l < nl; ++l) {
                const size_t o = (size_t)l * n + k;
                if (!fr) {
                    a.carry[o] = 0;
                    continue;
                }
                const int cr = a.carry[o];
                a.carryl[o] = cr;
                if (!cr) continue;
                const double F = a.x[(size_t)l * nv + k];
                const double* b = a.blk + (size_t)B_N * o;
                const double *q3 = a.q3 + (size_t)l * 3 * n, *g3 = a.g3 + (size_t)l * 3 * n;
                a.f0[o] = F;
#pragma unroll
                for (int j = 0; j < B_N; ++j) a.blkl[(size_t)B_N * o + j] = b[j];
                const double ff = F * F;
                d[0] += ff * b[B_AA];
                d[1] += ff * b[B_CC];
                rr[0] += F * q3[n + k];
                rr[1] += F * q3[2 * n + k];
                gg[0] += F * g3[n + k];
                gg[1] += F * g3[2 * n + k];
            }
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                const size_t i = NB + (size_t)ax * n + k;
                a.x[i] = 0.0;                 // delta = 0 at the start of every solve
                first_place(fr, fr ? d[ax] : 1.0, rr[ax], gg[ax], a.diag, a.r, a.p, i, rz, gz);
            }
            nf += fr ? 1.0 : 0.0;
        }
        const double nfr = block_sum<kStepThreads>(nf, part);        // (its barriers publish freem and carry)
        const double rho_d = block_sum<kStepThreads>(rz, part);
        const double rhog_d = block_sum<kStepThreads>(gz, part);
        if (tid == 0) {
            sd[D_RHO_D] = rho_d;
            sd[D_RHOG_D] = rhog_d;
            si[J_ALLDEAD] = alldead ? 1 : 0;
            si[J_FREENOW] = (int)nfr;
            if (a.gn) si[J_NFREE] = (int)nfr;
        }
    } else if constexpr (PHASE == CF_INIT) {
        if (a.gn && si[J_OUTER]) return;
        int ndone = si[J_DONE], ngn = si[J_GN], nouter = si[J_OUTER];
        const bool alldead = si[J_ALLDEAD] != 0, nobody = si[J_FREENOW] < 1;
        const double rho_d = sd[D_RHO_D], rhog_d = sd[D_RHOG_D];
        // the places of every layer
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            const bool dd = dead(l);
            const double wsum = lw(L_WSUM, l), gb = lw(L_GB, l), gd = lw(L_GD, l);
            const double *q3 = a.q3 + (size_t)l * 3 * n, *g3 = a.g3 + (size_t)l * 3 * n;
            double lz = 0.0, lg = 0.0;
#pragma unroll 1
            for (int i = lane; i <= n; i += 64) {
                const size_t at = (size_t)l * nv + i;
                bool on;
                double di, ri, gi;
                if (i == n) {
                    on = !dd && a.back;
                    di = wsum;
                    ri = gb;
                    gi = gd;
                } else {
                    on = !dd && a.accept[(size_t)l * n + i] != 0;
                    di = on ? a.blk[(size_t)B_N * ((size_t)l * n + i) + B_FF] : 1.0;
                    ri = on ? q3[i] : 0.0;
                    gi = on ? g3[i] : 0.0;
                }
                if (dd) a.x[at] = 0.0;
                first_place(on, di, ri, gi, a.diag, a.r, a.p, at, lz, lg);
            }
            lz = wave_sum(lz), lg = wave_sum(lg);
            if (lane == 0) {
                lw(L_RHO, l) = lz;
                lw(L_RHOG, l) = lg;
                lw(L_REL, l) = positive_finite(lg) ? sqrt(lz / lg) : 0.0;
            }
        }
        const double rho = layers_sum(L_RHO) + rho_d, rhog = layers_sum(L_RHOG) + rhog_d;
        if (a.gn && nobody) {                          // no star is free: the outer loop ends here, nothing to move
            nouter = 1;
            ngn = 1;
            if (tid == 0) si[J_POSOK] = 1;
        } else {
            const bool stop = rho <= a.tol2 * rhog;
            const bool more = !alldead && !stop && positive_finite(rho) && positive_finite(rhog);
            ndone = more ? 0 : 1;
            ngn = more ? 0 : 1;
            if (tid == 0) {
                sd[D_RHO] = rho;
                sd[D_RHOG] = rhog;
                sd[D_REL] = positive_finite(rhog) ? sqrt(rho / rhog) : 0.0;
                si[J_ITER] = 0;
                si[J_STOP] = stop ? 0 : 1;             // 1 until the stop test passes
            }
        }
        if (tid == 0) {
            si[J_DONE] = ndone;
            si[J_GN] = ngn;
            si[J_OUTER] = nouter;
        }
        set_gates(ndone, ngn, nouter);
    } else if constexpr (PHASE == CF_ITER) {
        if (*a.word) return;
        const double rho = sd[D_RHO], rhog = sd[D_RHOG];
        // q: its constants from the partials, its delta places from the layers; p . q
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            if (dead(l)) continue;
            double qb = 0.0;
            if (a.back) {
                const double* pa = a.partial + (size_t)l * 4 * a.nchunk;
                for (int c = lane; c < a.nchunk; c += 64) qb += pa[c];
                qb = wave_sum(qb);
            }
            const double* q3 = a.q3 + (size_t)l * 3 * n;
            double s = 0.0;
            for (int i = lane; i < nb; i += 64)
                if (i == n || a.accept[(size_t)l * n + i]) s += a.p[(size_t)l * nv + i] * (i == n ? qb : q3[i]);
            s = wave_sum(s);
            if (lane == 0) {
                lw(L_QB, l) = qb;
                lw(L_PQ, l) = s;
            }
        }
        double sdl = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            if (!a.freem[k]) continue;
            double qy = 0.0, qx = 0.0;
#pragma unroll 1
            for (int l = 0; l < nl; ++l) {
                const size_t o = (size_t)l * n + k;
                if (!a.carry[o]) continue;
                const double F = a.f0[o];
                const double* q3 = a.q3 + (size_t)l * 3 * n;
                qy += F * q3[n + k];
                qx += F * q3[2 * n + k];
            }
            a.qd[k] = qy;
            a.qd[n + k] = qx;
            sdl += a.p[NB + k] * qy;
            sdl += a.p[NB + n + k] * qx;
        }
        const double pq_d = block_sum<kStepThreads>(sdl, part);
        const double pq = layers_sum(L_PQ) + pq_d;
        const double alpha = cg_alpha(rho, pq);
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            if (dead(l)) continue;
            const double qb = lw(L_QB, l);
            const double* q3 = a.q3 + (size_t)l * 3 * n;
            double lz = 0.0;
            for (int i = lane; i < nb; i += 64)
                if (i == n || a.accept[(size_t)l * n + i])
                    lz += cg_advance(alpha, i == n ? qb : q3[i], a.x, a.r, a.p, a.diag, (size_t)l * nv + i);
            lz = wave_sum(lz);
            if (lane == 0) {
                lw(L_RHO, l) = lz;
                lw(L_REL, l) = sqrt(lz / lw(L_RHOG, l));
            }
        }
        double rz = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            if (!a.freem[k]) continue;
#pragma unroll
            for (int ax = 0; ax < 2; ++ax)
                rz += cg_advance(alpha, a.qd[ax * n + k], a.x, a.r, a.p, a.diag, NB + (size_t)ax * n + k);
        }
        const double rho_d = block_sum<kStepThreads>(rz, part);
        const CgEnd e = cg_end(layers_sum(L_RHO) + rho_d, pq, a.tol2, rhog);
        const double beta = cg_beta(e, rho);
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            if (dead(l)) continue;
            for (int i = lane; i < nb; i += 64)
                if (i == n || a.accept[(size_t)l * n + i]) cg_direct(beta, a.r, a.diag, a.p, (size_t)l * nv + i);
        }
        for (int k = tid; k < n; k += kStepThreads) {
            if (!a.freem[k]) continue;
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) cg_direct(beta, a.r, a.diag, a.p, NB + (size_t)ax * n + k);
        }
        if (tid == 0) free_iter_end(e, rhog, sd, si);
        if (e.end) set_gates(1, 1, si[J_OUTER]);       // (the outer word is not written in this phase)
    } else if constexpr (PHASE == CF_APPLY) {
        if (si[J_OUTER]) return;
        double md = 0.0;
        for (int k = tid; k < n; k += kStepThreads) {
            if (!a.freem[k]) continue;
            int flag = 0;
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                double absd;
                a.wshift[2 * k + ax] = move_shift(a.x[NB + (size_t)ax * n + k], a.wshift[2 * k + ax],
                                                  a.shift0[2 * k + ax], a.max_step, a.max_move, sd[D_LO8 + ax],
                                                  sd[D_HI8 + ax], flag, absd);
                md = fmax(md, absd);
            }
            a.sflag[k] = flag;
        }
        if (outer_end(md, a.pos_tol, sd, si, part)) set_gates(si[J_DONE], 1, 1);   // (J_DONE is not written here)
    } else {
        const bool alldead = si[J_ALLDEAD] != 0;
        const double status = alldead ? 2.0 : (si[J_STOP] == 0 && si[J_POSOK] != 0 ? 0.0 : 1.0);
        const double back = a.back ? 1.0 : 0.0;
        // the rows and the head of every layer: section 25's columns of the closing solve
#pragma unroll 1
        for (int l = wave; l < nl; l += kStepWaves) {
            const bool dd = dead(l);
            const double* pa = a.partial + (size_t)l * 4 * a.nchunk + 2 * (size_t)a.nchunk;
            double chi2 = 0.0;
            for (int c = lane; c < a.nchunk; c += 64) chi2 += pa[c];
            chi2 = wave_sum(chi2);
            const double nomega = lw(L_NOMEGA, l), nacc = lw(L_NACC, l);
            const double dof = nomega - nacc - back, s2 = dd ? 0.0 : chi2 / dof;
            const double* q3 = a.q3 + (size_t)l * 3 * n;
            for (int k = lane; k < n; k += 64) {
                const size_t o = (size_t)l * n + k, at = (size_t)l * nv + k;
                star_row(a.star_out + (size_t)NROW * o, !dd && a.accept[o] != 0, a.x[at], a.diag[at], q3[k], s2,
                         a.sump[o], a.ndisc[o], a.stat[o]);
            }
            if (lane == 0) {
                double* h = a.head_out + (size_t)NROW * l;
                solve_head(h, a.back != 0, dd, a.x[(size_t)l * nv + n], s2, lw(L_WSUM, l), chi2, nomega,
                           (double)si[J_ITER], lw(L_REL, l), nacc);
                h[7] = dd ? 2.0 : status;
                lw(L_CHI, l) = chi2;
                lw(L_S2, l) = s2;
                lw(L_DOF, l) = dof;
            }
        }
        const double chisum = layers_sum(L_CHI), dofsum = layers_sum(L_DOF);      // (their barriers publish s2)
        double ne = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            const bool on = a.seen[k] != 0;
            const double sy = a.wshift[2 * k], sx = a.wshift[2 * k + 1];
            double ey = 0.0, ex = 0.0;
            if (on && a.nfree[k] > 0) {
                // S = sum over the layers that carried the star in its last free step of (F^2 / s2) times the Schur
                // complement of (a, c) over F in the layer's block of that step; the errors from the diagonal of its inverse
                double saa = 0.0, scc = 0.0, sac = 0.0;
#pragma unroll 1
                for (int l = 0; l < nl; ++l) {
                    const size_t o = (size_t)l * n + k;
                    if (!a.carryl[o] || dead(l)) continue;
                    const double F = a.x[(size_t)l * nv + k];
                    if (!positive_finite(F)) continue;
                    const double* b = a.blkl + (size_t)B_N * o;
                    const double ff = b[B_FF], fa = b[B_FA], fc = b[B_FC];
                    const double w = (F * F) / lw(L_S2, l);
                    saa += w * (b[B_AA] - fa * fa / ff);
                    scc += w * (b[B_CC] - fc * fc / ff);
                    sac += w * (b[B_AC] - fa * fc / ff);
                }
                const double det = saa * scc - sac * sac;
                const double vy = scc / det, vx = saa / det;
                ey = positive_finite(vy) ? sqrt(vy) : 0.0;
                ex = positive_finite(vx) ? sqrt(vx) : 0.0;
            }
            double* o = a.pos_out + (size_t)NPOS * k;
            o[0] = sy;
            o[1] = sx;
            o[2] = ey;
            o[3] = ex;
            o[4] = on ? sy - a.shift0[2 * k] : 0.0;
            o[5] = on ? sx - a.shift0[2 * k + 1] : 0.0;
            o[6] = on ? (double)(a.sflag[k] | (a.held[k] ? FLAG_HELD : 0)) : 0.0;
            o[7] = on ? (double)a.nfree[k] : 0.0;
            a.shift_out[2 * k] = sy;
            a.shift_out[2 * k + 1] = sx;
            ne += a.nfree[k] > 0 ? 1.0 : 0.0;
        }
        const double ever = block_sum<kStepThreads>(ne, part);
        if (tid == 0) {
            double* h = a.call_out;
            h[0] = alldead ? 0.0 : chisum;
            h[1] = alldead ? 0.0 : dofsum - 2.0 * ever;
            h[2] = (double)si[J_NOUTER];
            h[3] = sd[D_MAXD];
            h[4] = (double)si[J_NFREE];
            h[5] = (double)si[J_ITERSUM];
            h[6] = status;
            h[7] = alldead ? 0.0 : sd[D_REL];
        }
    }
}

// The workspace of a call: the renderer's lists once (at its start); per layer the frames W and M, the layer's places
// of x, r, p, diag [nstar + 1], q3, g3 [3 nstar], the blocks of N now and of each star's last free step [6 nstar]
// each, F0, ndisc, sump [nstar], the partials of the two frame reductions [2][4][chunks], L_N scalars, and accept, stat,
// carry, carryl [nstar] with the gate [I_NINT] as int32; once the delta places of x, r, p, diag and q [2 nstar] each,
// the start and the working shifts [2 nstar] each, the scalars, and freem, nfree, sflag, held, seen [nstar] as int32
struct CubeFreeWork {
    RenderLists lists;
    size_t npix, n, nl, nvec;
    int nchunk;
    double *W, *M, *x, *r, *p, *diag, *q3, *g3, *blk, *blkl, *f0, *ndisc, *sump, *partial, *partial_d, *lw, *qd, *shift0,
        *wshift, *sd;
    int32_t *accept, *stat, *layer_i, *gate, *star_i, *si;
    CubeFreeWork(WorkspaceCarver& ws, int ny, int nx, int nstar, int layers)
        : lists(ws, ny, nx, nstar), npix((size_t)ny * nx), n((size_t)nstar), nl((size_t)layers),
          nvec(nl * (n + 1) + 2 * n), nchunk((int)((npix + kChunk - 1) / kChunk)), W(ws.take<double>(nl * npix)),
          M(ws.take<double>(nl * npix)), x(ws.take<double>(nvec)), r(ws.take<double>(nvec)), p(ws.take<double>(nvec)),
          diag(ws.take<double>(nvec)), q3(ws.take<double>(nl * 3 * n)), g3(ws.take<double>(nl * 3 * n)),
          blk(ws.take<double>(nl * B_N * n)), blkl(ws.take<double>(nl * B_N * n)), f0(ws.take<double>(nl * n)),
          ndisc(ws.take<double>(nl * n)), sump(ws.take<double>(nl * n)), partial(ws.take<double>(nl * 4 * nchunk)),
          partial_d(ws.take<double>(nl * 4 * nchunk)), lw(ws.take<double>(nl * L_N)), qd(ws.take<double>(2 * n)),
          shift0(ws.take<double>(2 * n)), wshift(ws.take<double>(2 * n)), sd(ws.take<double>(D_NDOUBLE)),
          accept(ws.take<int32_t>(nl * n)), stat(ws.take<int32_t>(nl * n)), layer_i(ws.take<int32_t>(2 * nl * n)),
          gate(ws.take<int32_t>(nl * I_NINT)), star_i(ws.take<int32_t>(5 * n)), si(ws.take<int32_t>(J_NINT)) {}
};

}  // namespace

size_t cube_free_workspace_bytes(int ny, int nx, int nstar, int layers) {
    return workspace_bytes<CubeFreeWork>(ny, nx, nstar, layers);
}

void launch_fit_cube_free(hipStream_t s, int ny, int nx, int layers, const double* d_cube, const double* d_var,
                          StarList stars, const double* d_scale0, double radius, bool background, int max_iter,
                          double tol, int max_outer, double pos_tol, double max_step, double max_move, double min_snr,
                          double* d_star_out, double* d_head_out, double* d_pos_out, double* d_shift_out,
                          double* d_call_out, double* d_resid_out, void* d_ws) {
    WorkspaceCarver ws(d_ws);
    const CubeFreeWork w(ws, ny, nx, stars.nstar, layers);
    const int n = stars.nstar, nl = layers, back = background ? 1 : 0, nv = n + 1;
    const double r2 = radius * radius;
    const double* d_shift_in = stars.shift;
    stars.shift = w.wshift;                               // the stars follow the working shifts from here on
    int32_t *carry = w.layer_i, *carryl = w.layer_i + (size_t)nl * n;
    int32_t *freem = w.star_i, *nfree = freem + n, *sflag = nfree + n, *held = sflag + n, *seen = held + n;
    const CubeStep st{n, nl, back, w.nchunk, 0, tol * tol, min_snr, max_step, max_move, pos_tol, w.accept, w.stat,
                      w.ndisc, w.sump, w.shift0, w.wshift, w.x, w.r, w.p, w.diag, w.q3, w.g3, w.blk, w.blkl, w.f0, w.qd,
                      w.partial, w.partial_d, w.lw, w.sd, w.si, w.gate, carry, carryl, freem, nfree, sflag, held, seen,
                      nullptr, d_star_out, d_head_out, d_pos_out, d_shift_out, d_call_out};
    // the renderer's walk of all layers: out = in (nullptr: zeros) +- sum scale P~ over the accepted stars
    auto render = [&](const double* in, const double* scale, bool subtract, double* out, const int32_t* dn) {
        launch_render_walk_layers(s, ny, nx, nl, in, stars, scale, nv, w.accept, subtract, out, d_ws, dn, I_NINT);
    };
    auto project = [&](bool first, const double* V, const double* c, double csign, const int32_t* dn) {
        const FreeProjection io{w.W, V, d_cube, c, csign, w.accept, carry, dn, w.q3, w.g3, w.blk};
        if (first)
            hipLaunchKernelGGL((k_fr_project<true, true>), dim3(n, nl), dim3(kStarThreads), 0, s, ny, nx, stars, io);
        else
            hipLaunchKernelGGL((k_fr_project<false, true>), dim3(n, nl), dim3(kStarThreads), 0, s, ny, nx, stars, io);
    };
    auto reduce = [&](const double* V, const double* c, double csign, double* partial, const int32_t* dn) {
        hipLaunchKernelGGL(k_ff_reduce<true>, dim3(w.nchunk, nl), dim3(256), 0, s, w.npix, w.nchunk, w.W, V, c, nv, csign,
                           partial, dn);
    };
    auto step = [&](auto phase, int gn, const int32_t* word) {
        CubeStep a = st;
        a.gn = gn;
        a.word = word;
        hipLaunchKernelGGL(k_cf_step<decltype(phase)::value>, dim3(1), dim3(kStepThreads), 0, s, a);
    };
    const double* b = w.x + n;                            // the constant of layer 0, and its place in the direction p
    const double* pb = w.p + n;
    const double* delta = w.p + (size_t)nl * nv;          // the delta places of p
    // One solve at the working shifts from the F and b that stand in x (delta = 0): section 26's, every launch over
    // all layers, the gates per layer.  A Gauss-Newton step (gn) does nothing once the outer loop has ended, and moves
    // the stars at its end.
    auto solve = [&](int gn) {
        const int32_t* outer = gn ? w.gate + G_OUTER : nullptr;
        const int32_t* inner = w.gate + (gn ? G_GN : G_DONE);
        render(d_cube, w.x, true, w.M, outer);
        project(true, w.M, b, -1.0, outer);
        reduce(w.M, b, -1.0, w.partial, outer);
        reduce(d_cube, nullptr, 1.0, w.partial_d, outer);
        step(std::integral_constant<int, CF_JUDGE>{}, gn, nullptr);
        step(std::integral_constant<int, CF_INIT>{}, gn, nullptr);
        for (int it = 0; it < max_iter; ++it) {           // q = N p: one tile walk, one projection, one frame reduction
            hipLaunchKernelGGL(k_fr_walk<true>, dim3(w.lists.ntx, w.lists.nty, nl), dim3(kWThreads), 0, s, ny, nx, stars,
                               w.p, carry, w.lists.offset, w.lists.pairs, inner, w.M,
                               FreeLayers{w.f0, delta, w.accept, I_NINT});
            project(false, w.M, pb, 1.0, inner);
            if (back) reduce(w.M, pb, 1.0, w.partial, inner);
            step(std::integral_constant<int, CF_ITER>{}, gn, w.si + (gn ? J_GN : J_DONE));
        }
        if (gn) step(std::integral_constant<int, CF_APPLY>{}, gn, nullptr);
    };
    size_t nbegin = std::max<size_t>(w.nvec, 2 * (size_t)nl * n);
    nbegin = std::max<size_t>(nbegin, std::max<size_t>((size_t)nl * I_NINT, 5 * (size_t)n + 16));
    hipLaunchKernelGGL(k_cf_begin, dim3((unsigned)((nbegin + 255) / 256)), dim3(256), 0, s, n, nl, d_shift_in,
                       stars.lshift, w.shift0, w.wshift, w.x, w.nvec, w.star_i, w.layer_i, w.gate, w.sd, w.si,
                       max_outer == 0 ? 1 : 0);
    // section 25's lists (every placed star, from the geometry alone, sorted once), judging and weights, at the start
    // shifts, once
    launch_render_lists(s, ny, nx, stars, nullptr, nullptr, nullptr, d_ws);
    launch_render_sort(s, ny, nx, n, d_ws);
    hipLaunchKernelGGL((k_ff_star<false, true>), dim3(n, nl), dim3(kStarThreads), 0, s, ny, nx, stars, r2,
                       StarJudging{d_cube, d_var, d_scale0, w.accept, w.stat, w.ndisc, w.sump, w.diag, w.x});
    hipLaunchKernelGGL(k_ff_domain<true>, dim3(w.lists.ntx, w.lists.nty, nl), dim3(256), 0, s, ny, nx, d_cube, d_var,
                       stars, r2, w.lists.offset, w.lists.pairs, w.accept, w.W);
    if (max_outer > 0) solve(0);
    for (int t = 0; t < max_outer; ++t) solve(1);
    solve(0);
    // the residual cube by the renderer itself, chi2 from it, the overlap from N 1 over the flux columns
    double* R = d_resid_out ? d_resid_out : w.M;
    render(d_cube, w.x, true, R, nullptr);
    reduce(R, b, -1.0, w.partial, nullptr);
    hipLaunchKernelGGL(k_ff_ones, dim3((nl * nv + 255) / 256), dim3(256), 0, s, nl * nv, w.p);
    render(nullptr, w.p, false, w.M, nullptr);
    project(false, w.M, nullptr, 1.0, nullptr);
    step(std::integral_constant<int, CF_FINAL>{}, 0, nullptr);
}

}  // namespace mpsfr
