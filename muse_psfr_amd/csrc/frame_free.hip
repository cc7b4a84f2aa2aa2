// Crowded-field PSF photometry with free positions (mpsfr_fit_frame_psf_free, include/mpsfr.h):
// Gauss-Newton around the solve of frame_fit_impl.h.  Omega, the valid pixels and the accepted stars are those of the
// start shifts (k_ff_star<false>, k_ff_domain: section 24's, unchanged) and stay; the shifts live in work memory, where
// StarList::shift points.  Every solve -- the opening one, the Gauss-Newton steps, the closing one -- is Jacobi-
// preconditioned conjugate gradients over the 3 nstar + 1 unknowns (F [nstar], a [nstar], c [nstar], b) with a live
// mask: a held star has its F alone, a free star F, a = F delta_y and c = F delta_x on the columns P~, dP~/ds_y, dP~/ds_x.
//   k_fr_begin     the working shifts, the counters and the scalars of a call
//   k_fr_walk      the three-column tile walk and
//   k_fr_project   the three-column projection with the star's 3 x 3 block of N: frame_free_impl.h, which the cube form
//                  (cube_free.hip) shares; here in their LAYERS = false forms
//   k_fr_step      one workgroup: FR_INIT (who is free, the live mask, the first residual, the stop reference),
//                  FR_ITER (a conjugate-gradient step), FR_APPLY (delta = (a, c) / F, its clips, the new shifts, the
//                  outer done word), FR_FINAL (the rows)
// k_ff_reduce, k_ff_ones and the renderer's own walk (first residuals, the residual frame, the overlap) are reused as
// they are.  FR_ITER is cg_step, the rows and the head star_row and solve_head (frame_fit_impl.h); the carry rule, a
// place of the first residual and the position update are frame_free_impl.h's, which k_cf_step shares.  Every sum has
// a fixed order, all arithmetic is fp64, nothing waits for the host.
#include "frame_free_impl.h"

namespace mpsfr {
namespace {

constexpr int NFREE = 16;                                     // MPSFR_NFRAMEFREE; the head: MPSFR_NFRAMEFREE_HEAD = 12

// the scalars of a call: the shared ones (frame_free_impl.h), then the frame's own
enum { D_WSUM = D_SHARED, D_NDOUBLE };
enum { J_NONE = J_SHARED, J_NACC, J_NOMEGA, J_NINT };

// v, computed here and now: the sums of FR_INIT's reductions one after the other, not all their partials held at once
__device__ __forceinline__ double settled(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(256) void k_fr_begin(int n, const double* __restrict__ shift_in, double* __restrict__ shift0,
                                                  double* __restrict__ wshift, double* __restrict__ x,
                                                  int32_t* __restrict__ freem, int32_t* __restrict__ nfree,
                                                  int32_t* __restrict__ sflag, int32_t* __restrict__ held,
                                                  double* __restrict__ sd, int32_t* __restrict__ si, int posok) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * n) {
        const double v = shift_in ? shift_in[i] : 0.0;
        shift0[i] = v;
        wshift[i] = v;
    }
    if (i <= 3 * n) x[i] = 0.0;
    if (i < n) {
        freem[i] = 0;
        nfree[i] = 0;
        sflag[i] = 0;
        held[i] = 0;
    }
    if (i < D_NDOUBLE) sd[i] = 0.0;
    if (i < J_NINT) si[i] = i == J_POSOK ? posok : 0;
}

enum { FR_INIT = 0, FR_ITER, FR_APPLY, FR_FINAL };

struct FreeStep {
    int n, back, nchunk, gn;                  // gn: a Gauss-Newton step (else the positions are held)
    double tol2, min_snr, max_step, max_move, pos_tol;
    const int32_t *accept, *stat;
    const double *ndisc, *sump, *shift0;
    double *wshift, *x, *r, *p, *q, *g, *diag, *blk, *blkl;
    const double *partial, *partial_d;
    double* sd;
    int32_t *si, *freem, *nfree, *sflag, *held;
    const int32_t* gate;                      // FR_ITER: the done word of its solve
    double *star_out, *shift_out, *head_out;
};

// One workgroup over the nu = 3 n + 1 unknowns: F of star k at k, a at n + k, c at 2 n + k, the constant last.
template <int PHASE>
__global__ __launch_bounds__(kStepThreads) void k_fr_step(FreeStep a) {
    __shared__ double part[kStepThreads / 64];
    const int tid = threadIdx.x, n = a.n, nb = 3 * n;
    double* const sd = a.sd;
    int32_t* const si = a.si;
    // the star and the column of unknown i < 3 n
    auto star_of = [&](int i) { return i < n ? i : (i < 2 * n ? i - n : i - 2 * n); };
    if constexpr (PHASE == FR_INIT) {
        if (a.gn && si[J_OUTER]) return;
        const double gb = settled(step_sum(a.partial, a.nchunk, part));
        const double wsum = settled(step_sum(a.partial + a.nchunk, a.nchunk, part));
        const double chi0 = settled(step_sum(a.partial + 2 * (size_t)a.nchunk, a.nchunk, part));
        const double nomega = settled(step_sum(a.partial + 3 * (size_t)a.nchunk, a.nchunk, part));
        const double gd = settled(step_sum(a.partial_d, a.nchunk, part));
        double na = 0.0;
        for (int i = tid; i < n; i += kStepThreads) na += a.accept[i] ? 1.0 : 0.0;
        const double nacc = settled(block_sum<kStepThreads>(na, part));
        const double back = a.back ? 1.0 : 0.0;
        const bool none = nacc < 1.0 || nomega < nacc + back + 1.0;
        // (no star moves unless the pixels of Omega outnumber the unknowns with every star free: dof >= 1 at the end)
        const bool movable = a.gn && !none && nomega >= 3.0 * nacc + back + 1.0;
        const double s2 = none ? 0.0 : chi0 / (nomega - nacc - back);
        double nf = 0.0;
#pragma unroll 1
        for (int k = tid; k < n; k += kStepThreads) {
            const bool acc = !none && a.accept[k] != 0;
            const double* b = a.blk + (size_t)B_N * k;
            const bool fr = movable && acc && carries(a.x[k], b, s2, a.min_snr);
            a.freem[k] = fr ? 1 : 0;
            if (a.gn) {
                a.held[k] = acc && !fr ? 1 : 0;
                if (fr) {
                    a.nfree[k] += 1;
                    for (int j = 0; j < B_N; ++j) a.blkl[(size_t)B_N * k + j] = b[j];
                }
            }
            nf += fr ? 1.0 : 0.0;
        }
        const double nfr = block_sum<kStepThreads>(nf, part);        // (its barriers publish freem to the workgroup)
        double rz = 0.0, gz = 0.0;
#pragma unroll 1
        for (int i = tid; i <= nb; i += kStepThreads) {
            bool on;
            double d, ri, gi;
            if (i == nb) {
                on = !none && a.back;
                d = wsum;
                ri = gb;
                gi = gd;
            } else {
                const int k = star_of(i), col = i / n;
                on = !none && (col == 0 ? a.accept[k] != 0 : a.freem[k] != 0);
                d = on ? a.blk[(size_t)B_N * k + col] : 1.0;
                ri = on ? a.q[i] : 0.0;
                gi = on ? a.g[i] : 0.0;
            }
            if (none || (i >= n && i < nb)) a.x[i] = 0.0;      // a = c = 0 at the start of every solve
            first_place(on, d, ri, gi, a.diag, a.r, a.p, i, rz, gz);
        }
        const double rho = block_sum<kStepThreads>(rz, part);
        const double rhog = block_sum<kStepThreads>(gz, part);
        if (tid == 0) {
            si[J_NONE] = none ? 1 : 0;
            si[J_NACC] = (int)nacc;
            si[J_NOMEGA] = (int)nomega;
            sd[D_WSUM] = wsum;
            if (a.gn) si[J_NFREE] = (int)nfr;
            if (a.gn && nfr < 1.0) {                   // no star is free: the outer loop ends here, nothing to move
                si[J_OUTER] = 1;
                si[J_GN] = 1;
                si[J_POSOK] = 1;
            } else {
                const bool stop = rho <= a.tol2 * rhog;
                const bool more = !none && !stop && positive_finite(rho) && positive_finite(rhog);
                sd[D_RHO] = rho;
                sd[D_RHOG] = rhog;
                sd[D_REL] = positive_finite(rhog) ? sqrt(rho / rhog) : 0.0;
                si[J_DONE] = more ? 0 : 1;
                si[J_GN] = more ? 0 : 1;
                si[J_ITER] = 0;
                si[J_STOP] = stop ? 0 : 1;             // 1 until the stop test passes
            }
        }
    } else if constexpr (PHASE == FR_ITER) {
        if (*a.gate) return;
        const double rhog = sd[D_RHOG];
        auto live = [&](int i) {
            if (i == nb) return a.back != 0;
            return i < n ? a.accept[i] != 0 : a.freem[star_of(i)] != 0;
        };
        const CgEnd e = cg_step(nb + (a.back ? 1 : 0), a.back != 0, live, a.x, a.r, a.p, a.q, a.diag, a.partial,
                                a.nchunk, sd[D_RHO], rhog, a.tol2, part);
        if (tid == 0) free_iter_end(e, rhog, sd, si);
    } else if constexpr (PHASE == FR_APPLY) {
        if (si[J_OUTER]) return;
        double md = 0.0;
        for (int k = tid; k < n; k += kStepThreads) {
            if (!a.freem[k]) continue;
            const double F = a.x[k];
            const bool ok = positive_finite(F);
            int flag = 0;
            for (int ax = 0; ax < 2; ++ax) {
                double absd;
                a.wshift[2 * k + ax] = move_shift(ok ? a.x[(ax + 1) * n + k] / F : 0.0, a.wshift[2 * k + ax],
                                                  a.shift0[2 * k + ax], a.max_step, a.max_move, -kPsfMaxShift,
                                                  kPsfMaxShift, flag, absd);
                md = fmax(md, absd);
            }
            a.sflag[k] = flag;
        }
        outer_end(md, a.pos_tol, sd, si, part);
    } else {
        const bool none = si[J_NONE] != 0;
        const int nacc = si[J_NACC], nomega = si[J_NOMEGA];
        double ne = 0.0;
        for (int k = tid; k < n; k += kStepThreads) ne += a.nfree[k] > 0 ? 1.0 : 0.0;
        const double ever = block_sum<kStepThreads>(ne, part);
        const double chi2 = step_sum(a.partial + 2 * (size_t)a.nchunk, a.nchunk, part);
        const double dof = (double)nomega - (double)nacc - 2.0 * ever - (a.back ? 1.0 : 0.0);
        const double s2 = none ? 0.0 : chi2 / dof;
        for (int k = tid; k < n; k += kStepThreads) {
            double* o = a.star_out + (size_t)NFREE * k;
            const bool on = !none && a.accept[k] != 0;
            const double F = star_row(o, on, a.x[k], a.diag[k], a.q[k], s2, a.sump[k], a.ndisc[k], a.stat[k]);
            const double sy = a.wshift[2 * k], sx = a.wshift[2 * k + 1];
            o[8] = sy;
            o[9] = sx;
            double ey = 0.0, ex = 0.0;
            if (on && a.nfree[k] > 0 && positive_finite(F)) {
                // the star's own 3 x 3 block of N from its last free step, inverted: the places of a and c
                const double* b = a.blkl + (size_t)B_N * k;
                const double ff = b[B_FF], aa = b[B_AA], cc = b[B_CC], fa = b[B_FA], fc = b[B_FC], ac = b[B_AC];
                const double det = ff * (aa * cc - ac * ac) - fa * (fa * cc - ac * fc) + fc * (fa * ac - aa * fc);
                const double vy = (ff * cc - fc * fc) / det * s2, vx = (ff * aa - fa * fa) / det * s2;
                ey = positive_finite(vy) ? sqrt(vy) / F : 0.0;
                ex = positive_finite(vx) ? sqrt(vx) / F : 0.0;
            }
            o[10] = ey;
            o[11] = ex;
            o[12] = on ? sy - a.shift0[2 * k] : 0.0;
            o[13] = on ? sx - a.shift0[2 * k + 1] : 0.0;
            o[14] = on ? (double)(a.sflag[k] | (a.held[k] ? FLAG_HELD : 0)) : 0.0;
            o[15] = on ? (double)a.nfree[k] : 0.0;
            a.shift_out[2 * k] = sy;
            a.shift_out[2 * k + 1] = sx;
        }
        if (tid == 0) {
            double* h = a.head_out;
            solve_head(h, a.back != 0, none, a.x[nb], s2, sd[D_WSUM], chi2, (double)nomega, (double)si[J_ITER],
                       sd[D_REL], (double)nacc);
            h[7] = none ? 2.0 : (si[J_STOP] == 0 && si[J_POSOK] != 0 ? 0.0 : 1.0);
            h[8] = (double)si[J_NOUTER];
            h[9] = sd[D_MAXD];
            h[10] = (double)si[J_NFREE];
            h[11] = (double)si[J_ITERSUM];
        }
    }
}

// The workspace of a call: the renderer's lists (at its start); the frames W and M; x, r, p, q, g, diag [3 nstar + 1];
// the blocks of N now and of each star's last free step [6 nstar] each; ndisc, sump [nstar]; the start and the working
// shifts [2 nstar] each; the partials of the frame reductions [2][4][chunks]; the scalars; accept, stat, freem, nfree,
// sflag, held [nstar]
struct FrameFreeWork {
    RenderLists lists;
    size_t npix, n, nu;
    int nchunk;
    double *W, *M, *x, *r, *p, *q, *g, *diag, *blk, *blkl, *ndisc, *sump, *shift0, *wshift, *partial, *partial_d, *sd;
    int32_t *si, *accept, *stat, *freem, *nfree, *sflag, *held;
    FrameFreeWork(WorkspaceCarver& ws, int ny, int nx, int nstar)
        : lists(ws, ny, nx, nstar), npix((size_t)ny * nx), n((size_t)nstar), nu(3 * n + 1),
          nchunk((int)((npix + kChunk - 1) / kChunk)), W(ws.take<double>(npix)), M(ws.take<double>(npix)),
          x(ws.take<double>(nu)), r(ws.take<double>(nu)), p(ws.take<double>(nu)), q(ws.take<double>(nu)),
          g(ws.take<double>(nu)), diag(ws.take<double>(nu)), blk(ws.take<double>(B_N * n)),
          blkl(ws.take<double>(B_N * n)), ndisc(ws.take<double>(n)), sump(ws.take<double>(n)),
          shift0(ws.take<double>(2 * n)), wshift(ws.take<double>(2 * n)), partial(ws.take<double>(4 * (size_t)nchunk)),
          partial_d(ws.take<double>(4 * (size_t)nchunk)), sd(ws.take<double>(D_NDOUBLE)), si(ws.take<int32_t>(J_NINT)),
          accept(ws.take<int32_t>(n)), stat(ws.take<int32_t>(n)), freem(ws.take<int32_t>(n)),
          nfree(ws.take<int32_t>(n)), sflag(ws.take<int32_t>(n)), held(ws.take<int32_t>(n)) {}
};

}  // namespace

size_t frame_free_workspace_bytes(int ny, int nx, int nstar) { return workspace_bytes<FrameFreeWork>(ny, nx, nstar); }

void launch_fit_frame_free(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, StarList stars,
                           const double* d_scale0, double radius, bool background, int max_iter, double tol,
                           int max_outer, double pos_tol, double max_step, double max_move, double min_snr,
                           double* d_star_out, double* d_shift_out, double* d_head_out, double* d_resid_out,
                           void* d_ws) {
    WorkspaceCarver ws(d_ws);
    const FrameFreeWork w(ws, ny, nx, stars.nstar);
    const int n = stars.nstar, back = background ? 1 : 0, nu = 3 * n + 1;
    const double r2 = radius * radius;
    const double* d_shift_in = stars.shift;
    stars.shift = w.wshift;                               // the stars follow the working shifts from here on
    FreeStep st{n, back, w.nchunk, 0, tol * tol, min_snr, max_step, max_move, pos_tol, w.accept, w.stat, w.ndisc,
                w.sump, w.shift0, w.wshift, w.x, w.r, w.p, w.q, w.g, w.diag, w.blk, w.blkl, w.partial, w.partial_d,
                w.sd, w.si, w.freem, w.nfree, w.sflag, w.held, nullptr, d_star_out, d_shift_out, d_head_out};
    auto project = [&](bool first, const double* V, const double* c, double csign, const int32_t* dn) {
        const FreeProjection io{w.W, V, d_image, c, csign, w.accept, w.freem, dn, w.q, w.g, w.blk};
        if (first)
            hipLaunchKernelGGL((k_fr_project<true, false>), dim3(n), dim3(kStarThreads), 0, s, ny, nx, stars, io);
        else
            hipLaunchKernelGGL((k_fr_project<false, false>), dim3(n), dim3(kStarThreads), 0, s, ny, nx, stars, io);
    };
    auto reduce = [&](const double* V, const double* c, double csign, double* partial, const int32_t* dn) {
        hipLaunchKernelGGL(k_ff_reduce<false>, dim3(w.nchunk), dim3(256), 0, s, w.npix, w.nchunk, w.W, V, c, nu, csign,
                           partial, dn);
    };
    auto step = [&](auto phase, int gn, const int32_t* gate) {
        FreeStep a = st;
        a.gn = gn;
        a.gate = gate;
        hipLaunchKernelGGL(k_fr_step<decltype(phase)::value>, dim3(1), dim3(kStepThreads), 0, s, a);
    };
    const double* b = w.x + 3 * n;                        // the constant, and its place in the direction p
    const double* pb = w.p + 3 * n;
    // One solve at the working shifts from the F and b that stand in x (a = c = 0): the first residual by the renderer,
    // its projection with that of the data and the blocks of N, the two frame reductions; then the iterations.  A
    // Gauss-Newton step (gn) does nothing once the outer loop has ended, and moves the stars at its end.
    auto solve = [&](int gn) {
        const int32_t* outer = gn ? w.si + J_OUTER : nullptr;
        const int32_t* inner = w.si + (gn ? J_GN : J_DONE);
        launch_render_walk(s, ny, nx, d_image, stars, w.x, true, w.M, d_ws, outer);
        project(true, w.M, b, -1.0, outer);
        reduce(w.M, b, -1.0, w.partial, outer);
        reduce(d_image, nullptr, 1.0, w.partial_d, outer);
        step(std::integral_constant<int, FR_INIT>{}, gn, nullptr);
        for (int it = 0; it < max_iter; ++it) {           // q = N p: one tile walk, one projection, one frame reduction
            hipLaunchKernelGGL(k_fr_walk<false>, dim3(w.lists.ntx, w.lists.nty), dim3(kWThreads), 0, s, ny, nx, stars,
                               w.p, w.freem, w.lists.offset, w.lists.pairs, inner, w.M, NoFreeLayers{});
            project(false, w.M, pb, 1.0, inner);
            if (back) reduce(w.M, pb, 1.0, w.partial, inner);
            step(std::integral_constant<int, FR_ITER>{}, gn, inner);
        }
        if (gn) step(std::integral_constant<int, FR_APPLY>{}, gn, nullptr);
    };
    const int nbegin = 3 * n + 1 > J_NINT ? 3 * n + 1 : J_NINT;
    hipLaunchKernelGGL(k_fr_begin, dim3((nbegin + 255) / 256), dim3(256), 0, s, n, d_shift_in, w.shift0, w.wshift, w.x,
                       w.freem, w.nfree, w.sflag, w.held, w.sd, w.si, max_outer == 0 ? 1 : 0);
    // section 24's judging, lists and weights, at the start shifts, once; the lists sorted once for k_fr_walk
    hipLaunchKernelGGL((k_ff_star<false, false>), dim3(n), dim3(kStarThreads), 0, s, ny, nx, stars, r2,
                       StarJudging{d_image, d_var, d_scale0, w.accept, w.stat, w.ndisc, w.sump, w.diag, w.x});
    launch_render_lists(s, ny, nx, stars, nullptr, w.accept, nullptr, d_ws);
    launch_render_sort(s, ny, nx, n, d_ws);
    hipLaunchKernelGGL(k_ff_domain<false>, dim3(w.lists.ntx, w.lists.nty), dim3(256), 0, s, ny, nx, d_image, d_var,
                       stars, r2, w.lists.offset, w.lists.pairs, w.accept, w.W);
    if (max_outer > 0) solve(0);
    for (int t = 0; t < max_outer; ++t) solve(1);
    solve(0);
    // the residual frame by the renderer itself, chi2 from it, the overlap from N 1 over the flux columns
    double* R = d_resid_out ? d_resid_out : w.M;
    launch_render_walk(s, ny, nx, d_image, stars, w.x, true, R, d_ws, nullptr);
    reduce(R, b, -1.0, w.partial, nullptr);
    hipLaunchKernelGGL(k_ff_ones, dim3((n + 255) / 256), dim3(256), 0, s, n, w.p);
    launch_render_walk(s, ny, nx, nullptr, stars, w.p, false, w.M, d_ws, nullptr);
    project(false, w.M, nullptr, 1.0, nullptr);
    step(std::integral_constant<int, FR_FINAL>{}, 0, nullptr);
}

}  // namespace mpsfr
