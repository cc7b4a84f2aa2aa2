// HIP kernel of the PSF energy metrics, written for gfx950 (MI355X, wave64).  See DESIGN.md section 16.
//
// K_STAMP_METRICS: per 40 x 40 stamp (float64 in and out, fp64 arithmetic in both precision modes) the flux, the
// brightest pixel, a centre (given, or the flux-weighted first moment), the encircled energy at up to 16 radii, the
// ensquared energy in up to 16 boxes and the radii that hold up to 16 fractions of the flux.  Pixel (p, q) is the unit
// square centred on (p, q), in the coordinates of the Moffat fits (p0, q0).
//
// One wave per stamp with the stamp in LDS, as the fit kernels hold it: lane (lr, lc) of an 8 x 8 cell owns pixel
// (8 mo + lr, 8 mi + lc) of the 5 x 5 blocks (the pixel map of the fits), kept at [5 mo + mi][lane] so that a sweep
// reads without bank conflicts.  (Held in registers, the 25 pixels of a lane plus the loop invariants of the unrolled
// sweeps spilled to scratch at any occupancy above one wave per SIMD.)  An encircled energy is one sweep -- a pixel
// whose farthest corner is inside the circle adds its value, one whose nearest point is outside adds nothing, both
// decided by a compare -- which queues the pixels the circle cuts (at most ~170: a circle crosses each of the 2 x 41
// grid lines twice) in LDS; the wave then takes the queue 64 pixels at a time, so that the exact overlap (four
// square roots and four arctangents per pixel) runs with all lanes busy instead of once per slot of the sweep.
// The same pass gives dEE/dr (the arc inside a pixel is the angle the overlap formula computes anyway), so the EE radii
// come from a bracketed Newton iteration.  Per-lane sums run in a fixed order and the wave sums on the DPP path of
// the fits (wave_total): a stamp's row depends on that stamp and the parameters only.  No atomics.
#include "device_common.h"
#include "fit_common.h"

namespace mpsfr {

namespace {

constexpr int NPXL = NS * NS / 64;           // pixels per lane
constexpr int MQ = 256;                      // queue of cut pixels (the geometry allows ~170)
constexpr double kCenterMax = 100.0;         // |cp|, |cq| bound of a centre (pixels); beyond it: status 2.  The overlap
                                             // area of a pixel is good to ~eps r^2 (1e-16 r^2 off the axes) and an EE
                                             // radius is searched up to the centre's distance: within this bound the
                                             // error of EE(r) stays below 1e-13 and the promise on R_k holds with a
                                             // factor 4 to spare
constexpr double kRootGoal = 2.0e-14;        // |EE(r) - f| at which the Newton iteration stops (Newton converges
                                             // quadratically: the step that gets below 1e-12 usually lands here)
constexpr double kRootTol = 5.0e-13;         // ... and above which the radius is flagged (the ABI promises 1e-12):
                                             // where this fp64 EE(r) is too coarse to settle -- the cancelling sums
                                             // of a stamp of mixed signs from sum |I| / flux ~1e4 on
constexpr int kRootMaxIt = 100;

struct MetricPar {
    double rad[METRIC_MAX];
    double box[METRIC_MAX];
    double frac[METRIC_MAX];
    int nrad, nbox, nfrac, pad;
};

// Area of the disc of radius r (r2 = r r) about the origin inside [0, x] x [0, y], for 0 <= x, y <= r, with
// xa = sqrt(r2 - y^2) and yb = sqrt(r2 - x^2): the rectangle when its corner is inside, else the two triangles
// (0, P1, (0,y)), (0, (x,0), P2) ... in closed form  (xa y + x yb) / 2 + r2 ang / 2, ang the angle of the arc between
// P2 = (x, yb) and P1 = (xa, y).  r ang is also d(area)/dr.
__device__ __forceinline__ double quadrant_area(double x, double y, double xa, double yb, double r2, double& ang) {
    if (x * x + y * y <= r2) {
        ang = 0.0;
        return x * y;
    }
    ang = atan2(x * y - yb * xa, x * xa + yb * y);
    return 0.5 * (xa * y + x * yb) + 0.5 * r2 * ang;
}

// Exact area of the unit pixel centred (ax, ay) >= 0 away from the centre of the circle (the pixel reflected into
// the first quadrant) inside the circle, by inclusion-exclusion over its corners:
// S(x1, y1) - S(x0, y1) - S(x1, y0) + S(x0, y0), S(x, y) = sgn(x) sgn(y) quadrant_area(min(|x|, r), min(|y|, r)).
// arc: the angle of the circle inside the pixel (d(area)/dr = r arc).
__device__ __forceinline__ double pixel_overlap(double ax, double ay, double r, double r2, double& arc) {
    const double x0 = ax - 0.5, y0 = ay - 0.5;
    const double X0 = fmin(fabs(x0), r), X1 = fmin(ax + 0.5, r), Y0 = fmin(fabs(y0), r), Y1 = fmin(ay + 0.5, r);
    const double yb0 = sqrt(fmax(r2 - X0 * X0, 0.0)), yb1 = sqrt(fmax(r2 - X1 * X1, 0.0));
    const double xa0 = sqrt(fmax(r2 - Y0 * Y0, 0.0)), xa1 = sqrt(fmax(r2 - Y1 * Y1, 0.0));
    const double sx = x0 < 0.0 ? 1.0 : -1.0, sy = y0 < 0.0 ? 1.0 : -1.0;     // signs of the x0 / y0 terms
    // (one corner at a time: four interleaved arctangents would cost the registers that hold the stamp)
    double area = 0.0;
    arc = 0.0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        const bool hx = c & 1, hy = c & 2;
        const double sg = (hx ? 1.0 : sx) * (hy ? 1.0 : sy);
        double ang;
        const double s = quadrant_area(hx ? X1 : X0, hy ? Y1 : Y0, hy ? xa1 : xa0, hx ? yb1 : yb0, r2, ang);
        area = fma(sg, s, area);
        arc = fma(sg, ang, arc);
    }
    return area;
}

// One wave's view of a stamp: the stamp in LDS ([25][64], see above) and the lane's cell coordinates
struct Lane {
    const double* sp;
    int lr, lc, lane;
};

// sum_pq A_circ(p, q; cp, cq, r) I_pq  (and, if DERIV, its derivative in r), on every lane.
// qo: the wave's queue in LDS (slots of L.sp).
template <bool DERIV>
__device__ __forceinline__ double circle_sum(const Lane& L, double cp, double cq, double r, int* qo, double* deriv) {
    const double r2 = r * r;
    double acc = 0.0, dacc = 0.0;
    const double dy0 = (double)L.lr - cp, dx0 = (double)L.lc - cq;
    // the sweep: whole pixels are added, cut pixels are queued in the order (m, lane)
    int count = 0;
#pragma unroll 1
    for (int m = 0; m < NPXL; ++m) {
        const int mo = m / 5, mi = m - 5 * mo;
        const double ay = fabs((double)(8 * mo) + dy0), ax = fabs((double)(8 * mi) + dx0);
        const double fx = ax + 0.5, fy = ay + 0.5;
        const double nx = fmax(ax - 0.5, 0.0), ny = fmax(ay - 0.5, 0.0);
        const bool in = fx * fx + fy * fy <= r2;
        const bool cut = !in && (nx * nx + ny * ny < r2);
        acc += in ? L.sp[m * 64 + L.lane] : 0.0;
        const unsigned long long mask = __ballot(cut);
        if (mask) {                                  // (wave-uniform)
            const int pos = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (cut && pos < MQ) qo[pos] = m * 64 + L.lane;
            count += __popcll(mask);
        }
    }
    __syncthreads();                 // (one wave: the queue entries other lanes wrote)
    if (count <= MQ) {
#pragma unroll 1
        for (int k = L.lane; k < count; k += 64) {
            const int o = qo[k], m = o >> 6, mo = m / 5, mi = m - 5 * mo, ln = o & 63;
            const double ay = fabs((double)(8 * mo + (ln >> 3)) - cp), ax = fabs((double)(8 * mi + (ln & 7)) - cq);
            double arc;
            const double a = pixel_overlap(ax, ay, r, r2, arc);
            const double v = L.sp[o];
            acc = fma(a, v, acc);
            if (DERIV) dacc = fma(arc, v, dacc);
        }
    } else {
        // more cut pixels than the queue holds (not reachable with a circle, kept for safety): every lane
        // evaluates its own cut pixels
#pragma unroll 1
        for (int m = 0; m < NPXL; ++m) {
            const int mo = m / 5, mi = m - 5 * mo;
            const double ay = fabs((double)(8 * mo) + dy0), ax = fabs((double)(8 * mi) + dx0);
            const double fx = ax + 0.5, fy = ay + 0.5;
            const double nx = fmax(ax - 0.5, 0.0), ny = fmax(ay - 0.5, 0.0);
            if (!(fx * fx + fy * fy <= r2) && nx * nx + ny * ny < r2) {
                double arc;
                const double a = pixel_overlap(ax, ay, r, r2, arc);
                const double v = L.sp[m * 64 + L.lane];
                acc = fma(a, v, acc);
                if (DERIV) dacc = fma(arc, v, dacc);
            }
        }
    }
    __syncthreads();                 // (the queue is refilled by the next call)
    if (DERIV) *deriv = r * wave_total(dacc);
    return wave_total(acc);
}

__global__ void __launch_bounds__(64)
k_stamp_metrics(int nstamp, const double* __restrict__ stamps, const double* __restrict__ centers, MetricPar P,
                double* __restrict__ out) {
    static_assert(NPXL * 64 == NS * NS && NS == 40, "5 x 5 blocks of 8 x 8 pixels");
    const int st = (int)blockIdx.x;
    if (st >= nstamp) return;
    __shared__ double sp_[NS * NS];
    __shared__ int qo[MQ];
    Lane L;
    L.sp = sp_;
    L.lane = threadIdx.x & 63;
    L.lr = L.lane >> 3;
    L.lc = L.lane & 7;
    const double* src = stamps + (size_t)st * NS * NS;
    const double* pl = src + L.lr * NS + L.lc;
    // flux, first moments, the brightest pixel (the first in row-major order: a lane's pixels come in that order)
    double s0 = 0.0, sp = 0.0, sq = 0.0, best = -INFINITY;
    int besto = NS * NS;
    bool finite = true;
#pragma unroll
    for (int m = 0; m < NPXL; ++m) {
        const int mo = m / 5, mi = m % 5;
        const double d = pl[mo * 8 * NS + mi * 8];
        sp_[m * 64 + L.lane] = d;
        finite = finite && (fabs(d) < INFINITY);           // (false for NaN too)
        s0 += d;
        sp = fma((double)(8 * mo + L.lr), d, sp);
        sq = fma((double)(8 * mi + L.lc), d, sq);
        if (d > best) { best = d; besto = (8 * mo + L.lr) * NS + 8 * mi + L.lc; }
    }
    wave_first_max(best, besto);
    if (besto >= NS * NS) besto = 0;                        // (no pixel compares: all NaN)
    const double flux = wave_total(s0);
    sp = wave_total(sp);
    sq = wave_total(sq);
    bool ok = __ballot(!finite) == 0ull && flux > 0.0 && flux < INFINITY;
    double cp, cq;
    if (centers) {
        cp = sgpr(centers[2 * (size_t)st]);
        cq = sgpr(centers[2 * (size_t)st + 1]);
        ok = ok && fabs(cp) <= kCenterMax && fabs(cq) <= kCenterMax;       // (false for NaN)
    } else {
        cp = ok ? sp / flux : NAN;
        cq = ok ? sq / flux : NAN;
        ok = ok && fabs(cp) <= kCenterMax && fabs(cq) <= kCenterMax;       // (a stamp of mixed signs)
    }
    const int nout = METRIC_HEAD + P.nrad + P.nbox + P.nfrac;
    double* o = out + (size_t)st * nout;
    if (L.lane == 0) {
        o[0] = flux;
        o[1] = best;
        o[2] = (double)(besto / NS);
        o[3] = (double)(besto % NS);
        o[4] = cp;
        o[5] = cq;
        o[7] = 0.0;
    }
    if (!ok) {                                              // (wave-uniform)
        if (L.lane == 0) o[6] = 2.0;
        for (int k = L.lane; k < nout - METRIC_HEAD; k += 64) o[METRIC_HEAD + k] = NAN;
        return;
    }
    const double iflux = 1.0 / flux;
    int status = 0;
    // encircled energy
#pragma unroll 1
    for (int k = 0; k < P.nrad; ++k) {
        const double e = circle_sum<false>(L, cp, cq, P.rad[k], qo, nullptr) * iflux;
        if (L.lane == 0) o[METRIC_HEAD + k] = e;
    }
    // ensquared energy: overlap length in p times overlap length in q
#pragma unroll 1
    for (int k = 0; k < P.nbox; ++k) {
        const double hs = 0.5 * P.box[k];
        const double plo = cp - hs, phi = cp + hs, qlo = cq - hs, qhi = cq + hs;
        double acc = 0.0;
#pragma unroll 1
        for (int m = 0; m < NPXL; ++m) {
            const int mo = m / 5, mi = m - 5 * mo;
            const double p = (double)(8 * mo + L.lr), q = (double)(8 * mi + L.lc);
            const double wp = fmax(fmin(p + 0.5, phi) - fmax(p - 0.5, plo), 0.0);
            const double wq = fmax(fmin(q + 0.5, qhi) - fmax(q - 0.5, qlo), 0.0);
            acc = fma(wp * wq, sp_[m * 64 + L.lane], acc);
        }
        const double e = wave_total(acc) * iflux;
        if (L.lane == 0) o[METRIC_HEAD + P.nrad + k] = e;
    }
    // EE radii: Newton on EE(r) - f inside a bracket [lo, hi] that every evaluation shrinks (a step that leaves
    // it, or a slope that is not positive, is replaced by the midpoint), from the radius at which a disc as bright
    // as the peak holds the fraction
    const double rmax = hypot(fmax(cp + 0.5, (double)NS - 0.5 - cp), fmax(cq + 0.5, (double)NS - 0.5 - cq));
#pragma unroll 1
    for (int k = 0; k < P.nfrac; ++k) {
        const double f = P.frac[k];
        double lo = 0.0, hi = rmax;
        double r = sqrt(f * flux / (kPi * fmax(best, flux / (double)(NS * NS))));
        if (!(r > lo && r < hi)) r = 0.5 * (lo + hi);
        double g = 0.0;
#pragma unroll 1
        for (int it = 0; it < kRootMaxIt; ++it) {
            double d;
            g = circle_sum<true>(L, cp, cq, r, qo, &d) * iflux - f;
            if (fabs(g) <= kRootGoal) break;
            if (g < 0.0) lo = r; else hi = r;
            double rn = r - g / (d * iflux);
            if (!(d > 0.0) || !(rn > lo && rn < hi)) rn = 0.5 * (lo + hi);
            // (rn == r: the bracket is down to neighbouring numbers; r stays the radius g belongs to)
            if (rn == r || !(hi > lo) || it == kRootMaxIt - 1) break;
            r = rn;
        }
        if (!(fabs(g) <= kRootTol)) status = 1;
        if (L.lane == 0) o[METRIC_HEAD + P.nrad + P.nbox + k] = r;
    }
    if (L.lane == 0) o[6] = (double)status;
}

}  // namespace

void launch_stamp_metrics(hipStream_t s, int nstamp, const double* d_stamps, const double* d_centers, int nrad,
                          const double* radii, int nbox, const double* boxes, int nfrac, const double* fractions,
                          double* d_out) {
    if (nstamp <= 0) return;
    MetricPar P = {};
    P.nrad = nrad; P.nbox = nbox; P.nfrac = nfrac;
    for (int k = 0; k < nrad; ++k) P.rad[k] = radii[k];
    for (int k = 0; k < nbox; ++k) P.box[k] = boxes[k];
    for (int k = 0; k < nfrac; ++k) P.frac[k] = fractions[k];
    // one wavefront (and workgroup) per stamp, as the fits
    hipLaunchKernelGGL(k_stamp_metrics, dim3(nstamp), dim3(64), 0, s, nstamp, d_stamps, d_centers, P, d_out);
}

}  // namespace mpsfr
