// The star finder: matched-filter detection on a frame with the core of a model stamp.
//   k_find_core    the (2 half + 1)^2 core K of the model stamp and its squares, as a table every later kernel reads
//                  through uniform loads
//   k_find_map     one workgroup per 32 x 32 frame tile: w and w D of the tile and its `half` apron go into LDS, every
//                  thread keeps four adjacent pixels of one row in registers, so that one LDS read and one uniform load
//                  of K serve up to four pixels; writes the statistic T
//   k_find_peaks   one workgroup per tile: T with a `sep` apron in LDS, the peak rule, one 32-bit mask per (frame row,
//                  tile column) segment by a half-wave ballot
//   k_find_count   the peaks of every chunk of kChunkSegs segments (segments in (row, tile column) order: pixel order)
//   k_scan_counts  exclusive scan of the chunk counts (render.hip, one workgroup)
//   k_find_list    one thread per four segments: its place in pixel order from the chunk's offset and a scan inside the
//                  chunk, then the pixel index of every peak below max_stars into a list
//   k_find_rows    one wave per listed peak: the window into LDS, the sums again, in the same order by the same code,
//                  the parabola out of T and the sharpness out of the frame
//   k_find_fill    the filler rows from the count up to max_stars
// Every pixel's sums run over the window in row-major tap order with the same operations, whatever its place in a tile:
// the rows depend on the frame alone.  fp64 in both precision modes; no atomics at all.
#include "frame_common.h"

namespace mpsfr {
namespace {

// (the bits of a mask word, k_find_peaks' half-wave ballot: the renderer's kFrameTile by value, not by construction)
constexpr int kTile = 32;                                     // frame tile side
constexpr int kTileThreads = 256;
constexpr int kTilePix = kTile * kTile / kTileThreads;        // pixels per thread: adjacent rows of one column
constexpr int kMaxHalf = 8, kMaxSep = 16;                     // MPSFR_FIND_MAX_HALF, MPSFR_FIND_MAX_SEP
constexpr int kMaxTaps = (2 * kMaxHalf + 1) * (2 * kMaxHalf + 1);
constexpr int kMapQ = (kTile + 2 * kMaxHalf) / 4;             // LDS of the map kernel: doubles of a row in one plane,
constexpr int kMapPlane = (kTile + 2 * kMaxHalf) * kMapQ + 8;  // and the pitch of the four planes (map_index)
constexpr int kPeakStride = kTile + 2 * kMaxSep;
constexpr int kChunkThreads = 256, kThreadSegs = 4, kChunkSegs = kChunkThreads * kThreadSegs;
constexpr int kRowThreads = 64, kRowBlocks = 8192;                // k_find_rows: one wave per peak, blocks striding over them
static_assert(kTilePix == 4 && kTileThreads / kTile * kTilePix == kTile, "tile layout");

// The pixel rule of the observed fits on frame pixel (Y, X): weight w (0 on a masked pixel or off the frame), datum d
// (0 there) and their product.
__device__ __forceinline__ void find_pixel(int ny, int nx, const double* __restrict__ image,
                                           const double* __restrict__ var, int Y, int X, double& w, double& d,
                                           double& wd) {
#pragma clang fp contract(off)
    const bool in = (unsigned)Y < (unsigned)ny && (unsigned)X < (unsigned)nx;
    const size_t i = in ? (size_t)Y * nx + (size_t)X : 0;
    const double dv = image[i];
    const double vv = var ? var[i] : 1.0;
    const bool ok = in && fabs(dv) < __builtin_inf() && vv > 0.0 && vv < __builtin_inf();
    w = ok ? 1.0 / vv : 0.0;
    d = ok ? dv : 0.0;
    wd = w * d;
}

// The five sums of one pixel; a tap adds to them in this order with these operations, here and in k_find_rows
struct FindSums {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    int nvalid = 0;
    __device__ __forceinline__ void tap(double w, double wd, double k, double k2) {
        s0 += w;
        s1 = fma(w, k, s1);
        s2 = fma(w, k2, s2);
        s3 += wd;
        s4 = fma(wd, k, s4);
        nvalid += w != 0.0 ? 1 : 0;
    }
};

// amplitude, background and statistic out of the sums; T is NaN where it is not defined
__device__ __forceinline__ void find_stat(const FindSums& s, bool centre, int ntap, bool usevar, double& T, double& H,
                                          double& b) {
#pragma clang fp contract(off)
    const double den = s.s2 - s.s1 * s.s1 / s.s0;
    H = (s.s4 - s.s1 * s.s3 / s.s0) / den;
    b = (s.s3 - H * s.s1) / s.s0;
    const bool ok = centre && 2 * s.nvalid > ntap && den > 0.0;
    T = ok ? (usevar ? H * sqrt(den) : H) : __builtin_nan("");
}

__global__ __launch_bounds__(kTileThreads) void k_find_core(const double* __restrict__ psf, int half,
                                                            double* __restrict__ kk) {
    const int W = 2 * half + 1, first = (NS / 2 - half) * (NS + 1);
    // A core that cannot be a filter (a value that is not finite, or all values equal, where den is 0 up to rounding)
    // becomes NaN: every T is NaN then and the frame has no peak.
    int differ = 0, bad = 0;
    for (int i = threadIdx.x; i < W * W; i += kTileThreads) {
        const double k = psf[first + (i / W) * NS + i % W];
        differ |= k != psf[first];
        bad |= !(fabs(k) < __builtin_inf());
    }
    differ = __syncthreads_or(differ);
    bad = __syncthreads_or(bad);
    for (int i = threadIdx.x; i < W * W; i += kTileThreads) {
        const double k = differ && !bad ? psf[first + (i / W) * NS + i % W] : __builtin_nan("");
        kk[i] = k;
        kk[kMaxTaps + i] = k * k;
    }
}

// LDS place of the staged pixel (si, sj): four planes by sj mod 4, so that the threads of a tile row, which hold four
// adjacent columns each, read consecutive doubles; the plane pitch keeps the four planes on different banks.
__device__ __forceinline__ int map_index(int si, int sj) { return (sj & 3) * kMapPlane + si * kMapQ + (sj >> 2); }

__global__ __launch_bounds__(kTileThreads) void k_find_map(int ny, int nx, const double* __restrict__ image,
                                                           const double* __restrict__ var,
                                                           const double* __restrict__ kk, int half,
                                                           double* __restrict__ tmap) {
    __shared__ double sw[4 * kMapPlane], swd[4 * kMapPlane];
    const int tid = threadIdx.x, lane = tid & 63;
    // a thread holds four adjacent columns of one tile row; the 32 lanes that read LDS together hold the rows 0, 2, 4, 6
    // (or 1, 3, 5, 7) of the wave's eight: 96-byte rows two apart fall on different banks
    const int cx = 4 * (lane & 7), ry = 8 * (tid >> 6) + 2 * ((lane >> 3) & 3) + (lane >> 5);
    const int Y0 = blockIdx.y * kTile, X0 = blockIdx.x * kTile;
    const int W = 2 * half + 1, S = kTile + 2 * half;
    for (int e = tid; e < S * S; e += kTileThreads) {
        const int si = e / S, sj = e - si * S;
        double w, d, wd;
        find_pixel(ny, nx, image, var, Y0 - half + si, X0 - half + sj, w, d, wd);
        sw[map_index(si, sj)] = w;
        swd[map_index(si, sj)] = wd;
    }
    __syncthreads();
    FindSums acc[kTilePix];
    // Staged column cx + c of row ry + a is tap (a, c - j) of pixel j: rows outer, columns inner is the row-major tap
    // order of every pixel, and the four taps of a step are four adjacent values of one row of K, which slide through
    // k0 .. k3 -- one uniform load of K and K^2 per step
    for (int a = 0; a < W; ++a) {
        const int rowbase = (ry + a) * kMapQ + (cx >> 2);
        const double* ka = kk + a * W;
        double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        for (int c = 0; c < W + kTilePix - 1; ++c) {
            const int o = (c & 3) * kMapPlane + rowbase + (c >> 2);
            const double w = sw[o], wd = swd[o];
            k3 = k2, k2 = k1, k1 = k0, k0 = ka[min(c, W - 1)];
            q3 = q2, q2 = q1, q1 = q0, q0 = ka[kMaxTaps + min(c, W - 1)];
            if (c < W) acc[0].tap(w, wd, k0, q0);
            if (c >= 1 && c < W + 1) acc[1].tap(w, wd, k1, q1);
            if (c >= 2 && c < W + 2) acc[2].tap(w, wd, k2, q2);
            if (c >= 3) acc[3].tap(w, wd, k3, q3);
        }
    }
    const int Y = Y0 + ry;
#pragma unroll
    for (int j = 0; j < kTilePix; ++j) {
        const int X = X0 + cx + j;
        const bool centre = sw[map_index(ry + half, cx + j + half)] != 0.0;
        double T, H, b;
        find_stat(acc[j], centre, W * W, var != nullptr, T, H, b);
        if (Y < ny && X < nx) tmap[(size_t)Y * nx + X] = T;
    }
}

__global__ __launch_bounds__(kTileThreads) void k_find_peaks(int ny, int nx, int ntx, const double* __restrict__ tmap,
                                                             int sep, double threshold, uint32_t* __restrict__ mask) {
    // st: T of the tile and its apron, -infinity where it is not finite or off the frame; rmax: for every staged row
    // the maximum over the 2 sep + 1 columns around each tile column.  The maximum over the square is then the maximum
    // of 2 sep + 1 row maxima: 2 (2 sep + 1) reads per pixel instead of (2 sep + 1)^2.
    __shared__ double st[kPeakStride * kPeakStride], rmax[kPeakStride * kTile];
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = kTilePix * (tid / kTile);
    const int Y0 = blockIdx.y * kTile, X0 = blockIdx.x * kTile;
    const int S = kTile + 2 * sep;
    const double ninf = -__builtin_inf();
    for (int e = tid; e < S * S; e += kTileThreads) {
        const int si = e / S, sj = e - si * S;
        const int Y = Y0 - sep + si, X = X0 - sep + sj;
        const bool in = (unsigned)Y < (unsigned)ny && (unsigned)X < (unsigned)nx;
        const double t = tmap[in ? (size_t)Y * nx + (size_t)X : 0];
        st[si * kPeakStride + sj] = in && fabs(t) < __builtin_inf() ? t : ninf;
    }
    __syncthreads();
    for (int e = tid; e < S * kTile; e += kTileThreads) {
        const int si = e / kTile, sj = e - si * kTile;
        double m = ninf;
        for (int dx = 0; dx <= 2 * sep; ++dx) m = fmax(m, st[si * kPeakStride + sj + dx]);
        rmax[e] = m;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTilePix; ++j) {
        const int Y = Y0 + ly + j, X = X0 + lx;
        const bool in = Y < ny && X < nx;
        const double t0 = tmap[in ? (size_t)Y * nx + (size_t)X : 0];
        double m = ninf;
        for (int dy = 0; dy <= 2 * sep; ++dy) m = fmax(m, rmax[(ly + j + dy) * kTile + lx]);
        // no finite T of the square lies above t0; what is left is the tie: an equal value at a lower pixel index
        bool peak = in && t0 >= threshold && t0 >= m;
        if (peak) {
            const int c = (ly + j + sep) * kPeakStride + lx + sep;
            for (int dy = -sep; dy <= 0; ++dy)
                for (int dx = -sep; dx <= (dy < 0 ? sep : -1); ++dx)
                    if (st[c + dy * kPeakStride + dx] == t0) peak = false;
        }
        const unsigned long long bal = __ballot(peak);
        if ((tid & 31) == 0 && Y < ny) mask[(size_t)Y * ntx + blockIdx.x] = (uint32_t)(bal >> (tid & 32));
    }
}

__device__ __forceinline__ int chunk_masks(int nseg, const uint32_t* __restrict__ mask, uint32_t (&m)[kThreadSegs]) {
    const int seg0 = (blockIdx.x * kChunkThreads + threadIdx.x) * kThreadSegs;
    int n = 0;
#pragma unroll
    for (int q = 0; q < kThreadSegs; ++q) {
        m[q] = seg0 + q < nseg ? mask[seg0 + q] : 0u;
        n += __popc(m[q]);
    }
    return n;
}

__global__ __launch_bounds__(kChunkThreads) void k_find_count(int nseg, const uint32_t* __restrict__ mask,
                                                              int* __restrict__ count) {
    __shared__ int part[kChunkThreads];
    uint32_t m[kThreadSegs];
    part[threadIdx.x] = chunk_masks(nseg, mask, m);
    block_scan<kChunkThreads>(part);
    if (threadIdx.x == kChunkThreads - 1) count[blockIdx.x] = part[threadIdx.x];
}

// the three-point parabola through (tm, t0, tp): the offset of its top, or 0 and `bit` where it has none
__device__ __forceinline__ double find_offset(double tm, double t0, double tp, int bit, int& flags) {
#pragma clang fp contract(off)
    const double curv = tm - 2.0 * t0 + tp;
    if (!(fabs(tm) < __builtin_inf()) || !(fabs(tp) < __builtin_inf()) || !(curv < 0.0)) {
        flags |= bit;
        return 0.0;
    }
    return fmin(fmax(0.5 * (tm - tp) / curv, -0.5), 0.5);
}

// The places of the peaks in pixel order: list[k] is the pixel index of peak k, for the first max_stars of them
__global__ __launch_bounds__(kChunkThreads) void k_find_list(int ny, int ntx, int nx, const uint32_t* __restrict__ mask,
                                                             const int* __restrict__ offset, int max_stars,
                                                             int* __restrict__ list, int32_t* __restrict__ count_out) {
    __shared__ int part[kChunkThreads];
    const int nseg = ny * ntx, tid = threadIdx.x;
    uint32_t m[kThreadSegs];
    const int mine = chunk_masks(nseg, mask, m);
    part[tid] = mine;
    block_scan<kChunkThreads>(part);
    if (blockIdx.x == 0 && tid == 0) count_out[0] = offset[gridDim.x];
    int k = offset[blockIdx.x] + part[tid] - mine;
    const int seg0 = (blockIdx.x * kChunkThreads + tid) * kThreadSegs;
#pragma unroll
    for (int q = 0; q < kThreadSegs; ++q) {
        const int Y = (seg0 + q) / ntx, X0 = ((seg0 + q) - Y * ntx) * kTile;
        for (uint32_t mm = m[q]; mm && k < max_stars; mm &= mm - 1, ++k) list[k] = Y * nx + X0 + __ffs((int)mm) - 1;
    }
}

// One wave per peak: its lanes fetch the window (the pixel rule on every tap) into LDS, then the sums run over it in
// tap order with the operations of k_find_map, the same in every lane; lane 0 writes the row.
__global__ __launch_bounds__(kRowThreads) void k_find_rows(int ny, int nx, const double* __restrict__ image,
                                                           const double* __restrict__ var,
                                                           const double* __restrict__ kk, int half,
                                                           const double* __restrict__ tmap,
                                                           const int* __restrict__ list, const int* __restrict__ total,
                                                           int max_stars, double* __restrict__ star_out,
                                                           int32_t* __restrict__ origin_out) {
#pragma clang fp contract(off)
    __shared__ double sw[kMaxTaps], swd[kMaxTaps], sd[kMaxTaps];
    const int W = 2 * half + 1, n = min(total[0], max_stars);
    const double nan = __builtin_nan("");
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int pix = list[k], Y = pix / nx, X = pix - Y * nx;
        for (int t = threadIdx.x; t < W * W; t += kRowThreads) {
            const int a = t / W, b = t - a * W;
            find_pixel(ny, nx, image, var, Y - half + a, X - half + b, sw[t], sd[t], swd[t]);
        }
        __syncthreads();
        FindSums s;
        double sumd = 0.0, sumk = 0.0;
        const int centre = half * W + half;
        for (int t = 0; t < W * W; ++t) {
            const double w = sw[t], k1 = kk[t];
            s.tap(w, swd[t], k1, kk[kMaxTaps + t]);
            if (w != 0.0 && t != centre) {
                sumd += sd[t];
                sumk += k1;
            }
        }
        double T, H, b;
        find_stat(s, true, W * W, var != nullptr, T, H, b);
        const double t0 = tmap[pix];
        int flags = 0;
        const double dy = find_offset(Y > 0 ? tmap[pix - nx] : nan, t0, Y + 1 < ny ? tmap[pix + nx] : nan, 1, flags);
        const double dx = find_offset(X > 0 ? tmap[pix - 1] : nan, t0, X + 1 < nx ? tmap[pix + 1] : nan, 2, flags);
        const int other = s.nvalid - 1;
        const double md = sumd / (double)other, mk = sumk / (double)other;
        const double sden = H * (kk[centre] - mk);
        double sharp = (sd[centre] - md) / sden;
        if (other < 1 || sden == 0.0) {
            sharp = nan;
            flags |= 4;
        }
        if (threadIdx.x == 0) {
            double* row = star_out + (size_t)k * 8;
            row[0] = (double)Y + dy;
            row[1] = (double)X + dx;
            row[2] = t0;
            row[3] = H;
            row[4] = b;
            row[5] = sharp;
            row[6] = (double)s.nvalid;
            row[7] = (double)flags;
            if (origin_out) {
                origin_out[(size_t)k * 2] = Y - NS / 2;
                origin_out[(size_t)k * 2 + 1] = X - NS / 2;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_find_fill(const int* __restrict__ total, int max_stars,
                                                   double* __restrict__ star_out, int32_t* __restrict__ origin_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= max_stars || k < total[0]) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) star_out[(size_t)k * 8 + c] = __builtin_nan("");
    if (origin_out) {
        origin_out[(size_t)k * 2] = kFillerOrigin;
        origin_out[(size_t)k * 2 + 1] = kFillerOrigin;
    }
}

// The workspace: kk [2][kMaxTaps], T [ny][nx] unless the caller takes the map, mask [ny][ntx], then from the next
// multiple of 8 bytes count [nchunk], offset [nchunk + 1], list [max_stars]
struct FindWork {
    int ntx, nty, nseg, nchunk;
    double *kk, *tmap;
    uint32_t* mask;
    int *count, *offset, *list;
    FindWork(WorkspaceCarver& ws, int ny, int nx, int max_stars, bool with_map)
        : ntx((nx + kTile - 1) / kTile), nty((ny + kTile - 1) / kTile), nseg(ny * ntx),
          nchunk((nseg + kChunkSegs - 1) / kChunkSegs), kk(ws.take<double>(2 * kMaxTaps)),
          tmap(with_map ? nullptr : ws.take<double>((size_t)ny * nx)), mask(ws.take<uint32_t>(nseg)),
          count(ws.take<int>(nchunk, 8)), offset(ws.take<int>((size_t)nchunk + 1)), list(ws.take<int>(max_stars)) {}
};

}  // namespace

size_t find_workspace_bytes(int ny, int nx, int max_stars, bool with_map) {
    return workspace_bytes<FindWork>(ny, nx, max_stars, with_map);
}

void launch_find_stars(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, const double* d_psf,
                       int half, int sep, double threshold, int max_stars, double* d_star_out, int32_t* d_origin_out,
                       int32_t* d_count_out, double* d_map_out, void* d_ws) {
    static_assert(kMaxHalf <= NS / 2, "the core lies inside the model stamp");
    WorkspaceCarver ws(d_ws);
    const FindWork w(ws, ny, nx, max_stars, d_map_out != nullptr);
    double* tmap = d_map_out ? d_map_out : w.tmap;
    const int* total = w.offset + w.nchunk;
    // (every word of the workspace that is read is written before by this call: nothing to clear; of `list` the rows
    // kernel reads the places below the count only, which k_find_list has written)
    hipLaunchKernelGGL(k_find_core, dim3(1), dim3(kTileThreads), 0, s, d_psf, half, w.kk);
    hipLaunchKernelGGL(k_find_map, dim3(w.ntx, w.nty), dim3(kTileThreads), 0, s, ny, nx, d_image, d_var, w.kk, half,
                       tmap);
    hipLaunchKernelGGL(k_find_peaks, dim3(w.ntx, w.nty), dim3(kTileThreads), 0, s, ny, nx, w.ntx, tmap, sep, threshold,
                       w.mask);
    hipLaunchKernelGGL(k_find_count, dim3(w.nchunk), dim3(kChunkThreads), 0, s, w.nseg, w.mask, w.count);
    launch_scan_counts(s, w.nchunk, w.count, w.offset);
    hipLaunchKernelGGL(k_find_list, dim3(w.nchunk), dim3(kChunkThreads), 0, s, ny, w.ntx, nx, w.mask, w.offset, max_stars,
                       w.list, d_count_out);
    hipLaunchKernelGGL(k_find_rows, dim3(max_stars < kRowBlocks ? max_stars : kRowBlocks), dim3(kRowThreads), 0, s, ny, nx,
                       d_image, d_var, w.kk, half, tmap, w.list, total, max_stars, d_star_out, d_origin_out);
    hipLaunchKernelGGL(k_find_fill, dim3((max_stars + 255) / 256), dim3(256), 0, s, total, max_stars, d_star_out,
                       d_origin_out);
}

}  // namespace mpsfr
