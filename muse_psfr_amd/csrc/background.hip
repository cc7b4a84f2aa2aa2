// The background map: clipped mesh medians of frames and cubes.
//   k_bg_cell   one workgroup per (mesh cell, layer): the valid pixels of the cell go into LDS once, as
//               order-preserving 64-bit keys, and are sorted there (bitonic).  In ascending order the deviations
//               |x - m| fall towards the median and rise behind it, so everything after the sort is a search: the
//               survivors of a clipping pass are a contiguous range, the median is read at its middle, the median
//               absolute deviation is the rank selection over two sorted lists.  Writes columns 2 .. 7 of the cell's
//               row of mesh_out.
//   k_bg_head   one workgroup per layer: the valid and filled cells by integer sums; writes the layer's row of head_out
//   k_bg_mesh   one thread per (cell, layer): the median of the raw levels and of the raw rms over the valid cells of
//               the filter window, in registers; a cell whose window is empty looks at growing rings.  Writes columns 0
//               and 1.
//   k_bg_map    one workgroup per 256 pixels of a frame row: 4 x 4 Keys taps of the level and the rms plane, linearly
//               continued beyond the mesh; writes up to three planes.
// Every column of mesh_out is an order statistic, an integer or a single rounding: the result does not depend on the
// order in which the keys reach LDS, which is the only thing here that is not fixed.  fp64 in both precision modes; no
// floating-point atomics.  The call has no work memory: k_bg_head, k_bg_mesh and k_bg_map read what the kernels before
// them wrote into mesh_out and head_out.
#include "frame_common.h"

namespace mpsfr {
namespace {

constexpr int kCellThreads = 256;
constexpr int kMinBox = 8, kMaxBox = 64;                      // MPSFR_BACKGROUND_MIN_BOX, MPSFR_BACKGROUND_MAX_BOX
constexpr int kMaxCell = kMaxBox * kMaxBox;                   // keys of one cell: 32 KiB of LDS
constexpr int kCellRun = kMaxCell / kCellThreads;             // pixels one thread takes in at most
constexpr int kNBack = 8, kNHead = 4;                         // MPSFR_NBACK, MPSFR_NBACK_HEAD
constexpr int kFilled = 1, kClipCap = 2, kFlat = 4;           // MPSFR_BACK_FILLED, _CLIP_CAP, _FLAT
constexpr double kMadToSigma = 1.4826;
constexpr int kMaxLayersPerLaunch = 65535;                    // the layer is grid dimension z
constexpr unsigned long long kSign = 0x8000000000000000ull;
static_assert(kCellRun * kCellThreads == kMaxCell, "a thread's run covers the largest cell");

// a finite double as a key whose unsigned order is the order of the values, and back
__device__ __forceinline__ unsigned long long key_of(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
    return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

// the smallest power of two (2 at least) that holds n keys
inline __host__ __device__ int sort_size(int n) {
    int P = 2;
    while (P < n) P <<= 1;
    return P;
}

// The first place of [a, b) at which `pred` holds (b if it holds nowhere); it holds from there on.  The 64 lanes of a
// wave probe 64 places a step; a, b and the answer are the same in every lane.
template <typename Pred>
__device__ __forceinline__ int first_place(int a, int b, Pred pred) {
    const int lane = threadIdx.x & 63;
    if (a >= b) return b;
    while (b - a > 64) {
        // probe f sits at a + (f + 1) step - 1, the last ones on b - 1
        const int step = (b - a + 63) >> 6;
        const unsigned long long bal = __ballot(pred(min(a + (lane + 1) * step, b) - 1));
        if (!bal) return b;
        const int f = __ffsll((long long)bal) - 1;
        b = min(a + (f + 1) * step, b) - 1;                          // it holds here, and not at probe f - 1
        a += f * step;
    }
    const unsigned long long bal = __ballot(a + lane < b && pred(min(a + lane, b - 1)));
    return bal ? a + __ffsll((long long)bal) - 1 : b;
}

// The cell in ascending order, the range [lo, hi) of it in use, its median m and the first place at or above m
struct SortedCell {
    const unsigned long long* keys;
    int lo, hi, split;
    double m;
    __device__ __forceinline__ double dev(int j) const {              // |x_j - m|, one rounded subtraction
#pragma clang fp contract(off)
        const double x = value_of(keys[j]);
        return j < split ? m - x : x - m;
    }
    // The deviation of rank k (0-based) of the range: the k + 1 smallest are the first i of the ascending list behind
    // the split and the first k + 1 - i of the list before it, read backwards, for the smallest i at which the last one
    // taken before the split does not exceed the next one behind it.
    __device__ __forceinline__ double dev_of_rank(int k) const {
        const int na = hi - split, nb = split - lo;
        const int i = first_place(max(0, k + 1 - nb), min(k + 1, na), [&](int i) {
            return k + 1 - i == 0 || i == na || dev(split - 1 - (k - i)) <= dev(split + i);
        });
        const int j = k + 1 - i;
        const double a = i > 0 ? dev(split + i - 1) : -1.0, b = j > 0 ? dev(split - j) : -1.0;
        return a > b ? a : b;
    }
};

__global__ __launch_bounds__(kCellThreads) void k_bg_cell(int layer0, int ny, int nx, int box, int my, int mx,
                                                          const double* __restrict__ image,
                                                          const double* __restrict__ var, double kc, int max_clip,
                                                          double min_frac, double* __restrict__ mesh) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long keys[];                     // sort_size(box box) of them
    __shared__ int count;
    const int tid = threadIdx.x, lane = tid & 63;
    const int cx = blockIdx.x, cy = blockIdx.y, layer = layer0 + blockIdx.z;
    const int Y0 = cy * box, X0 = cx * box;
    const int h = min(box, ny - Y0), w = min(box, nx - X0), npix = h * w;
    const size_t plane = (size_t)layer * ny * nx;
    if (tid == 0) count = 0;
    __syncthreads();
    // intake: the pixel rule of the observed fits; a valid zero counts as +0.  The valid ones go into LDS in any order.
#pragma unroll
    for (int j = 0; j < kCellRun; ++j) {
        if (j * kCellThreads >= npix) break;                         // (uniform)
        const int e = tid + j * kCellThreads;
        const int r = e / w, c = e - r * w;
        const bool in = e < npix;
        const size_t i = in ? plane + (size_t)(Y0 + r) * nx + (size_t)(X0 + c) : plane;
        const double dv = image[i];
        const double vv = var ? var[i] : 1.0;
        const bool ok = in && fabs(dv) < __builtin_inf() && vv > 0.0 && vv < __builtin_inf();
        const unsigned long long bal = __ballot(ok);
        if (bal) {                                                   // (wave-uniform)
            int base = 0;
            if (lane == 0) base = atomicAdd(&count, __popcll(bal));
            base = __shfl(base, 0);
            if (ok) keys[base + __popcll(bal & ((1ull << lane) - 1ull))] = key_of(dv + 0.0);
        }
    }
    __syncthreads();
    const int n_valid = count;
    const bool valid = n_valid >= 1 && (double)n_valid >= min_frac * (double)npix;
    double m = __builtin_nan(""), mad = __builtin_nan("");
    int n = n_valid, passes = 0, flags = valid ? 0 : kFilled;
    if (valid) {                                                 // (uniform over the workgroup, as every exit below)
        // the keys, padded with the largest key to a power of two, into ascending order
        const int P = sort_size(n_valid);
        for (int i = n_valid + tid; i < P; i += kCellThreads) keys[i] = ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += kCellThreads) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
                __syncthreads();
            }
        // nothing is written from here on: every thread walks the same passes on its own
        SortedCell cell{keys, 0, n_valid, 0, 0.0};
        for (;;) {
            n = cell.hi - cell.lo;
            const int k1 = (n - 1) >> 1, k2 = n >> 1;
            const double x1 = value_of(keys[cell.lo + k1]), x2 = value_of(keys[cell.lo + k2]);
            m = (n & 1) ? x1 : 0.5 * x1 + 0.5 * x2;
            cell.m = m;
            const unsigned long long mkey = key_of(m + 0.0);
            cell.split = first_place(cell.lo, cell.hi, [&](int j) { return keys[j] >= mkey; });
            const double d1 = cell.dev_of_rank(k1);
            mad = (n & 1) ? d1 : 0.5 * d1 + 0.5 * cell.dev_of_rank(k2);
            if (passes == max_clip) flags |= kClipCap;
            if (mad == 0.0) flags |= kFlat;
            if (flags) break;
            // the survivors d <= t: d falls up to the split and rises from it
            const double t = kc * mad;
            const int lo = first_place(cell.lo, cell.split, [&](int j) { return cell.dev(j) <= t; });
            const int hi = first_place(cell.split, cell.hi, [&](int j) { return !(cell.dev(j) <= t); });
            if (hi - lo == n) break;
            cell.lo = lo;
            cell.hi = hi;
            ++passes;
        }
    }
    if (tid == 0) {
        double* row = mesh + ((size_t)layer * my * mx + (size_t)cy * mx + cx) * kNBack;
        row[2] = m;
        row[3] = valid ? kMadToSigma * mad : mad;
        row[4] = valid ? (double)n : 0.0;
        row[5] = (double)n_valid;
        row[6] = (double)passes;
        row[7] = (double)flags;
    }
}

__global__ __launch_bounds__(kCellThreads) void k_bg_head(int layer0, int ncell, const double* __restrict__ mesh,
                                                          double* __restrict__ head) {
    __shared__ int part[kCellThreads];
    const int layer = layer0 + blockIdx.x;
    const double* rows = mesh + (size_t)layer * ncell * kNBack;
    int nvalid = 0;
    for (int i = threadIdx.x; i < ncell; i += kCellThreads)
        nvalid += ((int)rows[(size_t)i * kNBack + 7] & kFilled) ? 0 : 1;
    part[threadIdx.x] = nvalid;
    block_scan<kCellThreads>(part);
    if (threadIdx.x == kCellThreads - 1) {
        nvalid = part[threadIdx.x];
        double* row = head + (size_t)layer * kNHead;
        row[0] = nvalid == ncell ? 0.0 : nvalid > 0 ? 1.0 : 2.0;
        row[1] = (double)nvalid;
        row[2] = (double)(ncell - nvalid);
        row[3] = 0.0;
    }
}

// med of the values of v whose bit of `mask` is set (cnt of them, at least one), by counting: no value moves
template <int N>
__device__ __forceinline__ double median_masked(const double (&v)[N], unsigned mask, int cnt) {
#pragma clang fp contract(off)
    const int k1 = (cnt - 1) / 2, k2 = cnt / 2;
    double r1 = 0.0, r2 = 0.0;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        int less = 0, leq = 0;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const bool on = (mask >> b) & 1u;
            less += on && v[b] < v[a] ? 1 : 0;
            leq += on && v[b] <= v[a] ? 1 : 0;
        }
        const bool on = (mask >> a) & 1u;
        if (on && less <= k1 && k1 < leq) r1 = v[a];
        if (on && less <= k2 && k2 < leq) r2 = v[a];
    }
    return (cnt & 1) ? r1 : 0.5 * r1 + 0.5 * r2;
}

// med of column `col` over the valid cells on the ring at distance r of cell (ci, cj) (cnt of them, at least one)
__device__ double median_ring(const double* __restrict__ rows, int my, int mx, int ci, int cj, int r, int col,
                              int cnt) {
#pragma clang fp contract(off)
    const int k1 = (cnt - 1) / 2, k2 = cnt / 2;
    const int i0 = max(ci - r, 0), i1 = min(ci + r, my - 1), j0 = max(cj - r, 0), j1 = min(cj + r, mx - 1);
    double r1 = 0.0, r2 = 0.0;
    for (int ia = i0; ia <= i1; ++ia)
        for (int ja = j0; ja <= j1; ++ja) {
            if (max(abs(ia - ci), abs(ja - cj)) != r) continue;
            const double* a = rows + ((size_t)ia * mx + ja) * kNBack;
            if ((int)a[7] & kFilled) continue;
            const double va = a[col];
            int less = 0, leq = 0;
            for (int ib = i0; ib <= i1; ++ib)
                for (int jb = j0; jb <= j1; ++jb) {
                    if (max(abs(ib - ci), abs(jb - cj)) != r) continue;
                    const double* b = rows + ((size_t)ib * mx + jb) * kNBack;
                    if ((int)b[7] & kFilled) continue;
                    less += b[col] < va ? 1 : 0;
                    leq += b[col] <= va ? 1 : 0;
                }
            if (less <= k1 && k1 < leq) r1 = va;
            if (less <= k2 && k2 < leq) r2 = va;
        }
    return (cnt & 1) ? r1 : 0.5 * r1 + 0.5 * r2;
}

template <int FILTER>
__global__ __launch_bounds__(256) void k_bg_mesh(int layer0, int my, int mx, const double* __restrict__ head,
                                                 double* __restrict__ mesh) {
    constexpr int H = (FILTER - 1) / 2, N = FILTER * FILTER;
    const int cell = blockIdx.x * 256 + threadIdx.x, layer = layer0 + blockIdx.y;
    if (cell >= my * mx) return;
    const int ci = cell / mx, cj = cell - ci * mx;
    double* rows = mesh + (size_t)layer * my * mx * kNBack;
    double lv[N], rm[N];
    unsigned mask = 0;
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < FILTER; ++a)
#pragma unroll
        for (int b = 0; b < FILTER; ++b) {
            const int i = ci + a - H, j = cj + b - H;
            const bool in = (unsigned)i < (unsigned)my && (unsigned)j < (unsigned)mx;
            const double* row = rows + (in ? (size_t)i * mx + j : (size_t)cell) * kNBack;
            const bool ok = in && !((int)row[7] & kFilled);
            lv[a * FILTER + b] = row[2];
            rm[a * FILTER + b] = row[3];
            mask |= ok ? 1u << (a * FILTER + b) : 0u;
            cnt += ok ? 1 : 0;
        }
    double level = __builtin_nan(""), rms = __builtin_nan("");
    if (cnt > 0) {
        level = median_masked(lv, mask, cnt);
        rms = median_masked(rm, mask, cnt);
    } else if (head[(size_t)layer * kNHead + 1] > 0.0) {
        // an empty window in a layer that has valid cells: the first ring that holds one (the square inside is empty)
        const int rmax = max(my, mx);
        for (int r = H + 1; r <= rmax && cnt == 0; ++r) {
            const int i0 = max(ci - r, 0), i1 = min(ci + r, my - 1), j0 = max(cj - r, 0), j1 = min(cj + r, mx - 1);
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j)
                    if (max(abs(i - ci), abs(j - cj)) == r && !((int)rows[((size_t)i * mx + j) * kNBack + 7] & kFilled))
                        ++cnt;
            if (cnt > 0) {
                level = median_ring(rows, my, mx, ci, cj, r, 2, cnt);
                rms = median_ring(rows, my, mx, ci, cj, r, 3, cnt);
            }
        }
    }
    rows[(size_t)cell * kNBack] = level;
    rows[(size_t)cell * kNBack + 1] = rms;
}

// The plane of column `col` of a layer's mesh, continued linearly by two nodes each way: columns first, then rows
struct MeshPlane {
    const double* rows;                                              // the layer's rows, at column `col`
    int my, mx;
    __device__ __forceinline__ double node(int i, int j) const { return rows[((size_t)i * mx + j) * kNBack]; }
    __device__ __forceinline__ double along_row(int i, int j) const {
#pragma clang fp contract(off)
        if (mx == 1) return node(i, 0);
        if (j < 0) return node(i, 0) + (double)(-j) * (node(i, 0) - node(i, 1));
        if (j >= mx) return node(i, mx - 1) + (double)(j - mx + 1) * (node(i, mx - 1) - node(i, mx - 2));
        return node(i, j);
    }
    __device__ __forceinline__ double at(int i, int j) const {
#pragma clang fp contract(off)
        if (my == 1) return along_row(0, j);
        if (i < 0) return along_row(0, j) + (double)(-i) * (along_row(0, j) - along_row(1, j));
        if (i >= my) return along_row(my - 1, j) + (double)(i - my + 1) * (along_row(my - 1, j) - along_row(my - 2, j));
        return along_row(i, j);
    }
};

constexpr int kMapThreads = 256;
constexpr int kMapCols = kMapThreads / kMinBox + 4;              // mesh columns under a block's pixels, and the taps

// One workgroup per 256 pixels of a frame row: the 4 mesh rows of the row's taps, continued, over the mesh columns the
// block's taps reach go into LDS once per plane; a pixel then sums its 4 x 4 taps, rows outer, columns inner, both
// ascending.
__global__ __launch_bounds__(kMapThreads) void k_bg_map(int layer0, int ny, int nx, int box, int my, int mx,
                                                        const double* __restrict__ mesh, const double* apply_to,
                                                        double* __restrict__ map_out, double* __restrict__ rms_out,
                                                        double* applied_out) {
#pragma clang fp contract(off)
    __shared__ double sE[2][4][kMapCols];
    const int tid = threadIdx.x, X0 = blockIdx.x * kMapThreads, X = X0 + tid, Y = blockIdx.y;
    const int layer = layer0 + blockIdx.z;
    // node i of an axis sits at pixel (i + 0.5) box - 0.5: the mesh coordinate of a pixel, its floor and the fraction
    const double uy = ((double)Y + 0.5) / (double)box - 0.5;
    const double ux = ((double)min(X, nx - 1) + 0.5) / (double)box - 0.5;
    const KeysTaps<double> ty(-uy), tx(-ux);
    const int jbase = (int)__builtin_floor(((double)X0 + 0.5) / (double)box - 0.5) - 1;
    const int jlast = (int)__builtin_floor(((double)min(X0 + kMapThreads - 1, nx - 1) + 0.5) / (double)box - 0.5) + 2;
    const int ncols = min(jlast - jbase + 1, kMapCols);              // (at most 256 / box + 4 by construction)
    const double* rows = mesh + (size_t)layer * my * mx * kNBack;
    const bool level = map_out || applied_out;
    for (int e = tid; e < 2 * 4 * ncols; e += kMapThreads) {
        const int p = e / (4 * ncols), a = (e - p * 4 * ncols) / ncols, c = e - (p * 4 + a) * ncols;
        if (p == 0 ? level : rms_out != nullptr) sE[p][a][c] = MeshPlane{rows + p, my, mx}.at(ty.f - 1 + a, jbase + c);
    }
    __syncthreads();
    if (X >= nx) return;
    const size_t i = ((size_t)layer * ny + Y) * nx + X;
    const int c0 = tx.f - 1 - jbase;
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double inner = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) inner = inner + tx.w[b] * sE[p][a][c0 + b];
            sum[p] = sum[p] + ty.w[a] * inner;
        }
    if (map_out) map_out[i] = sum[0];
    if (applied_out) applied_out[i] = apply_to[i] - sum[0];
    if (rms_out) rms_out[i] = sum[1] < 0.0 ? 0.0 : sum[1];
}

}  // namespace

void launch_frame_background(hipStream_t s, int nl, int ny, int nx, const double* d_image, const double* d_var, int box,
                             int filter, double kc, int max_clip, double min_frac, const double* d_apply_to,
                             double* d_mesh_out, double* d_head_out, double* d_map_out, double* d_rms_out,
                             double* d_applied_out) {
    static_assert(kMaxCell * sizeof(unsigned long long) == 32768, "the keys of the largest cell: four workgroups a CU");
    const int my = (ny + box - 1) / box, mx = (nx + box - 1) / box, ncell = my * mx;
    const bool maps = d_map_out || d_rms_out || d_applied_out;
    const size_t lds = sort_size(box * box) * sizeof(unsigned long long);
    for (int l0 = 0; l0 < nl; l0 += kMaxLayersPerLaunch) {
        const int layers = nl - l0 < kMaxLayersPerLaunch ? nl - l0 : kMaxLayersPerLaunch;
        hipLaunchKernelGGL(k_bg_cell, dim3(mx, my, layers), dim3(kCellThreads), lds, s, l0, ny, nx, box, my, mx,
                           d_image, d_var, kc, max_clip, min_frac, d_mesh_out);
        hipLaunchKernelGGL(k_bg_head, dim3(layers), dim3(kCellThreads), 0, s, l0, ncell, d_mesh_out, d_head_out);
        const dim3 grid((ncell + 255) / 256, layers);
        if (filter == 1)
            hipLaunchKernelGGL(k_bg_mesh<1>, grid, dim3(256), 0, s, l0, my, mx, d_head_out, d_mesh_out);
        else if (filter == 3)
            hipLaunchKernelGGL(k_bg_mesh<3>, grid, dim3(256), 0, s, l0, my, mx, d_head_out, d_mesh_out);
        else
            hipLaunchKernelGGL(k_bg_mesh<5>, grid, dim3(256), 0, s, l0, my, mx, d_head_out, d_mesh_out);
        if (maps)
            hipLaunchKernelGGL(k_bg_map, dim3((nx + kMapThreads - 1) / kMapThreads, ny, layers), dim3(kMapThreads),
                               0, s, l0, ny, nx, box, my, mx, d_mesh_out, d_apply_to, d_map_out, d_rms_out,
                               d_applied_out);
    }
}

}  // namespace mpsfr
