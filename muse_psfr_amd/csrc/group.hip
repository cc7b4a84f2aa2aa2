// Friends-of-friends grouping of found stars: the connected components of "closer than crit", as
// the tables mpsfr_cut_stamps, mpsfr_fit_stamps_psf and mpsfr_fit_groups_psf take.
//   k_group_init     one thread per star: its kind (star, filler, out of range), a compact copy of its position, the
//                    union-find parent, the member slots and the size, and the count of its cell
//   k_scan_counts    exclusive scan of the cell counts (render.hip, one workgroup)
//   k_group_scatter  the stars of every cell at an atomic cursor (arbitrary order inside a cell)
//   k_group_link     one thread per star: the stars j < i of its 3 x 3 cells that the link rule joins to it are united
//                    with it in a lock-free union-find that hooks the larger root under the smaller
//   k_group_gather   one thread per star: its root (the label), the size of the root's group by an integer add and the
//                    group's four smallest members by a cascade of integer minima
//   k_group_count    the roots of every class in every chunk of kChunk stars
//   k_scan_counts    again, over the (class, chunk) counts: class first, star index second -- the row order
//   k_group_rows     one thread per star: a root's row from its class, chunk and rank; the group and origin rows
//   k_group_tail     one thread per output row: filler rows, the shifts at the per-class pitch, the six counts
// The order of the stars inside a cell and the interleaving of the atomics decide nothing: a root is the smallest index
// of its component however the hooks arrive, sizes are integer sums and the member slots hold the smallest indices
// whatever the order of the minima.  Integer atomics only; every workspace word that is read is written before by the
// same call.
#include "frame_common.h"

namespace mpsfr {
namespace {

// Side of a cell in pixels.  Two linked stars have |fl(y_i - y_j)| <= 16, so their true distance along an axis is below
// 17 and floor(y_i), floor(y_j) differ by at most 17: they lie in the same or in adjacent cells.  (With 16-pixel cells
// the rounded difference of 32 and the double below 16 is 16.0, a link at crit = 16 across a whole cell.)
constexpr int kCell = 17;
constexpr int kThreads = 256, kChunk = kThreads;              // stars of one workgroup; one star per thread
constexpr int kClasses = 5;                                   // 1, 2, 3, 4 members, oversize
constexpr int kMaxGroup = 4;                                  // MPSFR_MAX_GROUP
constexpr int kEmpty = 0x7fffffff;                            // a member slot nobody has claimed
constexpr int kWide = 2;                                      // MPSFR_GROUP_WIDE
constexpr int kOversize = 1;                                  // MPSFR_GROUP_OVERSIZE
constexpr double kMaxShift = 8.0;                             // MPSFR_FIT_PSF_MAX_SHIFT

__host__ __device__ __forceinline__ int cells(int n) { return (n + kCell) / kCell + 1; }

// the cell of a position inside [-1, ny] x [-1, nx]
__device__ __forceinline__ int cell_of(double v) { return ((int)floor(v) + kCell) / kCell; }

// 0 a star, -1 a filler (NaN in either coordinate), -2 out of range (beyond [-1, ny] x [-1, nx], infinities included)
__device__ __forceinline__ int star_kind(int ny, int nx, double y, double x) {
    if (y != y || x != x) return -1;
    return y >= -1.0 && y <= (double)ny && x >= -1.0 && x <= (double)nx ? 0 : -2;
}

__global__ __launch_bounds__(kThreads) void k_group_init(int ny, int nx, int nstar, const double* __restrict__ pos,
                                                         int stride, double2* __restrict__ yx,
                                                         int* __restrict__ kind, int* __restrict__ parent,
                                                         int* __restrict__ size, int* __restrict__ slots,
                                                         int* __restrict__ cellcount) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nstar) return;
    const double y = pos[(size_t)i * stride], x = pos[(size_t)i * stride + 1];
    const int k = star_kind(ny, nx, y, x);
    yx[i] = make_double2(y, x);
    kind[i] = k;
    parent[i] = i;
    size[i] = 0;
#pragma unroll
    for (int s = 0; s < kMaxGroup - 1; ++s) slots[(size_t)i * (kMaxGroup - 1) + s] = kEmpty;
    if (k == 0) atomicAdd(&cellcount[cell_of(y) * cells(nx) + cell_of(x)], 1);
}

__global__ __launch_bounds__(kThreads) void k_group_scatter(int nx, int nstar, const double2* __restrict__ yx,
                                                            const int* __restrict__ kind,
                                                            const int* __restrict__ celloff, int* __restrict__ cursor,
                                                            int* __restrict__ cellstars) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nstar || kind[i] != 0) return;
    const int c = cell_of(yx[i].x) * cells(nx) + cell_of(yx[i].y);
    cellstars[celloff[c] + atomicAdd(&cursor[c], 1)] = i;
}

__device__ __forceinline__ int parent_of(const int* parent, int a) {
    return __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[a] <= a always, so the walk ends at a root; a root that another thread hooks meanwhile is found out by the
// compare-and-swap below
__device__ __forceinline__ int root_of(const int* parent, int a) {
    for (int p = parent_of(parent, a); p != a; p = parent_of(parent, a)) a = p;
    return a;
}

// The same walk while the links are made, halving the path behind it: a node that is not a root never becomes one
// again and its ancestors stay its ancestors, so pointing it at its grandparent is safe whatever the other threads do.
__device__ __forceinline__ int root_of_halving(int* parent, int a) {
    int p = parent_of(parent, a);
    while (p != a) {
        const int gp = parent_of(parent, p);
        if (gp != p) __hip_atomic_store(parent + a, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = p;
        p = gp;
    }
    return a;
}

// Joins the components of a and b: the larger root goes under the smaller.  A failed compare-and-swap means that
// another thread has hooked that root since it was read: the walk goes on from there, nobody waits for anybody.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = root_of_halving(parent, a);
        b = root_of_halving(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
        a = hi;
        b = lo;
    }
}

// the link rule: each product rounded, then the sum, against the rounded crit^2
__device__ __forceinline__ bool linked(double2 a, double2 b, double c2) {
#pragma clang fp contract(off)
    const double dy = a.x - b.x, dx = a.y - b.y;
    const double d2 = dy * dy + dx * dx;
    return d2 <= c2;
}

__global__ __launch_bounds__(kThreads) void k_group_link(int ny, int nx, int nstar, const double2* __restrict__ yx,
                                                         const int* __restrict__ kind, double c2,
                                                         const int* __restrict__ celloff,
                                                         const int* __restrict__ cellstars, int* __restrict__ parent) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nstar || kind[i] != 0) return;
    const double2 me = yx[i];
    const int cy = cell_of(me.x), cx = cell_of(me.y), ncy = cells(ny), ncx = cells(nx);
    for (int ay = max(cy - 1, 0); ay <= min(cy + 1, ncy - 1); ++ay)
        for (int ax = max(cx - 1, 0); ax <= min(cx + 1, ncx - 1); ++ax) {
            const int c = ay * ncx + ax;
            for (int p = celloff[c], e = celloff[c + 1]; p < e; ++p) {
                const int j = cellstars[p];
                if (j < i && linked(me, yx[j], c2)) unite(parent, i, j);
            }
        }
}

__global__ __launch_bounds__(kThreads) void k_group_gather(int nstar, const int* __restrict__ kind,
                                                           const int* __restrict__ parent, int* __restrict__ size,
                                                           int* __restrict__ slots, int32_t* __restrict__ label_out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nstar) return;
    if (kind[i] != 0) {
        label_out[i] = kind[i];
        return;
    }
    const int r = root_of(parent, i);
    label_out[i] = r;
    atomicAdd(&size[r], 1);
    // The root is the smallest member.  The others go down the slots: a slot keeps the smaller of its value and the
    // arrival, the larger moves on -- every slot ends with the smallest value that ever reached it.
    int v = i;
    for (int s = 0; s < kMaxGroup - 1 && v != r && v != kEmpty; ++s) {
        const int old = atomicMin(&slots[(size_t)r * (kMaxGroup - 1) + s], v);
        v = max(old, v);
    }
}

// class of a root: 0 .. 3 for 1 .. 4 members, 4 oversize; -1: not a root
__device__ __forceinline__ int root_class(int i, int nstar, const int32_t* __restrict__ label,
                                          const int* __restrict__ size) {
    if (i >= nstar || label[i] != i) return -1;
    return min(size[i], kMaxGroup + 1) - 1;
}

// Roots of class c in the chunk before this thread (exclusive rank) and in the whole chunk; wavecount: LDS
// [kThreads / 64][kClasses]
__device__ __forceinline__ void chunk_ranks(int cls, int (*wavecount)[kClasses], int& rank, int (&total)[kClasses]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int below = 0;
#pragma unroll
    for (int c = 0; c < kClasses; ++c) {
        const unsigned long long bal = __ballot(cls == c);
        if (cls == c) below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wavecount[wave][c] = __popcll(bal);
    }
    __syncthreads();
    rank = below;
#pragma unroll
    for (int c = 0; c < kClasses; ++c) {
        total[c] = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave && c == cls) rank += wavecount[w][c];
            total[c] += wavecount[w][c];
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_group_count(int nstar, const int32_t* __restrict__ label,
                                                          const int* __restrict__ size, int* __restrict__ count) {
    __shared__ int wavecount[kThreads / 64][kClasses];
    const int cls = root_class(blockIdx.x * kChunk + threadIdx.x, nstar, label, size);
    int rank, total[kClasses];
    chunk_ranks(cls, wavecount, rank, total);
    if (threadIdx.x < kClasses) count[threadIdx.x * gridDim.x + blockIdx.x] = total[threadIdx.x];
}

// The members of the group of root r in ascending order (-1 beyond the group; the four smallest of an oversize group),
// and for a group of up to four its origin, shifts and flags.
struct GroupRow {
    int n, flags, member[kMaxGroup], origin[2];
    double shift[kMaxGroup][2];
};

__device__ __forceinline__ void group_row(int r, const int* __restrict__ size, const int* __restrict__ slots,
                                          const double2* __restrict__ yx, GroupRow& g) {
#pragma clang fp contract(off)
    g.n = size[r];
    g.member[0] = r;
#pragma unroll
    for (int s = 1; s < kMaxGroup; ++s) {
        const int m = slots[(size_t)r * (kMaxGroup - 1) + s - 1];
        g.member[s] = m == kEmpty ? -1 : m;
    }
    g.flags = g.n > kMaxGroup ? kOversize : 0;
    g.origin[0] = g.origin[1] = kFillerOrigin;
#pragma unroll
    for (int s = 0; s < kMaxGroup; ++s) g.shift[s][0] = g.shift[s][1] = 0.0;
    if (g.n > kMaxGroup) return;
    double lo0 = yx[r].x, hi0 = lo0, lo1 = yx[r].y, hi1 = lo1;
    // (fixed trip counts and guards, so that the row stays in registers)
#pragma unroll
    for (int s = 1; s < kMaxGroup; ++s) {
        if (s >= g.n) continue;
        const double2 p = yx[g.member[s]];
        lo0 = fmin(lo0, p.x), hi0 = fmax(hi0, p.x);
        lo1 = fmin(lo1, p.y), hi1 = fmax(hi1, p.y);
    }
    g.origin[0] = (int)floor(0.5 * (lo0 + hi0) + 0.5) - NS / 2;
    g.origin[1] = (int)floor(0.5 * (lo1 + hi1) + 0.5) - NS / 2;
#pragma unroll
    for (int s = 0; s < kMaxGroup; ++s) {
        if (s >= g.n) continue;
        const double2 p = yx[g.member[s]];
        g.shift[s][0] = p.x - (double)(g.origin[0] + NS / 2);
        g.shift[s][1] = p.y - (double)(g.origin[1] + NS / 2);
        if (fabs(g.shift[s][0]) > kMaxShift || fabs(g.shift[s][1]) > kMaxShift) g.flags |= kWide;
    }
}

__global__ __launch_bounds__(kThreads) void k_group_rows(int nstar, const int32_t* __restrict__ label,
                                                         const int* __restrict__ size, const int* __restrict__ slots,
                                                         const double2* __restrict__ yx,
                                                         const int* __restrict__ offset, int max_groups,
                                                         int* __restrict__ rowroot, int32_t* __restrict__ group_out,
                                                         int32_t* __restrict__ origin_out) {
    __shared__ int wavecount[kThreads / 64][kClasses];
    const int i = blockIdx.x * kChunk + threadIdx.x;
    const int cls = root_class(i, nstar, label, size);
    int rank, total[kClasses];
    chunk_ranks(cls, wavecount, rank, total);
    if (cls < 0) return;
    const int row = offset[cls * gridDim.x + blockIdx.x] + rank;
    if (row >= max_groups) return;
    GroupRow g;
    group_row(i, size, slots, yx, g);
    rowroot[row] = i;
    int32_t* out = group_out + (size_t)row * 8;
    out[0] = g.n;
    out[1] = g.flags;
    out[2] = i;
    out[3] = 0;
#pragma unroll
    for (int s = 0; s < kMaxGroup; ++s) out[4 + s] = g.member[s];
    if (origin_out) {
        origin_out[(size_t)row * 2] = g.origin[0];
        origin_out[(size_t)row * 2 + 1] = g.origin[1];
    }
}

// One thread per output row g: the filler rows behind the groups; the eight doubles [8 g, 8 g + 8) of shift_out, which
// hold the shifts of class k (k = 1 .. 4 members, rows o_k .. o_k + c_k - 1) at a pitch of 2 k doubles from 8 o_k on and
// zero elsewhere; the counts.
__global__ __launch_bounds__(kThreads) void k_group_tail(int nchunk, const int* __restrict__ offset,
                                                         const int* __restrict__ size, const int* __restrict__ slots,
                                                         const double2* __restrict__ yx,
                                                         const int* __restrict__ rowroot, int max_groups,
                                                         int32_t* __restrict__ group_out,
                                                         int32_t* __restrict__ origin_out,
                                                         double* __restrict__ shift_out, int32_t* __restrict__ count_out) {
    const unsigned place = blockIdx.x * kThreads + threadIdx.x;      // (max_groups may be close to 2^31)
    if (place >= (unsigned)max_groups) return;
    const int g = (int)place;
    const int total = offset[kClasses * nchunk];
    if (g == 0) {
        count_out[0] = total;
        for (int c = 0; c < kClasses; ++c) count_out[1 + c] = offset[(c + 1) * nchunk] - offset[c * nchunk];
    }
    if (g >= total) {
        int32_t* out = group_out + (size_t)g * 8;
#pragma unroll
        for (int s = 0; s < 8; ++s) out[s] = s < 4 ? 0 : -1;
        if (origin_out) origin_out[(size_t)g * 2] = origin_out[(size_t)g * 2 + 1] = kFillerOrigin;
    }
    if (!shift_out) return;
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0;
    int k = 0, ok = 0, ck = 0;              // members, first row and rows of the class row g lies in
    for (int c = 0; c < kMaxGroup; ++c) {
        const int o = offset[c * nchunk], e = offset[(c + 1) * nchunk];
        if (g >= o && g < e) k = c + 1, ok = o, ck = e - o;
    }
    if (k) {
        GroupRow row;
        long long have = -1;
        for (int j = 0; j < 8; ++j) {
            const long long q = 8ll * (g - ok) + j, r = q / (2 * k);
            const int rem = (int)(q - r * 2 * k);
            if (r >= ck || ok + r >= max_groups) break;
            if (r != have) {
                group_row(rowroot[ok + r], size, slots, yx, row);
                have = r;
            }
            // (selected by comparisons, not by a variable index, so that the row stays in registers)
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < kMaxGroup; ++m)
                if (m == rem >> 1) s = row.shift[m][rem & 1];
            v[j] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) shift_out[(size_t)g * 8 + j] = v[j];
}

// The workspace: yx [nstar] double2; then ints: cellcount [nc], cursor [nc], celloff [nc + 1], cellstars, kind, parent,
// size [nstar] each, slots [3 nstar], count [5 nchunk], offset [5 nchunk + 1], rowroot [min(nstar, max_groups)]
struct GroupWork {
    int nc, nchunk;
    double2* yx;
    int *cellcount, *cursor, *celloff, *cellstars, *kind, *parent, *size, *slots, *count, *offset, *rowroot;
    GroupWork(WorkspaceCarver& ws, int ny, int nx, int nstar, int max_groups)
        : nc(cells(ny) * cells(nx)), nchunk((nstar + kChunk - 1) / kChunk), yx(ws.take<double2>(nstar)),
          cellcount(ws.take<int>(nc)), cursor(ws.take<int>(nc)), celloff(ws.take<int>((size_t)nc + 1)),
          cellstars(ws.take<int>(nstar)), kind(ws.take<int>(nstar)), parent(ws.take<int>(nstar)),
          size(ws.take<int>(nstar)), slots(ws.take<int>((size_t)nstar * (kMaxGroup - 1))),
          count(ws.take<int>((size_t)kClasses * nchunk)), offset(ws.take<int>((size_t)kClasses * nchunk + 1)),
          rowroot(ws.take<int>(nstar < max_groups ? nstar : max_groups)) {}
};

}  // namespace

size_t group_workspace_bytes(int ny, int nx, int nstar, int max_groups) {
    return workspace_bytes<GroupWork>(ny, nx, nstar, max_groups);
}

void launch_group_stars(hipStream_t s, int ny, int nx, int nstar, const double* d_pos, int stride, double crit,
                        int max_groups, int32_t* d_label_out, int32_t* d_group_out, int32_t* d_origin_out,
                        double* d_shift_out, int32_t* d_count_out, void* d_ws) {
    WorkspaceCarver ws(d_ws);
    const GroupWork w(ws, ny, nx, nstar, max_groups);
    const int nchunk = w.nchunk;
    const double c2 = crit * crit;
    (void)hipMemsetAsync(w.cellcount, 0, (size_t)2 * w.nc * sizeof(int), s);         // cellcount and cursor
    hipLaunchKernelGGL(k_group_init, dim3(nchunk), dim3(kThreads), 0, s, ny, nx, nstar, d_pos, stride, w.yx, w.kind,
                       w.parent, w.size, w.slots, w.cellcount);
    launch_scan_counts(s, w.nc, w.cellcount, w.celloff);
    hipLaunchKernelGGL(k_group_scatter, dim3(nchunk), dim3(kThreads), 0, s, nx, nstar, w.yx, w.kind, w.celloff, w.cursor,
                       w.cellstars);
    hipLaunchKernelGGL(k_group_link, dim3(nchunk), dim3(kThreads), 0, s, ny, nx, nstar, w.yx, w.kind, c2, w.celloff,
                       w.cellstars, w.parent);
    hipLaunchKernelGGL(k_group_gather, dim3(nchunk), dim3(kThreads), 0, s, nstar, w.kind, w.parent, w.size, w.slots,
                       d_label_out);
    hipLaunchKernelGGL(k_group_count, dim3(nchunk), dim3(kThreads), 0, s, nstar, d_label_out, w.size, w.count);
    launch_scan_counts(s, kClasses * nchunk, w.count, w.offset);
    hipLaunchKernelGGL(k_group_rows, dim3(nchunk), dim3(kThreads), 0, s, nstar, d_label_out, w.size, w.slots, w.yx,
                       w.offset, max_groups, w.rowroot, d_group_out, d_origin_out);
    hipLaunchKernelGGL(k_group_tail, dim3((max_groups - 1) / kThreads + 1), dim3(kThreads), 0, s, nchunk, w.offset,
                       w.size, w.slots, w.yx, w.rowroot, max_groups, d_group_out, d_origin_out, d_shift_out, d_count_out);
}

}  // namespace mpsfr
