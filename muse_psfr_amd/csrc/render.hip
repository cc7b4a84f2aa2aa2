// Frame-level PSF photometry: k_cut_stamps gathers 40 x 40 stamps out of a frame, and the
// renderer adds or subtracts scaled, resampled model stamps in a frame as a gather over 32 x 32 frame tiles:
//   k_render_prepare  one thread per star: validates it, writes star_out, counts the star on the tiles its footprint
//                     (the kPsfSide x kPsfSide window around its stamp) reaches; with `accept` (the frame fit of
//                     frame_fit.hip, which has judged the stars already) only the stars it marks are listed
//   k_scan_counts     exclusive scan of the tile counts (one workgroup; the finder and the grouping scan with it too)
//   k_render_fill     writes each star's index into the lists of its tiles at an atomic cursor (arbitrary order)
//   k_render_tiles    one workgroup per tile: sorts its list by star index, then walks it in that order -- the model
//                     stamp part the tile needs goes into LDS (two buffers, the next star fetched while this one is
//                     evaluated), every thread keeps four pixels in registers
//   k_render_sort     (the layers of a cube, cube_fit.hip) sorts every tile's list once, in place; k_render_tiles<true>
//                     then walks the frames of a batch of layers over the sorted lists, which hold every placed star,
//                     and skips the stars its layer has not accepted
// The order of the sum at a pixel is the star index, whatever the tile grid or the scheduling; no floating-point atomics.
// Arithmetic is fp64 in both precision modes; P~ is psf_interp of fit_psf_common.h with KeysTaps<double>.
#include <type_traits>

#include "frame_common.h"

namespace mpsfr {
namespace {

constexpr int kTile = 32;                                     // frame tile side: kFrameTile, spelt out for the layout below
constexpr int kTileThreads = 256;
constexpr int kTileRows = kTileThreads / kTile;               // threads per tile column
constexpr int kTilePix = kTile / kTileRows;                   // pixels per thread: adjacent rows of one column
constexpr int kWaveRows = 64 / kTile * kTilePix;               // tile rows one wave holds
constexpr int kStageSide = kTile + 3;                         // model rows / columns the 4 taps of a tile touch
constexpr int kStageStride = kStageSide + 1;
constexpr int kStageLoads = (kStageSide * kStageSide + kTileThreads - 1) / kTileThreads;     // per thread
constexpr int kSortChunk = 256;                               // MPSFR_RENDER_SORT_CHUNK: lists up to here sort in LDS
constexpr int kScanThreads = 1024;
static_assert(kTile == kFrameTile, "the lists are built (RenderLists) and walked on one tile grid");
static_assert(kTile * kTile == kTileThreads * kTilePix && kTileRows * kTile == kTileThreads, "tile layout");
static_assert(kSortChunk == kTileThreads, "one list entry per thread in the LDS copy");

__global__ __launch_bounds__(256) void k_cut_stamps(int ny, int nx, const double* __restrict__ image,
                                                    const double* __restrict__ var, StarList stars,
                                                    double* __restrict__ out, double* __restrict__ var_out) {
    const int k = blockIdx.x;
    const FrameStar star(stars, k);              // (any origin: a stamp off the frame is NaN)
    const long long op = star.op, oq = star.oq;
    for (int i = threadIdx.x; i < NS * NS; i += 256) {
        const int p = i / NS, q = i - p * NS;
        const long long Y = op + p, X = oq + q;
        const bool in = Y >= 0 && Y < ny && X >= 0 && X < nx;
        const size_t src = in ? (size_t)Y * nx + (size_t)X : 0;
        const size_t dst = (size_t)k * (NS * NS) + i;
        const double d = image[src];
        out[dst] = in ? d : __builtin_nan("");
        if (var) {
            const double v = var[src];
            var_out[dst] = in ? v : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void k_render_prepare(int ny, int nx, int ntx, StarList stars,
                                                        const double* __restrict__ scale,
                                                        const int32_t* __restrict__ accept, int* __restrict__ count,
                                                        int* __restrict__ status, double* __restrict__ star_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= stars.nstar) return;
    const FrameStar star(stars, k);
    // (neither accept nor scale: the lists of a cube, from what places a star alone -- index, origin, footprint)
    const bool ok = accept  ? star.valid(stars.npsf) && accept[k] != 0
                    : scale ? star.valid(stars.npsf) && fabs(scale[k]) < __builtin_inf()
                            : star.placed(stars.npsf);
    int st = 2, npix = 0;
    if (ok) {
        int y0, y1, x0, x1;
        const bool hit = star.footprint(ny, nx, y0, y1, x0, x1);
        st = hit ? 0 : 1;
        if (hit) {
            npix = (y1 - y0) * (x1 - x0);
            for (int ty = y0 / kTile; ty <= (y1 - 1) / kTile; ++ty)
                for (int tx = x0 / kTile; tx <= (x1 - 1) / kTile; ++tx) atomicAdd(&count[ty * ntx + tx], 1);
        }
    }
    status[k] = st;
    if (star_out) {
        star_out[4 * (size_t)k + 0] = (double)st;
        star_out[4 * (size_t)k + 1] = (double)npix;
        star_out[4 * (size_t)k + 2] = 0.0;
        star_out[4 * (size_t)k + 3] = 0.0;
    }
}

// The exclusive scan of up to a few million counts by one workgroup: offset[t] = sum of count[0 .. t - 1], offset[nt] =
// the total.  Every thread sums a contiguous share, the shares are scanned in LDS.
__global__ __launch_bounds__(kScanThreads) void k_scan_counts(int nt, const int* __restrict__ count,
                                                              int* __restrict__ offset) {
    __shared__ int part[kScanThreads];
    const int tid = threadIdx.x;
    const int per = (nt + kScanThreads - 1) / kScanThreads;
    const int b = min(tid * per, nt), e = min(b + per, nt);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += count[i];
    part[tid] = sum;
    block_scan<kScanThreads>(part);
    int run = part[tid] - sum;
    for (int i = b; i < e; ++i) {
        offset[i] = run;
        run += count[i];
    }
    if (tid == kScanThreads - 1) offset[nt] = part[tid];
}

__global__ __launch_bounds__(256) void k_render_fill(int ny, int nx, int ntx, StarList stars,
                                                     const int* __restrict__ status, const int* __restrict__ offset,
                                                     int* __restrict__ cursor, int* __restrict__ pairs) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= stars.nstar || status[k] != 0) return;
    int y0, y1, x0, x1;
    FrameStar(stars, k).footprint(ny, nx, y0, y1, x0, x1);
    for (int ty = y0 / kTile; ty <= (y1 - 1) / kTile; ++ty)
        for (int tx = x0 / kTile; tx <= (x1 - 1) / kTile; ++tx) {
            const int t = ty * ntx + tx;
            pairs[offset[t] + atomicAdd(&cursor[t], 1)] = k;
        }
}

// Ascending bitonic sort of v[0 .. n - 1] by the whole workgroup (n is the same for all its threads); v is in LDS or,
// for a list longer than kSortChunk, the tile's own part of the work list in memory.  Every compare-exchange puts the
// smaller value at the lower place, so the places n .. 2^k - 1 count as +infinity without being stored.
__device__ void sort_indices(int* v, int n) {
    __syncthreads();
    if (n < 2) return;
    int m = 2;
    while (m < n) m <<= 1;
    const int tid = threadIdx.x;
    for (int k = 2; k <= m; k <<= 1) {
        const int hk = k >> 1;
        for (int i = tid; i < (m >> 1); i += kTileThreads) {
            const int off = i & (hk - 1), a = ((i - off) << 1) + off, b = a + k - 1 - 2 * off;
            if (b < n) {
                const int va = v[a], vb = v[b];
                if (va > vb) {
                    v[a] = vb;
                    v[b] = va;
                }
            }
        }
        __syncthreads();
        for (int j = hk >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < (m >> 1); i += kTileThreads) {
                const int off = i & (j - 1), a = ((i - off) << 1) + off, b = a + j;
                if (b < n) {
                    const int va = v[a], vb = v[b];
                    if (va > vb) {
                        v[a] = vb;
                        v[b] = va;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// every tile's list sorted once, in place, for the walks that take it sorted (k_render_tiles<true>)
__global__ __launch_bounds__(kTileThreads) void k_render_sort(const int* __restrict__ offset, int* pairs) {
    const int first = offset[blockIdx.x];
    sort_indices(pairs + first, offset[blockIdx.x + 1] - first);
}

// One star as a tile sees it: its parameters (the same for all threads) and the model pixel of stage[0][0]
struct TileStar {
    int op, oq, r0, c0;
    double sc;
    const double* P;
    KeysTaps<double> ty{0.0}, tx{0.0};
    __device__ __forceinline__ void load(int k, int Y0, int X0, const StarList& stars, const double* scale) {
        const FrameStar star(stars, k);
        op = star.op;
        oq = star.oq;
        sc = scale[k];
        ty = KeysTaps<double>(star.dp);
        tx = KeysTaps<double>(star.dq);
        P = star.model(stars);
        r0 = Y0 - op + ty.f - 1;
        c0 = X0 - oq + tx.f - 1;
    }
    // this thread's share of the kStageSide^2 model pixels the tile's taps can touch, zero outside the model
    __device__ __forceinline__ void fetch(int tid, double (&pre)[kStageLoads]) const {
#pragma unroll
        for (int m = 0; m < kStageLoads; ++m) {
            const int e = tid + m * kTileThreads, si = e / kStageSide, sj = e - si * kStageSide;
            pre[m] = model_pixel(P, r0 + si, c0 + sj, e < kStageSide * kStageSide);
        }
    }
};

// acc +- scale * val, the product rounded before the sum
__device__ __forceinline__ double add_term(double acc, double scale, double val, bool subtract) {
#pragma clang fp contract(off)
    const double t = scale * val;
    return subtract ? acc - t : acc + t;
}

// LAYERS: the frames of a batch of layers (blockIdx.z) side by side -- frames of ny nx pixels, scales at a pitch of
// lay.scale_pitch, done words at lay.done_pitch, lay.accept [layers][nstar] --, over lists that are sorted already and
// hold every placed star: a star its layer has not accepted is skipped.
struct NoLayers {};
struct WalkLayers {
    const int32_t* accept;
    int scale_pitch, done_pitch;
};
template <bool LAYERS>
__global__ __launch_bounds__(kTileThreads) void k_render_tiles(int ny, int nx, const double* image_in, StarList stars,
                                                               const double* __restrict__ scale, int subtract,
                                                               const int* __restrict__ offset, int* pairs,
                                                               const int32_t* __restrict__ done, double* image_out,
                                                               std::conditional_t<LAYERS, WalkLayers, NoLayers> lay) {
    __shared__ double stage[2 * kStageSide * kStageStride];
    __shared__ int slist[LAYERS ? 1 : kSortChunk];
    const int32_t* accept = nullptr;
    if constexpr (LAYERS) {
        const int b = blockIdx.z;
        if (done) done += (size_t)b * lay.done_pitch;
        if (image_in) image_in += (size_t)b * ny * nx;
        image_out += (size_t)b * ny * nx;
        scale += (size_t)b * lay.scale_pitch;
        accept = lay.accept + (size_t)b * stars.nstar;
        stars.layer = b;
    }
    if (done && *done) return;          // (a queued walk of the frame fit after its stop test has passed)
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly0 = tid / kTile;
    const int t = blockIdx.y * gridDim.x + blockIdx.x;
    const int Y0 = blockIdx.y * kTile, X0 = blockIdx.x * kTile, X = X0 + lx;
    const int first = offset[t], n = offset[t + 1] - first;
    // (image_out may be image_in: every pixel is read here and written at the end by the same thread)
    double acc[kTilePix];
    bool on[kTilePix];
#pragma unroll
    for (int j = 0; j < kTilePix; ++j) {
        const int Y = Y0 + kTilePix * ly0 + j;
        on[j] = Y < ny && X < nx;
        acc[j] = on[j] && image_in ? image_in[(size_t)Y * nx + X] : 0.0;
    }
    const int* list = slist;
    if constexpr (LAYERS) {
        list = pairs + first;
    } else if (n <= kSortChunk) {
        if (tid < n) slist[tid] = pairs[first + tid];
        sort_indices(slist, n);
    } else {
        sort_indices(pairs + first, n);
        list = pairs + first;
    }
    // the first place of the list from i on whose star takes part
    auto next = [&](int i) {
        if constexpr (LAYERS)
            while (i < n && !accept[list[i]]) ++i;
        return i;
    };
    // Star i + 1 is fetched into registers while star i is evaluated, and the stage alternates between two buffers:
    // one barrier per star (a buffer is rewritten two stars later, behind the barrier that every thread reaches only
    // after its last read of it).
    TileStar cur, nxt;
    double pre[kStageLoads];
    int i = next(0);
    if (i < n) {
        cur.load(list[i], Y0, X0, stars, scale);
        cur.fetch(tid, pre);
    }
    for (int turn = 0; i < n; ++turn) {
        double* buf = stage + (turn & 1) * (kStageSide * kStageStride);
#pragma unroll
        for (int m = 0; m < kStageLoads; ++m) {
            const int e = tid + m * kTileThreads;
            if (e < kStageSide * kStageSide) buf[(e / kStageSide) * kStageStride + e % kStageSide] = pre[m];
        }
        i = next(i + 1);
        if (i < n) {
            nxt.load(list[i], Y0, X0, stars, scale);
            nxt.fetch(tid, pre);
        }
        __syncthreads();
        const StagedStamp<kStageStride> st{buf};
        const int q = X - cur.oq;
        // (a wave holds kWaveRows rows of the tile: it skips a star whose footprint lies above or below them)
        const int pw = Y0 + (tid / 64) * kWaveRows - cur.op;
        if (pw + kWaveRows > -kPsfApron && pw < NS + kPsfApron) {
#pragma unroll
            for (int j = 0; j < kTilePix; ++j) {
                // (evaluated on every pixel of the wave -- the stage covers the whole tile, and the four rows of a
                // thread share the loads of their taps --, applied on the footprint only)
                const int ly = kTilePix * ly0 + j, p = Y0 + ly - cur.op;
                double val, gy, gx;
                psf_interp<double, false>(st, ly * kStageStride + lx, p, q, cur.ty, cur.tx, val, gy, gx);
                const bool inside = on[j] && p >= -kPsfApron && p < NS + kPsfApron && q >= -kPsfApron &&
                                    q < NS + kPsfApron;
                const double sum = add_term(acc[j], cur.sc, val, subtract != 0);
                acc[j] = inside ? sum : acc[j];
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (int j = 0; j < kTilePix; ++j) {
        const int Y = Y0 + kTilePix * ly0 + j;
        if (on[j]) image_out[(size_t)Y * nx + X] = acc[j];
    }
}

}  // namespace

void launch_cut_stamps(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, int nstar,
                       const int32_t* d_origin, double* d_stamps, double* d_var_out) {
    const StarList stars{nstar, 0, nullptr, nullptr, d_origin, nullptr};          // the origins alone
    hipLaunchKernelGGL(k_cut_stamps, dim3(nstar), dim3(256), 0, s, ny, nx, d_image, d_var, stars, d_stamps, d_var_out);
}

void launch_scan_counts(hipStream_t s, int nt, const int* d_count, int* d_offset) {
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(kScanThreads), 0, s, nt, d_count, d_offset);
}

size_t render_workspace_bytes(int ny, int nx, int nstar) { return workspace_bytes<RenderLists>(ny, nx, nstar); }

void launch_render_lists(hipStream_t s, int ny, int nx, StarList stars, const double* d_scale, const int32_t* d_accept,
                         double* d_star_out, void* d_ws) {
    static_assert(kPsfSide + kTile - 1 <= 3 * kTile, "a footprint reaches at most 3 x 3 tiles");
    WorkspaceCarver ws(d_ws);
    const RenderLists l(ws, ny, nx, stars.nstar);
    (void)hipMemsetAsync(l.count, 0, (size_t)2 * l.nt * sizeof(int), s);          // count and cursor
    const int gstar = (stars.nstar + 255) / 256;
    hipLaunchKernelGGL(k_render_prepare, dim3(gstar), dim3(256), 0, s, ny, nx, l.ntx, stars, d_scale, d_accept, l.count,
                       l.status, d_star_out);
    launch_scan_counts(s, l.nt, l.count, l.offset);
    hipLaunchKernelGGL(k_render_fill, dim3(gstar), dim3(256), 0, s, ny, nx, l.ntx, stars, l.status, l.offset, l.cursor,
                       l.pairs);
}

void launch_render_walk(hipStream_t s, int ny, int nx, const double* d_image_in, StarList stars, const double* d_scale,
                        bool subtract, double* d_image_out, void* d_ws, const int32_t* d_done) {
    WorkspaceCarver ws(d_ws);
    const RenderLists l(ws, ny, nx, stars.nstar);
    hipLaunchKernelGGL(k_render_tiles<false>, dim3(l.ntx, l.nty), dim3(kTileThreads), 0, s, ny, nx, d_image_in, stars,
                       d_scale, subtract ? 1 : 0, l.offset, l.pairs, d_done, d_image_out, NoLayers{});
}

void launch_render_sort(hipStream_t s, int ny, int nx, int nstar, void* d_ws) {
    WorkspaceCarver ws(d_ws);
    const RenderLists l(ws, ny, nx, nstar);
    hipLaunchKernelGGL(k_render_sort, dim3(l.nt), dim3(kTileThreads), 0, s, l.offset, l.pairs);
}

void launch_render_walk_layers(hipStream_t s, int ny, int nx, int layers, const double* d_image_in, StarList stars,
                               const double* d_scale, int scale_pitch, const int32_t* d_accept, bool subtract,
                               double* d_image_out, void* d_ws, const int32_t* d_done, int done_pitch) {
    WorkspaceCarver ws(d_ws);
    const RenderLists l(ws, ny, nx, stars.nstar);
    hipLaunchKernelGGL(k_render_tiles<true>, dim3(l.ntx, l.nty, layers), dim3(kTileThreads), 0, s, ny, nx, d_image_in,
                       stars, d_scale, subtract ? 1 : 0, l.offset, l.pairs, d_done, d_image_out,
                       WalkLayers{d_accept, scale_pitch, done_pitch});
}

void launch_render_stars(hipStream_t s, int ny, int nx, const double* d_image_in, StarList stars, const double* d_scale,
                         bool subtract, double* d_image_out, double* d_star_out, void* d_ws) {
    launch_render_lists(s, ny, nx, stars, d_scale, nullptr, d_star_out, d_ws);
    launch_render_walk(s, ny, nx, d_image_in, stars, d_scale, subtract, d_image_out, d_ws, nullptr);
}

}  // namespace mpsfr
