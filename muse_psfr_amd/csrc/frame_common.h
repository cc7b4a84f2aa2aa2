// What the frame calls share (render.hip, frame_fit.hip and cube_fit.hip, find.hip, group.hip; DESIGN.md sections 21 to 25): one star
// of a StarList (kernels.h) as every kernel sees it, with the rule that admits it and its footprint (FrameStar); the
// frame tile; a model stamp part staged in LDS (StagedStamp) and the pixel rule of staging it (model_pixel); the scan
// of a workgroup's counts in LDS (block_scan); and the one description of a workspace that both *_workspace_bytes and
// its launcher read (WorkspaceCarver, RenderLists).  Everything here has internal linkage.
#pragma once
#include "fit_psf_common.h"

namespace mpsfr {
namespace {

constexpr int kFrameTile = 32;                 // side of a frame tile of the renderer and the frame fit
constexpr int kMaxOrigin = 1 << 30;            // |origin| bound: origin +- the footprint stays an int
constexpr int kFillerOrigin = -kMaxOrigin;     // both origins of a filler row of the finder and the grouping
inline int frame_tiles(int n) { return (n + kFrameTile - 1) / kFrameTile; }

// Star k of a list: the frame pixel of its stamp's pixel [0][0], its model stamp, its shift
struct FrameStar {
    int op, oq, ix;
    double dp, dq;
    __device__ __forceinline__ FrameStar(const StarList& l, int k)
        : op(l.origin[2 * k]), oq(l.origin[2 * k + 1]), ix(l.index ? l.index[k] : k),
          dp(l.shift ? l.shift[2 * k] : 0.0), dq(l.shift ? l.shift[2 * k + 1] : 0.0) {
        if (l.lshift) {                        // (a layer of a cube: its offset, common to all stars)
            dp = dp + l.lshift[2 * l.layer];
            dq = dq + l.lshift[2 * l.layer + 1];
        }
    }
    // index and origin in range: what places a star, whatever its shift
    __device__ __forceinline__ bool placed(int npsf) const {
        return (unsigned)ix < (unsigned)npsf && op >= -kMaxOrigin && op <= kMaxOrigin && oq >= -kMaxOrigin &&
               oq <= kMaxOrigin;
    }
    // the rule of the device form: anything else is status 2 (a NaN shift fails)
    __device__ __forceinline__ bool valid(int npsf) const { return placed(npsf) && psf_inside(dp, dq); }
    // the frame pixels inside the footprint (the kPsfSide x kPsfSide window around the stamp): rows y0 .. y1 - 1,
    // columns x0 .. x1 - 1; false if there is none
    __device__ __forceinline__ bool footprint(int ny, int nx, int& y0, int& y1, int& x0, int& x1) const {
        y0 = max(op - kPsfApron, 0);
        y1 = min(op + NS + kPsfApron, ny);
        x0 = max(oq - kPsfApron, 0);
        x1 = min(oq + NS + kPsfApron, nx);
        return y0 < y1 && x0 < x1;
    }
    // the centre in frame pixels
    __device__ __forceinline__ double cy() const { return (double)(op + NS / 2) + dp; }
    __device__ __forceinline__ double cx() const { return (double)(oq + NS / 2) + dq; }
    __device__ __forceinline__ const double* model(const StarList& l) const {
        return l.psf + ((size_t)ix * l.nl + l.layer) * (NS * NS);
    }
};

// Pixel (r, c) of the fp64 model stamp P in memory, or zero outside the model (and where it is not `wanted`); the load
// is unconditional, of pixel 0 where the answer is zero.  (GlobalStamp::at of fit_psf_common.h spells the same rule out
// with its scale inside the selection: sharing it there moved the instructions of the fit kernels.)
__device__ __forceinline__ double model_pixel(const double* P, int r, int c, bool wanted = true) {
    const bool in = wanted && (unsigned)r < (unsigned)NS && (unsigned)c < (unsigned)NS;
    const double v = P[in ? r * NS + c : 0];
    return in ? v : 0.0;
}

// a part of a model stamp in LDS at a row pitch of STRIDE, zero outside the model: tap (a, b) of the pixel at offset o
template <int STRIDE>
struct StagedStamp {
    const double* base;
    template <typename RE>
    __device__ __forceinline__ RE at(int o, int, int, int a, int b) const {
        return (RE)base[o + a * STRIDE + b];
    }
};

// part[tid] becomes the sum of part[0 .. tid] over the T threads of the workgroup; part: T ints of LDS
template <int T>
__device__ __forceinline__ void block_scan(int* part) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const int add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
}

// A workspace described once, as a struct Work whose constructor takes its arrays in order: take<T>(n) aligns to T (or
// to `align` bytes), returns the place of n values -- nullptr without a base -- and moves on.  The launcher builds Work
// on d_ws; workspace_bytes<Work> builds it on no base and returns where the carver got to.
class WorkspaceCarver {
    char* base_;
    size_t off_ = 0;

public:
    explicit WorkspaceCarver(void* base) : base_((char*)base) {}
    template <typename T>
    T* take(size_t n, size_t align = alignof(T)) {
        off_ = (off_ + align - 1) & ~(align - 1);
        T* p = base_ ? (T*)(base_ + off_) : nullptr;
        off_ += n * sizeof(T);
        return p;
    }
    size_t bytes() const { return off_; }
};
template <typename Work, typename... Shape>
size_t workspace_bytes(Shape... shape) {
    WorkspaceCarver ws(nullptr);
    Work(ws, shape...);
    return ws.bytes();
}

// The work lists of the renderer in a workspace: count [nt], cursor [nt], offset [nt + 1], status [nstar], pairs
// [9 nstar] -- a footprint reaches at most 3 x 3 tiles
struct RenderLists {
    int ntx, nty, nt;                           // frame tiles each way, nt = ntx nty
    int *count, *cursor, *offset, *status, *pairs;
    RenderLists(WorkspaceCarver& ws, int ny, int nx, int nstar)
        : ntx(frame_tiles(nx)), nty(frame_tiles(ny)), nt(ntx * nty), count(ws.take<int>(nt)), cursor(ws.take<int>(nt)),
          offset(ws.take<int>((size_t)nt + 1)), status(ws.take<int>(nstar)), pairs(ws.take<int>((size_t)9 * nstar)) {}
};

}  // namespace
}  // namespace mpsfr
