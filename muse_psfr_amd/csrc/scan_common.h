// The exclusive scan of up to a few million counts by one workgroup (render.hip: the tile counts of the renderer;
// find.hip: the peak counts of the star finder): every thread sums a contiguous share, the shares are scanned in LDS.
#pragma once
#include <hip/hip_runtime.h>

namespace mpsfr {

constexpr int kScanThreads = 1024;

// offset[t] = sum of count[0 .. t - 1], offset[nt] = the total; `part`: kScanThreads ints of LDS
__device__ __forceinline__ void scan_shares(int nt, const int* __restrict__ count, int* __restrict__ offset, int* part) {
    const int tid = threadIdx.x;
    const int per = (nt + kScanThreads - 1) / kScanThreads;
    const int b = min(tid * per, nt), e = min(b + per, nt);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += count[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = b; i < e; ++i) {
        offset[i] = run;
        run += count[i];
    }
    if (tid == kScanThreads - 1) offset[nt] = part[tid];
}

}  // namespace mpsfr
