// What the tiled renderers share (nm_render.hip: plates; nm_mesh.hip: triangles and skeletons): the kernels' copy of the camera and the
// scan that turns the counts per (frame, tile) into the tile lists' offsets.  Moved here from nm_render.hip unchanged.
#pragma once
#include "nm_render.h"

namespace {

struct RenderCam {
    double e[12];                     // rows 0 .. 2 of the world -> camera extrinsic
    double fx, fy, cx, cy, near;
    int W, H, TX, TY;                 // image size, tiles along x and y
};

// exclusive scan over the workgroup; `total`: the sum of all 256 values
__device__ __forceinline__ long long render_block_scan(long long v, long long* sh, long long& total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < NM_RENDER_BLOCK; off <<= 1) {
        const long long t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const long long incl = sh[tid];
    total = sh[NM_RENDER_BLOCK - 1];
    __syncthreads();
    return incl - v;
}

// grid ceil(nt / 1024): off[g] = the exclusive prefix of counts inside the workgroup's 1024 tiles, bsum[blk] = their sum
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_scan_local_kernel(const int* __restrict__ counts, long long nt, long long* __restrict__ off,
                                                                             long long* __restrict__ bsum) {
    __shared__ long long sh[NM_RENDER_BLOCK];
    constexpr int PER = NM_RENDER_SCAN / NM_RENDER_BLOCK;
    const long long g0 = (long long)blockIdx.x * NM_RENDER_SCAN + (long long)threadIdx.x * PER;
    long long v[PER], sum = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) { v[u] = g0 + u < nt ? (long long)counts[g0 + u] : 0; sum += v[u]; }
    long long total, run = render_block_scan(sum, sh, total);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (g0 + u < nt) off[g0 + u] = run;
        run += v[u];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum becomes its own exclusive prefix, off[nt] = the total
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_scan_sums_kernel(long long* __restrict__ bsum, long long nblk, long long nt, long long* __restrict__ off) {
    __shared__ long long sh[NM_RENDER_BLOCK];
    long long carry = 0;
    for (long long b0 = 0; b0 < nblk; b0 += NM_RENDER_BLOCK) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < nblk ? bsum[b] : 0;
        long long total;
        const long long ex = render_block_scan(v, sh, total);
        if (b < nblk) bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) off[nt] = carry;
}

// grid ceil(nt / 1024): off[g] += bsum[workgroup]
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_scan_add_kernel(const long long* __restrict__ bsum, long long nt, long long* __restrict__ off) {
    constexpr int PER = NM_RENDER_SCAN / NM_RENDER_BLOCK;
    const long long g0 = (long long)blockIdx.x * NM_RENDER_SCAN + (long long)threadIdx.x * PER, add = bsum[blockIdx.x];
#pragma unroll
    for (int u = 0; u < PER; ++u)
        if (g0 + u < nt) off[g0 + u] += add;
}

}  // namespace
