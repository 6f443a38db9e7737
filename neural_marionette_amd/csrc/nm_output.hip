// Device output path: thresholded voxels to ordered point sets - what every consumer of the decoder's voxels in the reference does on
// the host before it draws anything (vis_generation.py:137-170, vis_interpolation.py:141-177, vis/visualize.py:58-59, :130-137): the
// in-place binarisation, np.where / torch.where per frame, the division into [-1, 1] coordinates, and the two-pass min_z / max_z of
// the last coordinate over a clip's frames with the per-point (z - min_z) / z_len of the shading - for B clips of T frames in two
// stream-ordered calls.  Normal estimation, colours and rendering stay with the caller.
//
// Order.  np.where / torch.where enumerate in row-major order, so the feature is a stream compaction that keeps the flat voxel order:
// frame after frame, and inside a frame by rising flat position p = (i * G + j) * G + k.  Three passes, none of which waits on
// another workgroup (no look-back, no spinning):
//   mask + count  occ_mask_kernel: a chunk of 64 occupancy words (4096 voxels) per workgroup; bit j of word w of a frame is its flat
//                 voxel 64 w + j, a frame is padded to whole words with zero bits.  Per chunk: the number of set bits and the min / max
//                 of the last-axis index k of its occupied voxels, as integers (an empty chunk holds INT_MAX / -1 and so adds nothing).
//   scan          occ_frame_kernel + occ_offsets_kernel: chunk figures -> frame figures -> offsets (F + 1, int64) and each clip's
//                 k-range over its T frames; occ_chunk_scan_kernel: the exclusive scan of the chunk counts inside each frame.
//   write         occ_write_kernel: reads the mask words only.  rank of a set bit = offsets[f] + its chunk's scan + popcount of the
//                 chunk's earlier words + popcount of the word's lower bits; thread r of a workgroup takes the chunk's r-th point, so
//                 consecutive ranks are written by consecutive lanes to consecutive rows.  Rows at or past `capacity` are skipped.
// nm_occupied_write depends on nothing but its arguments: it rebuilds the chunk scan from the mask words (1/32 of the voxels' bytes)
// instead of trusting workspace contents that another call on the context may have overwritten in between.
//
// Arithmetic (the library is built with -ffp-contract=off, both divisions are the correctly rounded ones):
//   float64 (numpy: int64 / float -> float64)   c = double(i) / ((G - 1) / 2.0) - 1.0
//   float32 (torch: int64 / float -> float32)   c = float(i) / float((G - 1) / 2.0) - 1.0f
//   depth (float64 only)                        (c_k - min_z) / (max_z - min_z), min_z / max_z = c of the clip's smallest / largest k;
//                                               a clip whose points share one k divides 0 by 0 like numpy: NaN.
// A clip without an occupied voxel keeps the scripts' initial values: z_range = (1e4, -1), z_idx_range = (INT_MAX, -1).
#include "nm_ctx.h"
#include "nm_output.h"
#include <climits>

namespace {

// threshold mode: what survives `x[x < thr] = 0; x[x >= thr] = 1` followed by np.where - NOT (v < thr), so a NaN is occupied;
// nonzero mode: torch.where(x) - v != 0 (NaN occupied, -0.0 empty)
template <int MODE> __device__ __forceinline__ bool occupied(float v, float thr) { return MODE == 0 ? !(v < thr) : v != 0.0f; }

// bit n of the low 16 bits of x -> bit 4 n
__device__ __forceinline__ unsigned long long spread4(unsigned long long x) {
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += nm_sx(v, off);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
    for (int off = 32; off > 0; off >>= 1) { const int q = nm_sx(v, off); v = q < v ? q : v; }
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int off = 32; off > 0; off >>= 1) { const int q = nm_sx(v, off); v = q > v ? q : v; }
    return v;
}

// ---- mask + count ----------------------------------------------------------------------------------------------------------------
// grid F * nC: workgroup f * nC + c takes words [64 c, 64 c + 64) of frame f; wavefront v of step s the four words from
// 64 c + 4 (4 s + v).  A tile that lies inside a 16-byte aligned frame is read with one 16-byte load per lane (lane l holds voxels
// 4 l .. 4 l + 3, so word q of the tile interleaves bits 16 q .. 16 q + 15 of the four ballots); the last tile of a frame and every
// tile of an unaligned frame with four 4-byte loads (lane l holds voxel 64 q + l: the ballot is the word).
template <int MODE>
__global__ __launch_bounds__(NM_OUT_BLOCK) void occ_mask_kernel(const float* __restrict__ vox, int G, int V, int W, int nC, float thr,
                                                                 unsigned long long* __restrict__ bits, int32_t* __restrict__ ccnt,
                                                                 int32_t* __restrict__ czmin, int32_t* __restrict__ czmax) {
    __shared__ int sh[3 * (NM_OUT_BLOCK / 64)];
    const int f = blockIdx.x / nC, c = blockIdx.x - f * nC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* fr = vox + (size_t)f * (size_t)V;
    unsigned long long* fb = bits + (size_t)f * (size_t)W;
    const bool aligned = (reinterpret_cast<uintptr_t>(fr) & 15) == 0;
    int cnt = 0, zmin = INT_MAX, zmax = -1;
    float4 q[NM_OUT_STEPS];                                     // every step's 16-byte load is issued before the first is used
#pragma unroll
    for (int s = 0; s < NM_OUT_STEPS; ++s) {
        const long long p0 = (long long)(c * NM_OUT_CHUNK_WORDS + (s * (NM_OUT_BLOCK / 64) + wave) * NM_OUT_TILE_WORDS) * 64;
        if (aligned && p0 + 64 * NM_OUT_TILE_WORDS <= (long long)V) q[s] = *reinterpret_cast<const float4*>(fr + p0 + 4 * lane);
    }
#pragma unroll
    for (int s = 0; s < NM_OUT_STEPS; ++s) {
        const int w0 = c * NM_OUT_CHUNK_WORDS + (s * (NM_OUT_BLOCK / 64) + wave) * NM_OUT_TILE_WORDS;
        if (w0 >= W) break;                                     // (the same for the whole wavefront)
        const long long p0 = (long long)w0 * 64;
        unsigned long long word[NM_OUT_TILE_WORDS];
        if (aligned && p0 + 64 * NM_OUT_TILE_WORDS <= (long long)V) {
            const float v[4] = {q[s].x, q[s].y, q[s].z, q[s].w};
            unsigned long long bal[4];
            int z = (int)((unsigned)(p0 + 4 * lane) % (unsigned)G);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool o = occupied<MODE>(v[k], thr);
                bal[k] = __ballot(o);
                if (o) { zmin = z < zmin ? z : zmin; zmax = z > zmax ? z : zmax; }
                z = z + 1 == G ? 0 : z + 1;
            }
#pragma unroll
            for (int w = 0; w < NM_OUT_TILE_WORDS; ++w)
                word[w] = spread4(bal[0] >> (16 * w)) | (spread4(bal[1] >> (16 * w)) << 1) | (spread4(bal[2] >> (16 * w)) << 2) |
                          (spread4(bal[3] >> (16 * w)) << 3);
        } else {
#pragma unroll
            for (int w = 0; w < NM_OUT_TILE_WORDS; ++w) {
                const long long p = p0 + 64 * w + lane;
                const bool o = p < (long long)V && occupied<MODE>(fr[p], thr);          // pad bits stay zero
                word[w] = __ballot(o);
                if (o) { const int z = (int)((unsigned)p % (unsigned)G); zmin = z < zmin ? z : zmin; zmax = z > zmax ? z : zmax; }
            }
        }
        unsigned long long mine = word[0];
#pragma unroll
        for (int w = 1; w < NM_OUT_TILE_WORDS; ++w) mine = lane == w ? word[w] : mine;
#pragma unroll
        for (int w = 0; w < NM_OUT_TILE_WORDS; ++w) cnt += __popcll(word[w]);
        if (lane < NM_OUT_TILE_WORDS && w0 + lane < W) fb[w0 + lane] = mine;
    }
    zmin = wave_min(zmin); zmax = wave_max(zmax);
    if (lane == 0) { sh[wave * 3] = cnt; sh[wave * 3 + 1] = zmin; sh[wave * 3 + 2] = zmax; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < NM_OUT_BLOCK / 64; ++v) {
            cnt += sh[v * 3];
            zmin = sh[v * 3 + 1] < zmin ? sh[v * 3 + 1] : zmin;
            zmax = sh[v * 3 + 2] > zmax ? sh[v * 3 + 2] : zmax;
        }
        ccnt[blockIdx.x] = cnt; czmin[blockIdx.x] = zmin; czmax[blockIdx.x] = zmax;
    }
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------
// grid F: the chunk figures of frame f -> fstat[3 f] = (count, min k, max k)
__global__ __launch_bounds__(NM_OUT_BLOCK) void occ_frame_kernel(const int32_t* __restrict__ ccnt, const int32_t* __restrict__ czmin,
                                                                 const int32_t* __restrict__ czmax, int nC, int32_t* __restrict__ fstat) {
    __shared__ int sh[3 * (NM_OUT_BLOCK / 64)];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0, zmin = INT_MAX, zmax = -1;
    for (int c = tid; c < nC; c += NM_OUT_BLOCK) {
        const size_t i = (size_t)f * nC + c;
        cnt += ccnt[i];
        zmin = czmin[i] < zmin ? czmin[i] : zmin;
        zmax = czmax[i] > zmax ? czmax[i] : zmax;
    }
    cnt = wave_sum(cnt); zmin = wave_min(zmin); zmax = wave_max(zmax);
    if (lane == 0) { sh[wave * 3] = cnt; sh[wave * 3 + 1] = zmin; sh[wave * 3 + 2] = zmax; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < NM_OUT_BLOCK / 64; ++v) {
            cnt += sh[v * 3];
            zmin = sh[v * 3 + 1] < zmin ? sh[v * 3 + 1] : zmin;
            zmax = sh[v * 3 + 2] > zmax ? sh[v * 3 + 2] : zmax;
        }
        fstat[3 * (size_t)f] = cnt; fstat[3 * (size_t)f + 1] = zmin; fstat[3 * (size_t)f + 2] = zmax;
    }
}

// exclusive scan of v over the workgroup through sh[NM_OUT_BLOCK]; *total = the workgroup's sum.  Ends with a barrier.
template <typename T> __device__ __forceinline__ T block_exclusive(T v, T* sh, T* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < NM_OUT_BLOCK; off <<= 1) {
        const T a = tid >= off ? sh[tid - off] : (T)0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    const T incl = sh[tid];
    *total = sh[NM_OUT_BLOCK - 1];
    __syncthreads();
    return incl - v;
}

template <typename CT> __device__ __forceinline__ CT coord_of(int i, CT half) { return (CT)i / half - (CT)1; }

// one workgroup: frame counts -> offsets (F + 1), and clip b's k-range over its T frames -> z_idx_range (B,2), z_range (B,2)
template <typename CT>
__global__ __launch_bounds__(NM_OUT_BLOCK) void occ_offsets_kernel(const int32_t* __restrict__ fstat, int B, int T, CT half,
                                                                   long long* __restrict__ offsets, int32_t* __restrict__ z_idx_range,
                                                                   CT* __restrict__ z_range) {
    __shared__ long long sh[NM_OUT_BLOCK];
    const int tid = threadIdx.x;
    const long long F = (long long)B * T;
    long long carry = 0;
    for (long long f0 = 0; f0 < F; f0 += NM_OUT_BLOCK) {
        const long long f = f0 + tid;
        const long long v = f < F ? (long long)fstat[3 * f] : 0;
        long long total;
        const long long ex = block_exclusive<long long>(v, sh, &total);
        if (f < F) offsets[f] = carry + ex;
        carry += total;
    }
    if (tid == 0) offsets[F] = carry;
    for (int b = tid; b < B; b += NM_OUT_BLOCK) {
        int zmin = INT_MAX, zmax = -1;
        for (int t = 0; t < T; ++t) {
            const int32_t* st = fstat + 3 * ((size_t)b * T + t);
            zmin = st[1] < zmin ? st[1] : zmin;
            zmax = st[2] > zmax ? st[2] : zmax;
        }
        z_idx_range[2 * b] = zmin; z_idx_range[2 * b + 1] = zmax;
        const bool any = zmax >= 0;
        z_range[2 * b] = any ? coord_of<CT>(zmin, half) : (CT)1e4;          // min_z = 1e4, max_z = -1 (vis_generation.py:143-144)
        z_range[2 * b + 1] = any ? coord_of<CT>(zmax, half) : (CT)-1;
    }
}

// grid F: coff[f * nC + c] = number of set bits in the chunks before c of frame f, from the mask words alone.  A thread per chunk:
// its 64 loads do not depend on one another, so a frame's words are in flight together (a wavefront per chunk, one load and one
// butterfly after the other, took 68 us for the 216 chunks of a 96^3 frame)
__global__ __launch_bounds__(NM_OUT_BLOCK) void occ_chunk_scan_kernel(const unsigned long long* __restrict__ bits, int W, int nC,
                                                                      int32_t* __restrict__ coff) {
    __shared__ int sh[NM_OUT_BLOCK];
    const int f = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* fb = bits + (size_t)f * (size_t)W;
    int carry = 0;
    for (int c0 = 0; c0 < nC; c0 += NM_OUT_BLOCK) {
        const int c = c0 + tid;
        int n = 0;
        if (c < nC) {
            const unsigned long long* cw = fb + (size_t)c * NM_OUT_CHUNK_WORDS;
            const int have = W - c * NM_OUT_CHUNK_WORDS;                     // (>= 1: c < nC)
            if (have >= NM_OUT_CHUNK_WORDS) {
#pragma unroll 16
                for (int i = 0; i < NM_OUT_CHUNK_WORDS; ++i) n += __popcll(cw[i]);
            } else {
                for (int i = 0; i < have; ++i) n += __popcll(cw[i]);
            }
        }
        int total;
        const int ex = block_exclusive<int>(n, sh, &total);
        if (c < nC) coff[(size_t)f * nC + c] = carry + ex;
        carry += total;
    }
}

// ---- write -----------------------------------------------------------------------------------------------------------------------
// grid F * nC: workgroup f * nC + c writes the points of chunk c of frame f.  The first wavefront loads the chunk's 64 words and
// scans their popcounts; thread r then finds the word holding the chunk's r-th set bit (binary search over the scan) and the bit
// inside it (binary descent over popcounts of the word's halves).
template <typename CT>
__global__ __launch_bounds__(NM_OUT_BLOCK) void occ_write_kernel(const unsigned long long* __restrict__ bits, const long long* __restrict__ offsets,
                                                                 const int32_t* __restrict__ coff, const int32_t* __restrict__ z_idx_range,
                                                                 int T, int G, int W, int nC, CT half, long long capacity,
                                                                 int32_t* __restrict__ idx, CT* __restrict__ coords, double* __restrict__ depth) {
    __shared__ unsigned long long wsh[NM_OUT_CHUNK_WORDS];
    __shared__ int pre[NM_OUT_CHUNK_WORDS + 1];
    const int f = blockIdx.x / nC, c = blockIdx.x - f * nC, tid = threadIdx.x;
    const long long base = offsets[f] + (long long)coff[blockIdx.x];
    if (base >= capacity) return;                                // (the same for the whole workgroup)
    if (tid < NM_OUT_CHUNK_WORDS) {
        const long long w = (long long)c * NM_OUT_CHUNK_WORDS + tid;
        const unsigned long long word = w < (long long)W ? bits[(size_t)f * (size_t)W + w] : 0ull;
        wsh[tid] = word;
        int incl = __popcll(word);
        for (int off = 1; off < 64; off <<= 1) { const int q = __shfl_up(incl, off); if (tid >= off) incl += q; }
        pre[tid + 1] = incl;
        if (tid == 0) pre[0] = 0;
    }
    __syncthreads();
    const int total = pre[NM_OUT_CHUNK_WORDS];
    if (total == 0) return;
    const int b = f / T;
    double zlo = 0.0, zlen = 0.0;
    if (depth) {                                                 // (float64 coordinates only: CT is double)
        zlo = (double)coord_of<CT>(z_idx_range[2 * b], half);
        zlen = (double)coord_of<CT>(z_idx_range[2 * b + 1], half) - zlo;
    }
    for (int r = tid; r < total; r += NM_OUT_BLOCK) {
        const long long row = base + r;
        if (row >= capacity) break;
        int wi = 0;
#pragma unroll
        for (int s = NM_OUT_CHUNK_WORDS / 2; s > 0; s >>= 1) wi += pre[wi + s] <= r ? s : 0;       // the last word with pre[wi] <= r
        const unsigned long long word = wsh[wi];
        int n = r - pre[wi], pos = 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const int below = __popcll((word >> pos) & ((1ull << s) - 1ull));
            if (n >= below) { n -= below; pos += s; }
        }
        const unsigned p = ((unsigned)c * NM_OUT_CHUNK_WORDS + (unsigned)wi) * 64u + (unsigned)pos;   // flat voxel of the frame, < G^3
        const unsigned ij = p / (unsigned)G;
        const int k = (int)(p - ij * (unsigned)G), i = (int)(ij / (unsigned)G), j = (int)(ij - (unsigned)i * (unsigned)G);
        if (idx) { int32_t* o = idx + row * 3; o[0] = i; o[1] = j; o[2] = k; }
        const CT ck = coord_of<CT>(k, half);
        if (coords) { CT* o = coords + row * 3; o[0] = coord_of<CT>(i, half); o[1] = coord_of<CT>(j, half); o[2] = ck; }
        if (depth) depth[row] = ((double)ck - zlo) / zlen;
    }
}

using OutGeom = NmOutGeom;
// NM_ERR_ARG / NM_ERR_UNSUPPORTED of the shapes, else the launch geometry
int out_geom(const char* who, int B, int T, int G, OutGeom* g) {
    if (B < 1 || T < 1 || G < 2) { nm_set_error("%s: B = %d clips, T = %d frames, G = %d", who, B, T, G); return NM_ERR_ARG; }
    const long long F = (long long)B * T;
    if (G > 1290 || F > ((1LL << 31) - 1) / ((long long)G * G * G)) {         // (1291^3 > 2^31: G^3 fits once G has passed)
        nm_set_error("%s: B * T * G^3 = %lld * %d^3 voxels, the call indexes fewer than 2^31", who, F, G);
        return NM_ERR_UNSUPPORTED;
    }
    g->F = (int)F; g->V = G * G * G; g->W = (g->V + 63) / 64; g->nC = (g->W + NM_OUT_CHUNK_WORDS - 1) / NM_OUT_CHUNK_WORDS;
    return NM_OK;
}

}  // namespace

// for nm_surface.hip (nm_output.h)
int nm_out_geom(const char* who, int B, int T, int G, NmOutGeom* g) { return out_geom(who, B, T, G, g); }
void nm_out_launch_chunk_scan(hipStream_t s, const unsigned long long* bits, const NmOutGeom& g, int32_t* coff) {
    hipLaunchKernelGGL(occ_chunk_scan_kernel, dim3((unsigned)g.F), dim3(NM_OUT_BLOCK), 0, s, bits, g.W, g.nC, coff);
}

extern "C" {

int nm_occupied_count(nm_ctx* c, const float* vox, int32_t B, int32_t T, int32_t G, int32_t mode, float thr, int32_t coord_f64,
                      uint64_t* bits, int64_t* offsets, int32_t* z_idx_range, void* z_range) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("occupied_count: null ctx"); return NM_ERR_ARG; }
    if (!vox || !bits || !offsets || !z_idx_range || !z_range) { nm_set_error("occupied_count: null argument"); return NM_ERR_ARG; }
    if (mode != NM_OCC_THRESHOLD && mode != NM_OCC_NONZERO) { nm_set_error("occupied_count: mode %d", (int)mode); return NM_ERR_ARG; }
    OutGeom g;
    int rc = out_geom("occupied_count", B, T, G, &g);
    if (rc) return rc;
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    const size_t nchunks = (size_t)g.F * g.nC, bytes = (3 * nchunks + 3 * (size_t)g.F) * sizeof(int32_t);
    if ((rc = nm_ctx_reserve(c, bytes + 4096))) return rc;               // (grows the workspace only the first time)
    c->ws.release(0);
    int32_t* scratch = static_cast<int32_t*>(c->ws.alloc_bytes(bytes));
    if (!scratch) { nm_set_error("occupied_count: workspace"); return NM_ERR_INTERNAL; }
    int32_t *ccnt = scratch, *czmin = ccnt + nchunks, *czmax = czmin + nchunks, *fstat = czmax + nchunks;
    hipStream_t s = c->stream;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(bits);
    if (mode == NM_OCC_THRESHOLD)
        hipLaunchKernelGGL(occ_mask_kernel<0>, dim3((unsigned)nchunks), dim3(NM_OUT_BLOCK), 0, s, vox, (int)G, g.V, g.W, g.nC, thr, words, ccnt, czmin, czmax);
    else
        hipLaunchKernelGGL(occ_mask_kernel<1>, dim3((unsigned)nchunks), dim3(NM_OUT_BLOCK), 0, s, vox, (int)G, g.V, g.W, g.nC, thr, words, ccnt, czmin, czmax);
    hipLaunchKernelGGL(occ_frame_kernel, dim3((unsigned)g.F), dim3(NM_OUT_BLOCK), 0, s, (const int32_t*)ccnt, (const int32_t*)czmin,
                       (const int32_t*)czmax, g.nC, fstat);
    const double half = (double)(G - 1) / 2.0;
    if (coord_f64)
        hipLaunchKernelGGL(occ_offsets_kernel<double>, dim3(1), dim3(NM_OUT_BLOCK), 0, s, (const int32_t*)fstat, (int)B, (int)T, half,
                           reinterpret_cast<long long*>(offsets), z_idx_range, static_cast<double*>(z_range));
    else
        hipLaunchKernelGGL(occ_offsets_kernel<float>, dim3(1), dim3(NM_OUT_BLOCK), 0, s, (const int32_t*)fstat, (int)B, (int)T, (float)half,
                           reinterpret_cast<long long*>(offsets), z_idx_range, static_cast<float*>(z_range));
    return nm_check_hip(hipGetLastError(), "occupied_count launch");
} catch (...) { return nm_abi_catch("nm_occupied_count"); }

int nm_occupied_write(nm_ctx* c, const uint64_t* bits, const int64_t* offsets, const int32_t* z_idx_range, int32_t B, int32_t T, int32_t G,
                      int32_t coord_f64, int64_t capacity, int32_t* idx, void* coords, double* depth) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("occupied_write: null ctx"); return NM_ERR_ARG; }
    if (!bits || !offsets || !z_idx_range) { nm_set_error("occupied_write: null argument"); return NM_ERR_ARG; }
    if (depth && !coord_f64) { nm_set_error("occupied_write: depth is float64 arithmetic, coord_f64 = 0"); return NM_ERR_ARG; }
    if (capacity < 0) { nm_set_error("occupied_write: capacity %lld", (long long)capacity); return NM_ERR_ARG; }
    OutGeom g;
    int rc = out_geom("occupied_write", B, T, G, &g);
    if (rc) return rc;
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    if (capacity == 0 || (!idx && !coords && !depth)) return NM_OK;       // nothing to write
    const size_t nchunks = (size_t)g.F * g.nC, bytes = nchunks * sizeof(int32_t);
    if ((rc = nm_ctx_reserve(c, bytes + 4096))) return rc;
    c->ws.release(0);
    int32_t* coff = static_cast<int32_t*>(c->ws.alloc_bytes(bytes));
    if (!coff) { nm_set_error("occupied_write: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(bits);
    const long long* offs = reinterpret_cast<const long long*>(offsets);
    hipLaunchKernelGGL(occ_chunk_scan_kernel, dim3((unsigned)g.F), dim3(NM_OUT_BLOCK), 0, s, words, g.W, g.nC, coff);
    const double half = (double)(G - 1) / 2.0;
    if (coord_f64)
        hipLaunchKernelGGL(occ_write_kernel<double>, dim3((unsigned)nchunks), dim3(NM_OUT_BLOCK), 0, s, words, offs, (const int32_t*)coff, z_idx_range,
                           (int)T, (int)G, g.W, g.nC, half, (long long)capacity, idx, static_cast<double*>(coords), depth);
    else
        hipLaunchKernelGGL(occ_write_kernel<float>, dim3((unsigned)nchunks), dim3(NM_OUT_BLOCK), 0, s, words, offs, (const int32_t*)coff, z_idx_range,
                           (int)T, (int)G, g.W, g.nC, (float)half, (long long)capacity, idx, static_cast<float*>(coords), (double*)nullptr);
    return nm_check_hip(hipGetLastError(), "occupied_write launch");
} catch (...) { return nm_abi_catch("nm_occupied_write"); }

}  // extern "C"
