// Mesh surface sampling: mesh sequences to the (frames, count, 3) point arrays the input path reads - what the reference's offline
// preparation computed on the host with trimesh.sample.sample_surface(mesh, 20000) and mesh.face_normals once per frame
// (dataset/dfaust/write_sequence_to_obj.py:20-23, :107-115, dataset/aistpp/prepare_aistpp.py:13-16, :75-83) - for T frames in one
// stream-ordered call.  The contract is include/nm355.h's; tests/sample_ref.py restates it in numpy.
//
// trimesh picks a face by searching a float64 cumulative sum of the areas, whose bits depend on the order of the additions.  Here the
// areas of a frame become integers below 2^32, scaled by the power of two above the frame's largest area: a maximum and an integer sum
// do not depend on their order, so every scan gives the same table and every pick the same face.  Three passes:
//   faces   sample_faces_kernel: a lane per (frame, face): area (float64) and unit normal (float32) into the scratch, the frame's
//           largest finite area by a wave reduction and one atomic maximum per wavefront on the bit pattern (non-negative doubles order
//           like their bit patterns), the rows of `triangles` with an index outside the vertices counted once.
//   scan    sample_scan_kernel: weights from the areas and the frame's maximum, their inclusive scan, and every 64th entry of it into
//           the coarse table.  The weights are never stored: a frame past NM_SAMPLE_SCAN_ONE faces computes them twice (chunk sums,
//           then the chunks), 8 bytes read again instead of 8 written and 8 read.
//   draw    sample_draw_kernel: a lane per (frame, sample): the uniforms (Philox4x32-10 or the caller's), the pick by binary search of
//           the coarse table - in LDS while it fits - and of one 64-entry segment of the scan, the point from the face's three vertices.
// Arithmetic: float64, every operation rounded on its own (the library is built with -ffp-contract=off).
#include "nm_ctx.h"
#include "nm_sample.h"
#include <cmath>

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    for (int off = 32; off > 0; off >>= 1) { const u64 q = __shfl_xor(v, off); v = q > v ? q : v; }
    return v;
}
// inclusive scan of v over the wavefront
__device__ __forceinline__ u64 wave_inclusive_u64(u64 v, int lane) {
    for (int off = 1; off < 64; off <<= 1) { const u64 q = __shfl_up(v, off); if (lane >= off) v += q; }
    return v;
}

// ---- faces -----------------------------------------------------------------------------------------------------------------------
// grid T * nFB: workgroup t * nFB + b takes faces [256 b, 256 b + 256) of frame t
template <typename VT, typename IT>
__global__ __launch_bounds__(NM_SAMPLE_BLOCK) void sample_faces_kernel(const VT* __restrict__ vert, const IT* __restrict__ tri, int V, int F, int nFB,
                                                                        double* __restrict__ area, float* __restrict__ nrm,
                                                                        u64* __restrict__ amax, int32_t* __restrict__ counters) {
    const int t = blockIdx.x / nFB, i = (blockIdx.x - t * nFB) * NM_SAMPLE_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    double ar = 0.0;
    float n[3] = {0.0f, 0.0f, 0.0f};
    bool bad = false;
    if (i < F) {
        const long long i0 = (long long)tri[3 * (size_t)i], i1 = (long long)tri[3 * (size_t)i + 1], i2 = (long long)tri[3 * (size_t)i + 2];
        bad = i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V;
        if (!bad) {
            const VT* fv = vert + (size_t)t * (size_t)V * 3;
            const VT *p0 = fv + 3 * i0, *p1 = fv + 3 * i1, *p2 = fv + 3 * i2;
            const double ox = (double)p0[0], oy = (double)p0[1], oz = (double)p0[2];
            const double ax = (double)p1[0] - ox, ay = (double)p1[1] - oy, az = (double)p1[2] - oz;
            const double bx = (double)p2[0] - ox, by = (double)p2[1] - oy, bz = (double)p2[2] - oz;
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const double n2 = (cx * cx + cy * cy) + cz * cz;
            const double r = sqrt(n2);
            ar = 0.5 * r;
            if (n2 != 0.0 && isfinite(n2)) { n[0] = (float)(cx / r); n[1] = (float)(cy / r); n[2] = (float)(cz / r); }
        }
        const size_t row = (size_t)t * (size_t)F + (size_t)i;
        area[row] = ar;
        nrm[3 * row] = n[0]; nrm[3 * row + 1] = n[1]; nrm[3 * row + 2] = n[2];
    }
    // (an area is +0, positive, +inf or NaN: n2 is a sum of squares)
    const u64 mine = isfinite(ar) ? (u64)__double_as_longlong(ar) : 0ull;
    const u64 top = wave_max_u64(mine);
    if (lane == 0 && top != 0ull) atomicMax(amax + t, top);
    if (t == 0) {                                                 // (the same for the whole workgroup)
        const int nbad = __popcll(__ballot(bad));
        if (lane == 0 && nbad) atomicAdd(counters, nbad);
    }
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------
// the shift 32 - e of a frame whose largest finite area has the bit pattern `bits`
__device__ __forceinline__ int weight_shift(u64 bits) {
    int e = 0;
    (void)frexp(__longlong_as_double((long long)bits), &e);      // (0 for amax = 0)
    return 32 - e;
}
__device__ __forceinline__ u64 weight_of(double a, int shift) {
    return isfinite(a) ? (u64)floor(ldexp(a, shift)) : 0ull;       // a <= amax < 2^e: below 2^32
}

// grid T * nK: sums[t * nK + k] = the weights of faces [k chunk, k chunk + chunk) of frame t
__global__ __launch_bounds__(NM_SAMPLE_BLOCK) void sample_chunk_sums_kernel(const double* __restrict__ area, const u64* __restrict__ amax, int F, int nK,
                                                                             int chunk, u64* __restrict__ sums) {
    __shared__ u64 sh[NM_SAMPLE_BLOCK / 64];
    const int t = blockIdx.x / nK, k = blockIdx.x - t * nK, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = k * chunk, hi = min(F, lo + chunk), shift = weight_shift(amax[t]);
    const double* fa = area + (size_t)t * (size_t)F;
    u64 s = 0;
    for (int i = lo + tid; i < hi; i += NM_SAMPLE_BLOCK) s += weight_of(fa[i], shift);
    s = wave_inclusive_u64(s, lane);
    if (lane == 63) sh[wave] = s;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// grid T, one workgroup: the exclusive scan of a frame's nK <= 2 * NM_SAMPLE_BLOCK chunk sums, in place
__global__ __launch_bounds__(NM_SAMPLE_BLOCK) void sample_chunk_offsets_kernel(u64* __restrict__ sums, int nK) {
    __shared__ u64 sh[NM_SAMPLE_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64* fs = sums + (size_t)blockIdx.x * (size_t)nK;
    const int k0 = 2 * tid;
    const u64 a = k0 < nK ? fs[k0] : 0ull, b = k0 + 1 < nK ? fs[k0 + 1] : 0ull;
    const u64 incl = wave_inclusive_u64(a + b, lane);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    u64 ex = incl - (a + b);
    for (int v = 0; v < wave; ++v) ex += sh[v];
    if (k0 < nK) fs[k0] = ex;
    if (k0 + 1 < nK) fs[k0 + 1] = ex + a;
}

// grid T * nK: workgroup t * nK + k scans faces [k chunk, k chunk + chunk) of frame t, NM_SAMPLE_SCAN_STEP per step, starting from
// offs[t * nK + k] (offs NULL: one chunk per frame, from 0).  Writes cum, the coarse table entries that fall into its range -
// coarse[j] = cum[min(64 j + 63, F - 1)] - and counts the frame as empty if its last entry is 0.
__global__ __launch_bounds__(NM_SAMPLE_BLOCK) void sample_scan_kernel(const double* __restrict__ area, const u64* __restrict__ amax,
                                                                       const u64* __restrict__ offs, int F, int nK, int chunk, int nC,
                                                                       u64* __restrict__ cum, u64* __restrict__ coarse, int32_t* __restrict__ counters) {
    __shared__ u64 sh[NM_SAMPLE_BLOCK / 64];
    const int t = blockIdx.x / nK, k = blockIdx.x - t * nK, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = k * chunk, hi = min(F, lo + chunk), shift = weight_shift(amax[t]);
    const double* fa = area + (size_t)t * (size_t)F;
    u64* fc = cum + (size_t)t * (size_t)F;
    u64* fco = coarse + (size_t)t * (size_t)nC;
    u64 carry = offs ? offs[blockIdx.x] : 0ull;
    for (int base = lo; base < hi; base += NM_SAMPLE_SCAN_STEP) {
        const int i0 = base + NM_SAMPLE_SCAN_ITEMS * tid;
        u64 w[NM_SAMPLE_SCAN_ITEMS], s = 0;
#pragma unroll
        for (int j = 0; j < NM_SAMPLE_SCAN_ITEMS; ++j) {
            s += i0 + j < hi ? weight_of(fa[i0 + j], shift) : 0ull;
            w[j] = s;                                              // inclusive inside the thread
        }
        const u64 incl = wave_inclusive_u64(s, lane);
        if (lane == 63) sh[wave] = incl;
        __syncthreads();
        u64 ex = carry + (incl - s);
        for (int v = 0; v < wave; ++v) ex += sh[v];
        carry += (sh[0] + sh[1]) + (sh[2] + sh[3]);
#pragma unroll
        for (int j = 0; j < NM_SAMPLE_SCAN_ITEMS; ++j) {
            const int i = i0 + j;
            if (i < hi) {
                const u64 c = ex + w[j];
                fc[i] = c;
                if ((i & (NM_SAMPLE_SEG - 1)) == NM_SAMPLE_SEG - 1 || i == F - 1) fco[i / NM_SAMPLE_SEG] = c;
                if (i == F - 1 && c == 0ull) atomicAdd(counters + 1, 1);
            }
        }
        __syncthreads();                                           // sh is rewritten by the next step
    }
}

// ---- draw ------------------------------------------------------------------------------------------------------------------------
// the smallest j in [0, n) with tab[j] > p; the caller knows tab[n - 1] > p
template <typename P> __device__ __forceinline__ int first_above(P tab, int n, u64 p) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// grid T * nB: workgroup t * nB + b draws samples [1024 b, 1024 b + 1024) of frame t, thread r its samples 1024 b + 256 j + r
template <typename VT, typename IT>
__global__ __launch_bounds__(NM_SAMPLE_BLOCK) void sample_draw_kernel(const VT* __restrict__ vert, const IT* __restrict__ tri, const u64* __restrict__ cum,
                                                                       const u64* __restrict__ coarse, const float* __restrict__ nrm,
                                                                       const double* __restrict__ u, u64 seed, int V, int F, int nC, long long count,
                                                                       int nB, float* __restrict__ points, float* __restrict__ normals,
                                                                       int32_t* __restrict__ face_index, double* __restrict__ uout) {
    __shared__ u64 shc[NM_SAMPLE_LDS_COARSE];
    const int t = blockIdx.x / nB, b = blockIdx.x - t * nB, tid = threadIdx.x;
    const u64* fc = cum + (size_t)t * (size_t)F;
    const u64* fco = coarse + (size_t)t * (size_t)nC;
    const float* fn = nrm + 3 * (size_t)t * (size_t)F;
    const VT* fv = vert + (size_t)t * (size_t)V * 3;
    const bool staged = nC <= NM_SAMPLE_LDS_COARSE;               // (the same for the whole launch)
    if (staged) {
        for (int j = tid; j < nC; j += NM_SAMPLE_BLOCK) shc[j] = fco[j];
        __syncthreads();
    }
    const u64 W = fc[F - 1];
#pragma unroll 1
    for (int j = 0; j < NM_SAMPLE_DRAW_ITEMS; ++j) {
        const long long s = (long long)b * NM_SAMPLE_DRAW_PER_BLOCK + j * NM_SAMPLE_BLOCK + tid;
        if (s >= count) break;
        const size_t row = (size_t)t * (size_t)count + (size_t)s;
        double uu[3];
        if (u) { uu[0] = u[3 * row]; uu[1] = u[3 * row + 1]; uu[2] = u[3 * row + 2]; }
        else nm_sample_uniforms(seed, (uint64_t)s, (uint32_t)t, uu);
        if (uout) { uout[3 * row] = uu[0]; uout[3 * row + 1] = uu[1]; uout[3 * row + 2] = uu[2]; }
        int face = 0;
        if (W != 0ull) {
            const double x = uu[0] * (double)W;
            const u64 p = !(x >= 0.0) ? 0ull : (x >= (double)W ? W - 1ull : (u64)x);     // floor of a non-negative number; W - 1 caps it
            const int seg = staged ? first_above(shc, nC, p) : first_above(fco, nC, p);
            const int base = seg * NM_SAMPLE_SEG;
            face = base + first_above(fc + base, min(NM_SAMPLE_SEG, F - base), p);
        }
        const long long i0 = (long long)tri[3 * (size_t)face], i1 = (long long)tri[3 * (size_t)face + 1], i2 = (long long)tri[3 * (size_t)face + 2];
        double pt[3] = {0.0, 0.0, 0.0};
        float n[3] = {0.0f, 0.0f, 0.0f};
        if (W == 0ull) {                                           // a frame without surface: v0 of face 0
            if (i0 >= 0 && i0 < V) { pt[0] = (double)fv[3 * i0]; pt[1] = (double)fv[3 * i0 + 1]; pt[2] = (double)fv[3 * i0 + 2]; }
        } else if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {        // (a picked face has weight: its indices were in range)
            double u1 = uu[1], u2 = uu[2];
            if (u1 + u2 > 1.0) { u1 = fabs(u1 - 1.0); u2 = fabs(u2 - 1.0); }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double o = (double)fv[3 * i0 + d];
                const double a = (double)fv[3 * i1 + d] - o, bb = (double)fv[3 * i2 + d] - o;
                pt[d] = o + (a * u1 + bb * u2);
            }
            n[0] = fn[3 * (size_t)face]; n[1] = fn[3 * (size_t)face + 1]; n[2] = fn[3 * (size_t)face + 2];
        }
        points[3 * row] = (float)pt[0]; points[3 * row + 1] = (float)pt[1]; points[3 * row + 2] = (float)pt[2];
        normals[3 * row] = n[0]; normals[3 * row + 1] = n[1]; normals[3 * row + 2] = n[2];
        face_index[row] = face;
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// where the tables lie in the caller's scratch (bytes from its start)
struct SampleLayout {
    int nC = 0, nK = 0, chunk = 0;
    size_t area = 0, cum = 0, nrm = 0, coarse = 0, sums = 0, amax = 0, total = 0;
};
bool sample_layout(int T, int F, SampleLayout* L) {
    if (T < 1 || F < 1 || F > NM_SAMPLE_MAX_FACES) return false;
    const size_t rows = (size_t)T * (size_t)F;
    L->nC = (F + NM_SAMPLE_SEG - 1) / NM_SAMPLE_SEG;
    L->chunk = F <= NM_SAMPLE_SCAN_ONE ? F : NM_SAMPLE_SCAN_CHUNK;
    L->nK = (F + L->chunk - 1) / L->chunk;
    size_t at = 0;
    L->area = at; at = align256(at + rows * sizeof(double));
    L->cum = at; at = align256(at + rows * sizeof(u64));
    L->nrm = at; at = align256(at + rows * 3 * sizeof(float));
    L->coarse = at; at = align256(at + (size_t)T * L->nC * sizeof(u64));
    L->sums = at; at = align256(at + (size_t)T * L->nK * sizeof(u64));
    L->amax = at; at = align256(at + (size_t)T * sizeof(u64));
    L->total = at;
    return true;
}

template <typename VT, typename IT>
void sample_launch(hipStream_t s, const SampleLayout& L, char* scratch, const void* vertices, const void* triangles, int T, int V, int F, long long count,
                   u64 seed, const double* u, float* points, float* normals, int32_t* face_index, double* uout, int32_t* counters) {
    double* area = reinterpret_cast<double*>(scratch + L.area);
    u64* cum = reinterpret_cast<u64*>(scratch + L.cum);
    float* nrm = reinterpret_cast<float*>(scratch + L.nrm);
    u64* coarse = reinterpret_cast<u64*>(scratch + L.coarse);
    u64* sums = reinterpret_cast<u64*>(scratch + L.sums);
    u64* amax = reinterpret_cast<u64*>(scratch + L.amax);
    const VT* vert = static_cast<const VT*>(vertices);
    const IT* tri = static_cast<const IT*>(triangles);
    const int nFB = (F + NM_SAMPLE_BLOCK - 1) / NM_SAMPLE_BLOCK;
    const int nB = (int)((count + NM_SAMPLE_DRAW_PER_BLOCK - 1) / NM_SAMPLE_DRAW_PER_BLOCK);
    hipLaunchKernelGGL((sample_faces_kernel<VT, IT>), dim3((unsigned)T * (unsigned)nFB), dim3(NM_SAMPLE_BLOCK), 0, s, vert, tri, V, F, nFB, area, nrm, amax, counters);
    const unsigned nchunks = (unsigned)T * (unsigned)L.nK;
    if (L.nK > 1) {
        hipLaunchKernelGGL(sample_chunk_sums_kernel, dim3(nchunks), dim3(NM_SAMPLE_BLOCK), 0, s, (const double*)area, (const u64*)amax, F, L.nK, L.chunk, sums);
        hipLaunchKernelGGL(sample_chunk_offsets_kernel, dim3((unsigned)T), dim3(NM_SAMPLE_BLOCK), 0, s, sums, L.nK);
    }
    hipLaunchKernelGGL(sample_scan_kernel, dim3(nchunks), dim3(NM_SAMPLE_BLOCK), 0, s, (const double*)area, (const u64*)amax,
                       L.nK > 1 ? (const u64*)sums : (const u64*)nullptr, F, L.nK, L.chunk, L.nC, cum, coarse, counters);
    hipLaunchKernelGGL((sample_draw_kernel<VT, IT>), dim3((unsigned)T * (unsigned)nB), dim3(NM_SAMPLE_BLOCK), 0, s, vert, tri, (const u64*)cum, (const u64*)coarse,
                       (const float*)nrm, u, seed, V, F, L.nC, count, nB, points, normals, face_index, uout);
}

}  // namespace

extern "C" {

size_t nm_sample_surface_workspace(int32_t T, int32_t F) try {
    SampleLayout L;
    return sample_layout(T, F, &L) ? L.total : 0;
} catch (...) { (void)nm_abi_catch("nm_sample_surface_workspace"); return 0; }

int nm_sample_surface(nm_ctx* c, const void* vertices, int32_t vertices_f64, const void* triangles, int32_t triangles_i64, int32_t T, int32_t V,
                      int32_t F, int64_t count, uint64_t seed, const double* u, void* scratch, size_t scratch_bytes, float* points, float* normals,
                      int32_t* face_index, double* uniforms_out, int32_t* counters) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("sample_surface: null ctx"); return NM_ERR_ARG; }
    if (!vertices || !triangles || !scratch || !points || !normals || !face_index || !counters) { nm_set_error("sample_surface: null argument"); return NM_ERR_ARG; }
    if (T < 1 || V < 1 || F < 1 || count < 1) {
        nm_set_error("sample_surface: T = %d frames, V = %d vertices, F = %d faces, count = %lld", (int)T, (int)V, (int)F, (long long)count);
        return NM_ERR_ARG;
    }
    if (F > NM_SAMPLE_MAX_FACES) { nm_set_error("sample_surface: F = %d faces, at most 2^21 (the frame's integer weights sum below 2^53)", (int)F); return NM_ERR_ARG; }
    SampleLayout L;
    if (!sample_layout(T, F, &L)) { nm_set_error("sample_surface: T = %d, F = %d", (int)T, (int)F); return NM_ERR_ARG; }
    if (scratch_bytes < L.total) { nm_set_error("sample_surface: scratch of %zu bytes, nm_sample_surface_workspace asks for %zu", scratch_bytes, L.total); return NM_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(scratch) & 255) { nm_set_error("sample_surface: scratch is not 256-byte aligned"); return NM_ERR_ARG; }
    const long long lim = (1LL << 31) - 1;
    const long long nFB = (F + NM_SAMPLE_BLOCK - 1) / NM_SAMPLE_BLOCK;
    if (count >= lim - NM_SAMPLE_DRAW_PER_BLOCK || (long long)T * ((count + NM_SAMPLE_DRAW_PER_BLOCK - 1) / NM_SAMPLE_DRAW_PER_BLOCK) > lim || (long long)T * nFB > lim) {
        nm_set_error("sample_surface: T = %d frames of %d faces and %lld samples, one call launches fewer than 2^31 workgroups per pass", (int)T, (int)F, (long long)count);
        return NM_ERR_UNSUPPORTED;
    }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    hipStream_t s = c->stream;
    char* base = static_cast<char*>(scratch);
    if ((rc = nm_check_hip(hipMemsetAsync(base + L.amax, 0, (size_t)T * sizeof(u64), s), "sample_surface memset"))) return rc;
    if ((rc = nm_check_hip(hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s), "sample_surface memset"))) return rc;
    const u64 sd = (u64)seed;
    if (vertices_f64) {
        if (triangles_i64) sample_launch<double, long long>(s, L, base, vertices, triangles, T, V, F, count, sd, u, points, normals, face_index, uniforms_out, counters);
        else sample_launch<double, int32_t>(s, L, base, vertices, triangles, T, V, F, count, sd, u, points, normals, face_index, uniforms_out, counters);
    } else {
        if (triangles_i64) sample_launch<float, long long>(s, L, base, vertices, triangles, T, V, F, count, sd, u, points, normals, face_index, uniforms_out, counters);
        else sample_launch<float, int32_t>(s, L, base, vertices, triangles, T, V, F, count, sd, u, points, normals, face_index, uniforms_out, counters);
    }
    return nm_check_hip(hipGetLastError(), "sample_surface launch");
} catch (...) { return nm_abi_catch("nm_sample_surface"); }

int nm_sample_tables(nm_ctx* c, const void* scratch, int32_t T, int32_t F, double* areas, int64_t* cum) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("sample_tables: null ctx"); return NM_ERR_ARG; }
    SampleLayout L;
    if (!scratch || !sample_layout(T, F, &L)) { nm_set_error("sample_tables: null scratch, or T = %d, F = %d", (int)T, (int)F); return NM_ERR_ARG; }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    const char* base = static_cast<const char*>(scratch);
    const size_t bytes = (size_t)T * (size_t)F * 8;
    if (areas && (rc = nm_check_hip(hipMemcpyAsync(areas, base + L.area, bytes, hipMemcpyDeviceToDevice, c->stream), "sample_tables copy"))) return rc;
    if (cum && (rc = nm_check_hip(hipMemcpyAsync(cum, base + L.cum, bytes, hipMemcpyDeviceToDevice, c->stream), "sample_tables copy"))) return rc;
    return NM_OK;
} catch (...) { return nm_abi_catch("nm_sample_tables"); }

}  // extern "C"
