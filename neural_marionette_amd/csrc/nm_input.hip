// Device input path for batches: what the reference's dataset classes do per clip in numpy between np.load and the network -
// crop_sequence, episodic_normalization (with its translation and its joints) and voxelize (utils/dataset_utils.py:6-31 as called
// from dataset/dataset.py:47-88, :123-183 and vis_generation.py:14-25) - for B crops of device-resident sequences in one
// stream-ordered call.
//
// Arithmetic.  The indices are a floor of a quotient, so they are reproduced only by the reference's own roundings, and those depend
// on the dtype of the data (numpy 2 promotion: a Python float never widens an array):
//   float32 points:  blen = max_d f32(bmax_d - bmin_d), den = f32(blen + f32(1e-5)),
//                    v = f32(p - bmin_d), v = f32(v * f32(scale)), v = f32(v / den), v = f32(v * 2), v = f32(v - 1)
//                    and only then float64: w = double(v) + t_d, w = w - (-1.0), w = w / (2.0 / G + 1e-5), idx = (int32)w
//   float64 points:  the same chain in float64 throughout (what nm_voxelize_clip evaluates with t = 0).
// t = (x_trans, 0, z_trans).  The library is built with -ffp-contract=off and the fp32 division is the correctly rounded one.
// The joints follow episodic_normalization's second expression, ((j - bmin) * scale / den) * 2 - 1, in numpy's result type of
// (joints dtype, points dtype): float32 only when both are, else float64 with bmin and den widened from the points' dtype.
//
// Indices.  numpy indexing wraps [-G, -1] to idx + G, and so does the scatter here.  A row with an index outside [-G, G) or a
// non-finite coordinate makes the reference raise; here it writes nothing and is counted in bad_rows[b].
//
// The descriptor table lives in device memory and the entry point reads nothing back, so a descriptor's own consistency (start,
// sample_rate, frames) is the caller's to check before the call (NeuralMarionette.voxelize_batch does).  The kernels are safe
// whatever it holds: a frame index is never read past frames - 1, and a clip whose crop does not fit without `pad` writes nothing
// and counts every one of its rows as bad.
#include "nm_ctx.h"
#include "nm_input.h"
#include <algorithm>

namespace {

__device__ __forceinline__ bool clip_fits(const nm_clip_desc& d, int T) {
    if (d.frames < 1 || d.start < 0 || d.sample_rate < 1 || !d.points) return false;
    return d.pad != 0 || (long long)d.start + (long long)(T - 1) * d.sample_rate < (long long)d.frames;
}
// frame t of the crop: start + t * sample_rate, the last frame repeated where the reference pads (dataset.py:65-68)
__device__ __forceinline__ size_t clip_frame(const nm_clip_desc& d, int t) {
    const long long f = (long long)d.start + (long long)t * d.sample_rate;
    return (size_t)(f < (long long)d.frames ? f : (long long)d.frames - 1);
}

// numpy's amin / amax: a NaN wins, whatever the order (v != v picks it up, and nothing compares below or above it afterwards)
template <typename PT> __device__ __forceinline__ PT in_min(PT a, PT v) { return (v < a || v != v) ? v : a; }
template <typename PT> __device__ __forceinline__ PT in_max(PT a, PT v) { return (v > a || v != v) ? v : a; }
template <typename PT> __device__ __forceinline__ PT in_inf();
template <> __device__ __forceinline__ float in_inf<float>() { return __int_as_float(0x7f800000); }
template <> __device__ __forceinline__ double in_inf<double>() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---- box -------------------------------------------------------------------------------------------------------------------------
// grid (parts, B): per-axis min / max over the T cropped frames x N points of clip b in the source dtype (exact in any order; a NaN
// coordinate makes the box, and with it every row of the clip, NaN as in numpy);
// workgroup p takes the points p * 256 + tid, stride parts * 256, of every frame.  part (B, parts, 6) = min xyz, max xyz.
template <typename PT>
__global__ __launch_bounds__(NM_IN_BLOCK) void clip_bbox_kernel(const nm_clip_desc* __restrict__ clips, int T, long long N, PT* __restrict__ part) {
    __shared__ PT sh[NM_IN_BLOCK * 6];
    const int b = blockIdx.y, tid = threadIdx.x;
    const nm_clip_desc d = clips[b];
    PT mn[3] = {in_inf<PT>(), in_inf<PT>(), in_inf<PT>()}, mx[3] = {-in_inf<PT>(), -in_inf<PT>(), -in_inf<PT>()};
    if (clip_fits(d, T)) {
        const PT* pts = static_cast<const PT*>(d.points);
        for (int t = 0; t < T; ++t) {
            const PT* fr = pts + clip_frame(d, t) * (size_t)N * 3;
            for (long long n = (long long)blockIdx.x * NM_IN_BLOCK + tid; n < N; n += (long long)gridDim.x * NM_IN_BLOCK)
                for (int k = 0; k < 3; ++k) { const PT v = fr[n * 3 + k]; mn[k] = in_min(mn[k], v); mx[k] = in_max(mx[k], v); }
        }
    }
    for (int k = 0; k < 3; ++k) { sh[tid * 6 + k] = mn[k]; sh[tid * 6 + 3 + k] = mx[k]; }
    __syncthreads();
    for (int st = NM_IN_BLOCK / 2; st > 0; st >>= 1) {
        if (tid < st)
            for (int k = 0; k < 3; ++k) {
                sh[tid * 6 + k] = in_min(sh[tid * 6 + k], sh[(tid + st) * 6 + k]);
                sh[tid * 6 + 3 + k] = in_max(sh[tid * 6 + 3 + k], sh[(tid + st) * 6 + 3 + k]);
            }
        __syncthreads();
    }
    if (tid < 6) part[((size_t)b * gridDim.x + blockIdx.x) * 6 + tid] = sh[tid];
}

// the clip's box from its partials into bb[6], then one barrier: lane j of the first wave holds partial j (nparts <= 64), six xor
// butterflies over the wave (min / max are exact in any order)
template <typename PT>
__device__ __forceinline__ void finish_box(const PT* __restrict__ part, int nparts, int b, PT* bb) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        const PT* p = part + ((size_t)b * nparts + (tid < nparts ? tid : 0)) * 6;      // (lanes past the last partial repeat partial 0)
        PT v[6];
        for (int k = 0; k < 6; ++k) v[k] = p[k];
        for (int off = 32; off > 0; off >>= 1)
            for (int k = 0; k < 6; ++k) { const PT q = __shfl_xor(v[k], off); v[k] = k < 3 ? in_min(v[k], q) : in_max(v[k], q); }
        if (tid == 0) for (int k = 0; k < 6; ++k) bb[k] = v[k];
    }
    __syncthreads();
}
template <typename PT> __device__ __forceinline__ PT box_den(const PT* bb) {
    const PT e0 = bb[3] - bb[0], e1 = bb[4] - bb[1], e2 = bb[5] - bb[2];
    return in_max(in_max(e0, e1), e2) + (PT)1e-5;
}

// ---- normalise + voxelise --------------------------------------------------------------------------------------------------------
// grid (T * tiles, B): workgroup x = t * tiles + tile takes the points tile * 256 + tid, stride tiles * 256, of frame t.
template <typename PT>
__global__ __launch_bounds__(NM_IN_BLOCK) void voxelize_batch_kernel(const nm_clip_desc* __restrict__ clips, int T, long long N, int G, int tiles,
                                                                    const PT* __restrict__ part, int nparts, float* __restrict__ vox,
                                                                    int32_t* __restrict__ idx_out, double* __restrict__ bbox_out,
                                                                    int32_t* __restrict__ bad_rows) {
    __shared__ PT bb[6];
    const int b = blockIdx.y, tid = threadIdx.x;
    const nm_clip_desc d = clips[b];
    const int t = blockIdx.x / tiles, tile = blockIdx.x - t * tiles;
    finish_box(part, nparts, b, bb);
    if (bbox_out && blockIdx.x == 0 && tid < 6) bbox_out[(size_t)b * 6 + tid] = (double)bb[tid];
    int bad = 0;
    if (!clip_fits(d, T)) {
        for (long long n = (long long)tile * NM_IN_BLOCK + tid; n < N; n += (long long)tiles * NM_IN_BLOCK) {
            ++bad;
            if (idx_out) { int32_t* o = idx_out + (((size_t)b * T + t) * (size_t)N + n) * 3; o[0] = o[1] = o[2] = 0; }
        }
    } else {
        const PT den = box_den(bb), sc = (PT)d.scale;
        const double tr[3] = {d.x_trans, 0.0, d.z_trans};
        const double step = 2.0 / (double)G + 1e-5;
        const PT* fr = static_cast<const PT*>(d.points) + clip_frame(d, t) * (size_t)N * 3;
        float* grid = vox + ((size_t)b * T + t) * ((size_t)G * G * G);
        for (long long n = (long long)tile * NM_IN_BLOCK + tid; n < N; n += (long long)tiles * NM_IN_BLOCK) {
            int id[3];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                PT v = fr[n * 3 + k] - bb[k];
                v = v * sc; v = v / den; v = v * (PT)2; v = v - (PT)1;
                double w = (double)v + tr[k];          // the reference adds the float64 translation vector: float64 from here on
                w = w - (-1.0);
                w = w / step;
                const bool fits = w > -2147483648.0 && w < 2147483648.0;       // (a NaN fails both comparisons)
                id[k] = fits ? (int)w : 0;             // astype(np.int32): truncation toward zero; 0 where int32 cannot hold it
                ok = ok && fits && id[k] >= -G && id[k] < G;
            }
            if (idx_out) {                             // the indices as computed, before the wrap
                int32_t* o = idx_out + (((size_t)b * T + t) * (size_t)N + n) * 3;
                o[0] = id[0]; o[1] = id[1]; o[2] = id[2];
            }
            if (ok) {
#pragma unroll
                for (int k = 0; k < 3; ++k) id[k] += id[k] < 0 ? G : 0;         // numpy's negative indices
                grid[((size_t)id[0] * G + id[1]) * G + id[2]] = 1.0f;           // idempotent set: no atomics needed
            } else ++bad;
        }
    }
    for (int off = 32; off > 0; off >>= 1) bad += nm_sx(bad, off);
    if ((tid & 63) == 0 && bad) atomicAdd(bad_rows + b, bad);
}

// ---- joints ----------------------------------------------------------------------------------------------------------------------
// grid (x, B): the T x J x 3 joint coordinates of clip b's crop, an element per thread (grid-stride).
template <typename PT, typename JT, typename RT>
__global__ __launch_bounds__(NM_IN_BLOCK) void joints_norm_kernel(const nm_clip_desc* __restrict__ clips, int T, int J, const PT* __restrict__ part,
                                                                 int nparts, RT* __restrict__ out) {
    __shared__ PT bb[6];
    const int b = blockIdx.y;
    const nm_clip_desc d = clips[b];
    finish_box(part, nparts, b, bb);
    const bool fits = clip_fits(d, T) && d.joints;
    const RT den = (RT)box_den(bb), sc = (RT)d.scale;
    const int per = J * 3, total = T * per;
    for (int e = blockIdx.x * NM_IN_BLOCK + threadIdx.x; e < total; e += gridDim.x * NM_IN_BLOCK) {
        RT v = (RT)0;
        if (fits) {
            const int t = e / per, r = e - t * per;
            v = (RT)static_cast<const JT*>(d.joints)[clip_frame(d, t) * (size_t)per + r] - (RT)bb[r % 3];
            v = v * sc; v = v / den; v = v * (RT)2; v = v - (RT)1;
        }
        out[(size_t)b * total + e] = v;
    }
}

template <typename PT>
int launch_batch(nm_ctx* c, const nm_clip_desc* clips, int B, int T, long long N, int J, int joints_f64, float* vox, void* joints_out,
                 int32_t* idx_out, double* bbox_out, int32_t* bad_rows, void* part_ws) {
    const int G = c->cfg.grid_size;
    const long long ntiles = (N + NM_IN_BLOCK - 1) / NM_IN_BLOCK;
    const int nparts = (int)std::min<long long>(ntiles, NM_IN_MAXPARTS), tiles = (int)std::min<long long>(ntiles, NM_IN_MAXTILES);
    PT* part = static_cast<PT*>(part_ws);
    hipStream_t s = c->stream;
    int rc = nm_check_hip(hipMemsetAsync(vox, 0, (size_t)B * T * G * G * G * sizeof(float), s), "voxelize_batch: memset");
    if (rc) return rc;
    if ((rc = nm_check_hip(hipMemsetAsync(bad_rows, 0, (size_t)B * sizeof(int32_t), s), "voxelize_batch: memset"))) return rc;
    hipLaunchKernelGGL(clip_bbox_kernel<PT>, dim3(nparts, B), dim3(NM_IN_BLOCK), 0, s, clips, T, N, part);
    hipLaunchKernelGGL(voxelize_batch_kernel<PT>, dim3((unsigned)T * tiles, B), dim3(NM_IN_BLOCK), 0, s, clips, T, N, G, tiles, (const PT*)part, nparts,
                       vox, idx_out, bbox_out, bad_rows);
    if (J > 0) {
        const dim3 jg((unsigned)std::min((T * J * 3 + NM_IN_BLOCK - 1) / NM_IN_BLOCK, 64), B);
        if (joints_f64)
            hipLaunchKernelGGL((joints_norm_kernel<PT, double, double>), jg, dim3(NM_IN_BLOCK), 0, s, clips, T, J, (const PT*)part, nparts, static_cast<double*>(joints_out));
        else                                        // float32 joints: float32 result only beside float32 points
            hipLaunchKernelGGL((joints_norm_kernel<PT, float, PT>), jg, dim3(NM_IN_BLOCK), 0, s, clips, T, J, (const PT*)part, nparts, static_cast<PT*>(joints_out));
    }
    return nm_check_hip(hipGetLastError(), "voxelize_batch launch");
}

}  // namespace

extern "C" {

int nm_voxelize_batch(nm_ctx* c, const nm_clip_desc* clips_dev, int32_t B, int32_t T, int64_t N, int32_t J, int32_t points_f64, int32_t joints_f64,
                      float* vox, void* joints_out, int32_t* idx_out, double* bbox_out, int32_t* bad_rows) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("voxelize_batch: null ctx"); return NM_ERR_ARG; }
    if (!clips_dev || !vox || !bad_rows) { nm_set_error("voxelize_batch: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || N < 1 || J < 0) { nm_set_error("voxelize_batch: B = %d clips, T = %d frames, N = %lld points, J = %d joints", (int)B, (int)T, (long long)N, (int)J); return NM_ERR_ARG; }
    if (J > 0 && !joints_out) { nm_set_error("voxelize_batch: J = %d joints without joints_out", (int)J); return NM_ERR_ARG; }
    if (B > NM_IN_MAXB || (long long)T * NM_IN_MAXTILES > 0x7fffffffLL || (long long)T * J * 3 > 0x7fffffffLL || N > (1LL << 40)) {
        nm_set_error("voxelize_batch: B = %d, T = %d, N = %lld, J = %d exceed the launch grid", (int)B, (int)T, (long long)N, (int)J);
        return NM_ERR_UNSUPPORTED;
    }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    const size_t part_bytes = (size_t)B * NM_IN_MAXPARTS * 6 * sizeof(double);
    if ((rc = nm_ctx_reserve(c, part_bytes + 4096))) return rc;       // (grows the workspace only the first time)
    c->ws.release(0);
    void* part = c->ws.alloc_bytes(part_bytes);
    if (!part) { nm_set_error("voxelize_batch: workspace"); return NM_ERR_INTERNAL; }
    return points_f64 ? launch_batch<double>(c, clips_dev, B, T, N, J, joints_f64, vox, joints_out, idx_out, bbox_out, bad_rows, part)
                      : launch_batch<float>(c, clips_dev, B, T, N, J, joints_f64, vox, joints_out, idx_out, bbox_out, bad_rows, part);
} catch (...) { return nm_abi_catch("nm_voxelize_batch"); }

}  // extern "C"
