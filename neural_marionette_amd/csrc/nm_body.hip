// Body models on the device: SMPL-form linear blend skinning with shape and pose blend shapes, and the joint regression over the posed
// vertices - what the reference's AIST++ preparation computes on the host with smplx before it samples the surface
// (dataset/aistpp/prepare_aistpp.py:54-62, :86-89).  This is NOT smplx's float32 arithmetic: the contract is the library's own, float64,
// unfused, written out in include/nm355.h and restated in tests/body_ref.py.  The model arrives as plain arrays
// (neural_marionette_amd/body.py, BodyModel).
//   body_shaped_kernel     a lane per (vertex, component): v_shaped = v_template + the shape blend shapes, s ascending
//   body_regress_kernel    a lane per (frame, joint, component): its CSR row of the regressor over (frames of) vertices, in row order -
//                          J_rest from v_shaped (one "frame") and joints from the finished vertices
//   body_rodrigues_kernel  a lane per (frame, joint): axis-angle to rotation, the one stage with sin, cos and a square root
//   body_chain_kernel      a lane per (frame, row of the 3x4 transforms) walking the J joints, the parents' rows in LDS: posed joints,
//                          skinning transforms
//   body_vertices_kernel   the hot one: a lane per vertex, NM_BODY_FRAMES frames per read of posedirs (nm_body.h)
// (the library is built with -ffp-contract=off: every line is numpy's operation order, unfused.)  No atomics: every output is written
// once by the lane that owns it, results are bit-identical from run to run.
#include "nm_ctx.h"
#include "nm_body.h"
#include <cmath>

namespace {

// grid ceil(3 V / 256): column i = 3 v + c
__global__ __launch_bounds__(NM_BODY_SMALL) void body_shaped_kernel(const double* __restrict__ v_template, const double* __restrict__ shapedirs,
                                                                     const double* __restrict__ betas, long long cols, int S, double* __restrict__ v_shaped) {
    const long long i = (long long)blockIdx.x * NM_BODY_SMALL + threadIdx.x;
    if (i >= cols) return;
    double s = v_template[i];
    const double* d = shapedirs + (size_t)i * (size_t)S;
    for (int k = 0; k < S; ++k) s = s + d[k] * betas[k];
    v_shaped[i] = s;
}

// grid ceil(T J 3 / 256): out[t,j,c] = the running sum over row j's entries of val * x[t,col,c].  The table is judged before anything is
// read through it: a row with an offset pair outside [0, nnz] or a column outside [0, V) is quiet NaN.
__global__ __launch_bounds__(NM_BODY_SMALL) void body_regress_kernel(const double* __restrict__ x, long long n, int V, int J, const int* __restrict__ offsets,
                                                                      const int* __restrict__ cols, const double* __restrict__ vals, int nnz,
                                                                      double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NM_BODY_SMALL + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 3), j = (int)((i / 3) % J);
    const long long t = i / (3 * (long long)J);
    const double* xf = x + (size_t)t * (size_t)V * 3 + c;
    const int lo = offsets[j], hi = offsets[j + 1];
    bool bad = lo < 0 || hi > nnz || lo > hi;
    double s = 0.0;
    if (!bad)
        for (int k = lo; k < hi; ++k) {
            const int col = cols[k];
            if (col < 0 || col >= V) { bad = true; break; }
            s = s + vals[k] * xf[(size_t)col * 3];
        }
    out[i] = bad ? __builtin_nan("") : s;
}

// grid ceil(T J / 256): rotation (t, j) from the axis-angle vector (t, j)
template <typename PT>
__global__ __launch_bounds__(NM_BODY_SMALL) void body_rodrigues_kernel(const PT* __restrict__ poses, long long n, double* __restrict__ rot) {
    const long long i = (long long)blockIdx.x * NM_BODY_SMALL + threadIdx.x;
    if (i >= n) return;
    const double rx = (double)poses[3 * i], ry = (double)poses[3 * i + 1], rz = (double)poses[3 * i + 2];
    const double ex = rx + 1e-8, ey = ry + 1e-8, ez = rz + 1e-8;
    const double angle = sqrt((ex * ex + ey * ey) + ez * ez);
    const double ux = rx / angle, uy = ry / angle, uz = rz / angle;
    const double s = sin(angle), c1 = 1.0 - cos(angle);
    const double K[3][3] = {{0.0, -uz, uy}, {uz, 0.0, -ux}, {-uy, ux, 0.0}};
    double* R = rot + 9 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double kk = (K[a][0] * K[0][b] + K[a][1] * K[1][b]) + K[a][2] * K[2][b];
            R[3 * a + b] = ((a == b ? 1.0 : 0.0) + s * K[a][b]) + c1 * kk;
        }
}

// grid ceil(3 T / L), L lanes a workgroup: lane (t, a) walks the J joints for row a of frame t's transforms - row a of [Gr_j | Gt_j] needs
// row a of the parent's only, which the lane keeps in LDS ([joint][entry][lane], J * 4 * L doubles; the host picks L so that they fit
// NM_BODY_CHAIN_LDS), so no joint waits for a global store of the one before.  tr (T,J,3,4) receives [Gr_j | Gt_j - Gr_j J_rest_j].
__global__ __launch_bounds__(NM_BODY_SMALL) void body_chain_kernel(const double* __restrict__ rot, int T, int J, NmBodyParents par, const double* __restrict__ J_rest,
                                  const double* __restrict__ transl, double scaling, double* __restrict__ tr, double* __restrict__ posed_joints) {
    extern __shared__ double body_sh[];
    const int L = blockDim.x, lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * L + lane;
    if (i >= 3ll * T) return;
    const int a = (int)(i % 3);
    const size_t t = (size_t)(i / 3);
    const double* fr = rot + t * (size_t)J * 9;
    double* ft = tr + t * (size_t)J * 12 + 4 * a;
    const double tl = transl ? transl[3 * t + a] : 0.0;
    for (int j = 0; j < J; ++j) {
        const double* R = fr + 9 * j;
        const double j0 = J_rest[3 * j], j1 = J_rest[3 * j + 1], j2 = J_rest[3 * j + 2];
        double g0, g1, g2, gt;
        if (j == 0) {
            g0 = R[3 * a]; g1 = R[3 * a + 1]; g2 = R[3 * a + 2]; gt = J_rest[a];
        } else {
            const int p = par.p[j];
            const double* P = body_sh + (size_t)p * 4 * L + lane;
            const double p0 = P[0], p1 = P[L], p2 = P[2 * L];
            const double r0 = j0 - J_rest[3 * p], r1 = j1 - J_rest[3 * p + 1], r2 = j2 - J_rest[3 * p + 2];
            g0 = (p0 * R[0] + p1 * R[3]) + p2 * R[6];
            g1 = (p0 * R[1] + p1 * R[4]) + p2 * R[7];
            g2 = (p0 * R[2] + p1 * R[5]) + p2 * R[8];
            gt = ((p0 * r0 + p1 * r1) + p2 * r2) + P[3 * L];
        }
        double* G = body_sh + (size_t)j * 4 * L + lane;
        G[0] = g0; G[L] = g1; G[2 * L] = g2; G[3 * L] = gt;
        const double q = scaling * gt;
        posed_joints[(t * (size_t)J + (size_t)j) * 3 + a] = transl ? q + tl : q;
        ft[12 * j] = g0; ft[12 * j + 1] = g1; ft[12 * j + 2] = g2;
        ft[12 * j + 3] = gt - ((g0 * j0 + g1 * j1) + g2 * j2);
    }
}

// grid nVB * groups of frames: workgroup g * nVB + b takes vertices [128 b, 128 b + 128) of the frames 8 g ... 8 g + 7.  Dynamic LDS:
// NM_BODY_FRAMES * J * 12 doubles, first the pose features [row p][frame], then the skinning transforms [joint][entry][frame].
__global__ __launch_bounds__(NM_BODY_BLOCK) void body_vertices_kernel(const double* __restrict__ rot, const double* __restrict__ tr, int T, int V, int J, int nVB,
                                                                       const double* __restrict__ v_shaped, const double* __restrict__ posedirs,
                                                                       const double* __restrict__ weights, const double* __restrict__ transl, double scaling,
                                                                       double* __restrict__ vertices) {
    extern __shared__ double body_sh[];
    constexpr int NF = NM_BODY_FRAMES;
    const int g = blockIdx.x / nVB, b = blockIdx.x - g * nVB, tid = threadIdx.x;
    const int f0 = g * NF, nf = T - f0 < NF ? T - f0 : NF;
    const int v = b * NM_BODY_BLOCK + tid;
    const bool live = v < V;
    const int P = 9 * (J - 1);
    // pose features: row p = 9 (j - 1) + 3 a + b is entry 9 + p of the frame's (J,3,3) rotations, minus the identity's
    for (int i = tid; i < P * NF; i += NM_BODY_BLOCK) {
        const int p = i / NF, f = i - p * NF;
        const int ab = p % 9;
        body_sh[i] = f < nf ? rot[((size_t)(f0 + f) * (size_t)J) * 9 + 9 + p] - ((ab == 0 || ab == 4 || ab == 8) ? 1.0 : 0.0) : 0.0;
    }
    __syncthreads();
    double off[NF][3];
#pragma unroll
    for (int f = 0; f < NF; ++f) off[f][0] = off[f][1] = off[f][2] = 0.0;
    if (live) {
        const size_t cols = (size_t)V * 3;
        const double* pd = posedirs + (size_t)v * 3;
        for (int p = 0; p < P; ++p) {
            const double d0 = pd[0], d1 = pd[1], d2 = pd[2];
            const double* ft = body_sh + p * NF;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const double x = ft[f];
                off[f][0] = off[f][0] + x * d0; off[f][1] = off[f][1] + x * d1; off[f][2] = off[f][2] + x * d2;
            }
            pd += cols;
        }
    }
    __syncthreads();                                               // the features are read; the same LDS takes the transforms
    for (int i = tid; i < J * 12 * NF; i += NM_BODY_BLOCK) {
        const int jk = i / NF, f = i - jk * NF;
        body_sh[i] = f < nf ? tr[(size_t)(f0 + f) * (size_t)J * 12 + jk] : 0.0;
    }
    __syncthreads();
    if (!live) return;
    const double s0 = v_shaped[(size_t)v * 3], s1 = v_shaped[(size_t)v * 3 + 1], s2 = v_shaped[(size_t)v * 3 + 2];
    const double* w = weights + (size_t)v * (size_t)J;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (f < nf) {
            const double px = s0 + off[f][0], py = s1 + off[f][1], pz = s2 + off[f][2];
            double M[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) M[k] = 0.0;
            for (int j = 0; j < J; ++j) {
                const double wj = w[j];
                if (wj == 0.0) continue;
                const double* A = body_sh + (size_t)j * 12 * NF + f;
#pragma unroll
                for (int k = 0; k < 12; ++k) M[k] = M[k] + wj * A[k * NF];
            }
            const size_t t = (size_t)(f0 + f);
            double* out = vertices + (t * (size_t)V + (size_t)v) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x = ((M[4 * c] * px + M[4 * c + 1] * py) + M[4 * c + 2] * pz) + M[4 * c + 3];
                const double q = scaling * x;
                out[c] = transl ? q + transl[3 * t + c] : q;
            }
        }
    }
}

// the regressor's table arguments, judged on the host
int body_regressor_args(const char* who, int32_t V, int32_t J, const int32_t* offsets, const int32_t* cols, const double* vals, int32_t nnz) {
    if (V < 1 || J < 1 || J > NM_BODY_MAX_JOINTS || nnz < 0) {
        nm_set_error("%s: V = %d vertices, J = %d joints (at most %d), %d regressor entries", who, (int)V, (int)J, NM_BODY_MAX_JOINTS, (int)nnz);
        return NM_ERR_ARG;
    }
    if (!offsets || (nnz > 0 && (!cols || !vals))) { nm_set_error("%s: null regressor table", who); return NM_ERR_ARG; }
    return NM_OK;
}

unsigned body_blocks(long long n) { return (unsigned)((n + NM_BODY_SMALL - 1) / NM_BODY_SMALL); }

}  // namespace

extern "C" {

int nm_body_shape(nm_ctx* c, const double* v_template, const double* shapedirs, const double* betas, int32_t V, int32_t S, int32_t J,
                  const int32_t* reg_offsets, const int32_t* reg_cols, const double* reg_vals, int32_t reg_nnz, double* v_shaped,
                  double* J_rest) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("body_shape: null ctx"); return NM_ERR_ARG; }
    int rc = body_regressor_args("body_shape", V, J, reg_offsets, reg_cols, reg_vals, reg_nnz);
    if (rc) return rc;
    if (S < 0) { nm_set_error("body_shape: S = %d shape coefficients", (int)S); return NM_ERR_ARG; }
    if (!betas) S = 0;
    if (!v_template || !v_shaped || !J_rest || (S > 0 && !shapedirs)) { nm_set_error("body_shape: null argument"); return NM_ERR_ARG; }
    const long long cols = 3 * (long long)V;
    if (cols >= (1ll << 31)) { nm_set_error("body_shape: %d vertices, a model indexes fewer than 2^31 vertex components", (int)V); return NM_ERR_UNSUPPORTED; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(body_shaped_kernel, dim3(body_blocks(cols)), dim3(NM_BODY_SMALL), 0, s, v_template, shapedirs, betas, cols, (int)S, v_shaped);
    hipLaunchKernelGGL(body_regress_kernel, dim3(body_blocks(3ll * J)), dim3(NM_BODY_SMALL), 0, s, (const double*)v_shaped, 3ll * J, (int)V, (int)J,
                       (const int*)reg_offsets, (const int*)reg_cols, reg_vals, (int)reg_nnz, J_rest);
    return nm_check_hip(hipGetLastError(), "body_shape launch");
} catch (...) { return nm_abi_catch("nm_body_shape"); }

int nm_body_pose(nm_ctx* c, const void* poses, int32_t poses_f64, const double* rotations, int32_t T, int32_t V, int32_t J, const int32_t* parents,
                 const double* v_shaped, const double* J_rest, const double* posedirs, const double* lbs_weights, const double* transl,
                 double scaling, double* rotations_out, double* transforms, double* posed_joints, double* vertices) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("body_pose: null ctx"); return NM_ERR_ARG; }
    if (T < 1 || V < 1 || J < 1 || J > NM_BODY_MAX_JOINTS) {
        nm_set_error("body_pose: T = %d frames, V = %d vertices, J = %d joints (at most %d)", (int)T, (int)V, (int)J, NM_BODY_MAX_JOINTS);
        return NM_ERR_ARG;
    }
    if ((poses == nullptr) == (rotations == nullptr)) { nm_set_error("body_pose: exactly one of poses and rotations is given"); return NM_ERR_ARG; }
    if (!parents || !v_shaped || !J_rest || !lbs_weights || !transforms || !posed_joints || !vertices || (poses && !rotations_out) || (J > 1 && !posedirs)) {
        nm_set_error("body_pose: null argument");
        return NM_ERR_ARG;
    }
    NmBodyParents par;
    for (int j = 0; j < NM_BODY_MAX_JOINTS; ++j) par.p[j] = -1;
    for (int j = 0; j < J; ++j) {
        if (j == 0 ? parents[0] != -1 : (parents[j] < 0 || parents[j] >= j)) {
            nm_set_error("body_pose: parents[%d] = %d: the root's is -1, every other joint's lies in [0, its own index)", j, (int)parents[j]);
            return NM_ERR_ARG;
        }
        par.p[j] = parents[j];
    }
    if (!std::isfinite(scaling) || scaling == 0.0) { nm_set_error("body_pose: scaling = %g must be finite and not zero", scaling); return NM_ERR_ARG; }
    const long long lim = 1ll << 31;
    const long long nVB = ((long long)V + NM_BODY_BLOCK - 1) / NM_BODY_BLOCK, groups = ((long long)T + NM_BODY_FRAMES - 1) / NM_BODY_FRAMES;
    if ((long long)T * V >= lim || (long long)T * J >= lim || 3ll * V >= lim || nVB * groups >= lim) {
        nm_set_error("body_pose: T = %d frames of %d vertices and %d joints, one call indexes fewer than 2^31 rows", (int)T, (int)V, (int)J);
        return NM_ERR_UNSUPPORTED;
    }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    hipStream_t s = c->stream;
    const double* rot = rotations;
    if (poses) {
        const long long n = (long long)T * J;
        if (poses_f64) hipLaunchKernelGGL(body_rodrigues_kernel<double>, dim3(body_blocks(n)), dim3(NM_BODY_SMALL), 0, s, static_cast<const double*>(poses), n, rotations_out);
        else hipLaunchKernelGGL(body_rodrigues_kernel<float>, dim3(body_blocks(n)), dim3(NM_BODY_SMALL), 0, s, static_cast<const float*>(poses), n, rotations_out);
        rot = rotations_out;
    }
    int L = NM_BODY_CHAIN_LDS / ((int)J * 4 * (int)sizeof(double));                 // 64 lanes at J = 24, 24 at the limit of 64 joints
    L = L > NM_BODY_SMALL ? NM_BODY_SMALL : L;
    hipLaunchKernelGGL(body_chain_kernel, dim3((unsigned)((3ll * T + L - 1) / L)), dim3((unsigned)L), (size_t)J * 4 * L * sizeof(double), s, rot, (int)T, (int)J, par, J_rest,
                       transl, scaling, transforms, posed_joints);
    const size_t lds = (size_t)NM_BODY_FRAMES * (size_t)J * 12 * sizeof(double);
    hipLaunchKernelGGL(body_vertices_kernel, dim3((unsigned)(nVB * groups)), dim3(NM_BODY_BLOCK), lds, s, rot, (const double*)transforms, (int)T, (int)V, (int)J, (int)nVB,
                       v_shaped, posedirs, lbs_weights, transl, scaling, vertices);
    return nm_check_hip(hipGetLastError(), "body_pose launch");
} catch (...) { return nm_abi_catch("nm_body_pose"); }

int nm_body_joints(nm_ctx* c, const double* vertices, int32_t T, int32_t V, int32_t J, const int32_t* reg_offsets, const int32_t* reg_cols,
                   const double* reg_vals, int32_t reg_nnz, double* joints) try { NmScope nm_scope_(c);
    if (!c) { nm_set_error("body_joints: null ctx"); return NM_ERR_ARG; }
    int rc = body_regressor_args("body_joints", V, J, reg_offsets, reg_cols, reg_vals, reg_nnz);
    if (rc) return rc;
    if (T < 1) { nm_set_error("body_joints: T = %d frames", (int)T); return NM_ERR_ARG; }
    if (!vertices || !joints) { nm_set_error("body_joints: null argument"); return NM_ERR_ARG; }
    const long long lim = 1ll << 31, n = 3ll * T * J;
    if ((long long)T * V >= lim || n >= lim) {
        nm_set_error("body_joints: T = %d frames of %d vertices and %d joints, one call indexes fewer than 2^31 rows", (int)T, (int)V, (int)J);
        return NM_ERR_UNSUPPORTED;
    }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    hipLaunchKernelGGL(body_regress_kernel, dim3(body_blocks(n)), dim3(NM_BODY_SMALL), 0, c->stream, vertices, n, (int)V, (int)J, (const int*)reg_offsets,
                       (const int*)reg_cols, reg_vals, (int)reg_nnz, joints);
    return nm_check_hip(hipGetLastError(), "body_joints launch");
} catch (...) { return nm_abi_catch("nm_body_joints"); }

}  // extern "C"
