// Motion retargeting on the device: the computation of the reference's vis_retarget.py between its two detector calls and its
// first render - extract_skin_weights (:21-62) with the local coordinates of :268-270 (bind), the re-posing loop of :275-300
// (fk) and the blend of :303-322 (pose).
//
// The reference walks the N target points in a Python loop and blends with a dense (N,K) x (K,4,N) contraction per frame although a
// row of its weight matrix has at most two non-zero entries (the nearest bone's child joint and that joint's parent).  Here a point
// is bound once to a record {child, parent, two weights, two local positions} and every frame is posed from the record: two
// streaming kernels whose cost is the (T,N,3) float64 output.
//
// Arithmetic.  The reference's points are float64 numpy, so its distances, weights and blend are float64 against fp32 keypoints and
// rotations; the bind kernel repeats that operation by operation (the library is built with -ffp-contract=off), the pose kernel uses
// explicit fused multiply-adds (its reference is an einsum whose summation order is not defined either).
//
// One place has no reference behaviour to match: the ancestor walk of :41-42 looks for the nearest valid ancestor and never ends
// when it reaches an INVALID root (parents[root] == root).  The walk here stops at the root whatever its intensity, and is bounded by
// K steps.
#include "nm_ctx.h"
#include "nm_retarget.h"

namespace {

// ---- bind ------------------------------------------------------------------------------------------------------------------------
// One point per thread, grid-stride.  Every workgroup first builds the K-entry tables in LDS: joint positions and bone points as
// float64 (the values are fp32 results, widened as the reference's float64 - fp32 subtraction widens them), the selection mask and
// R_bind^T; lane k of the first wave does joint k's ancestor walk.
__global__ __launch_bounds__(NM_RT_BLOCK) void retarget_bind_kernel(
    const double* __restrict__ points, long long N, const float* __restrict__ kp, const float* __restrict__ Rb,
    const int32_t* __restrict__ parents, const int32_t* __restrict__ order, int K, double hardness, float thr,
    const int32_t* __restrict__ force, int32_t* __restrict__ child_out, int32_t* __restrict__ parent_out, float* __restrict__ w_out,
    double* __restrict__ local_out, double* __restrict__ margin_out, float* __restrict__ dense) {
    __shared__ double s_pos[NM_RT_MAXK * 3], s_bone[NM_RT_MAXK * 3];
    __shared__ float s_rt[NM_RT_MAXK * 9];
    __shared__ int s_mask[NM_RT_MAXK], s_par[NM_RT_MAXK];
    const int tid = threadIdx.x;
    if (tid < K) {
        const int k = tid, root = order[0];
        const float x = kp[4 * k], y = kp[4 * k + 1], z = kp[4 * k + 2];
        const int par = parents[k];
        float bx = x, by = y, bz = z;                       // the root's bone point is the joint itself
        if (par != k) {
            int a = par;                                    // nearest ancestor that is not invalid; stops at the root, at most K steps
            for (int step = 0; step < K && kp[4 * a + 3] < thr && parents[a] != a; ++step) a = parents[a];
            bx = (x + kp[4 * a]) / 2.f; by = (y + kp[4 * a + 1]) / 2.f; bz = (z + kp[4 * a + 2]) / 2.f;
        }
        s_pos[3 * k] = (double)x; s_pos[3 * k + 1] = (double)y; s_pos[3 * k + 2] = (double)z;
        s_bone[3 * k] = (double)bx; s_bone[3 * k + 1] = (double)by; s_bone[3 * k + 2] = (double)bz;
        s_mask[k] = (kp[4 * k + 3] < thr) || k == root;     // these joints' distance is the VALUE 1e4, as the reference assigns it
        s_par[k] = par;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) s_rt[9 * k + 3 * i + j] = Rb ? Rb[9 * k + 3 * j + i] : (i == j ? 1.f : 0.f);
    }
    __syncthreads();
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (long long n = (long long)blockIdx.x * NM_RT_BLOCK + tid; n < N; n += (long long)gridDim.x * NM_RT_BLOCK) {
        const double px = points[3 * n], py = points[3 * n + 1], pz = points[3 * n + 2];
        double best = inf, second = inf;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const double dx = px - s_bone[3 * k], dy = py - s_bone[3 * k + 1], dz = pz - s_bone[3 * k + 2];
            double d = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
            if (s_mask[k]) d = 1e4;
            if (k == 0 || d < best) { second = best; best = d; arg = k; }      // first minimum, as argmin
            else if (d < second) second = d;
        }
        int c = arg;
        if (force) { c = force[n]; c = c < 0 ? 0 : (c >= K ? K - 1 : c); }     // (the caller checks the range; clamped for memory safety)
        const int p = s_par[c];                                                // from the ORIGINAL tree: may be an invalid joint
        const double cx = px - s_pos[3 * c], cy = py - s_pos[3 * c + 1], cz = pz - s_pos[3 * c + 2];
        const double qx = px - s_pos[3 * p], qy = py - s_pos[3 * p + 1], qz = pz - s_pos[3 * p + 2];
        const double ec = exp(__dsqrt_rn((cx * cx + cy * cy) + cz * cz) * hardness);
        const double ep = exp(__dsqrt_rn((qx * qx + qy * qy) + qz * qz) * hardness);
        const float wc = (float)(ep / (ec + ep));
        const float wp = (p == c) ? 0.f : (float)(ec / (ec + ep));             // root chosen: the child's assignment overwrote the parent's
        child_out[n] = c;
        parent_out[n] = p;
        reinterpret_cast<float2*>(w_out)[n] = make_float2(wc, wp);
        const float* rc = s_rt + 9 * c; const float* rp = s_rt + 9 * p;
        double l[6];
        for (int i = 0; i < 3; ++i) {
            l[i] = ((double)rc[3 * i] * cx + (double)rc[3 * i + 1] * cy) + (double)rc[3 * i + 2] * cz;
            l[3 + i] = ((double)rp[3 * i] * qx + (double)rp[3 * i + 1] * qy) + (double)rp[3 * i + 2] * qz;
        }
        double2* lo = reinterpret_cast<double2*>(local_out + 6 * n);          // 48-byte record, 16-byte aligned
        lo[0] = make_double2(l[0], l[1]); lo[1] = make_double2(l[2], l[3]); lo[2] = make_double2(l[4], l[5]);
        if (margin_out) margin_out[n] = second - best;
        if (dense) {
            float* row = dense + (size_t)n * K;
            for (int k = 0; k < K; ++k) row[k] = (k == c) ? wc : (k == p ? wp : 0.f);
        }
    }
}

// ---- fk --------------------------------------------------------------------------------------------------------------------------
// pos[t, root] = root_pos[t]; pos[t, j] = R[t, j] offset[j] + pos[t, parents[j]] in `order`, fp32, clipped to [-1, 1] at the end (the
// children are chained from the unclipped positions, as the reference clips the stacked result).  A thread per frame; the frame's
// chain lives in LDS ([component][thread]: no bank conflicts, no scratch).
__global__ __launch_bounds__(NM_RT_FK_BLOCK) void retarget_fk_kernel(
    const float* __restrict__ R, const float* __restrict__ root_pos, const float* __restrict__ offset, const int32_t* __restrict__ parents,
    const int32_t* __restrict__ order, int T, int K, float* __restrict__ pos) {
    extern __shared__ float s_chain[];                      // [K * 3][NM_RT_FK_BLOCK]
    const int tid = threadIdx.x, t = blockIdx.x * NM_RT_FK_BLOCK + tid;
    if (t >= T) return;
    const int root = order[0];
    for (int i = 0; i < 3; ++i) s_chain[(3 * root + i) * NM_RT_FK_BLOCK + tid] = root_pos[3 * (size_t)t + i];
    for (int q = 1; q < K; ++q) {
        const int j = order[q], p = parents[j];
        const float* M = R + ((size_t)t * K + j) * 9;
        const float ox = offset[3 * j], oy = offset[3 * j + 1], oz = offset[3 * j + 2];
        for (int i = 0; i < 3; ++i)
            s_chain[(3 * j + i) * NM_RT_FK_BLOCK + tid] = ((M[3 * i] * ox + M[3 * i + 1] * oy) + M[3 * i + 2] * oz) + s_chain[(3 * p + i) * NM_RT_FK_BLOCK + tid];
    }
    float* o = pos + (size_t)t * K * 3;
    for (int e = 0; e < 3 * K; ++e) o[e] = fminf(fmaxf(s_chain[e * NM_RT_FK_BLOCK + tid], -1.f), 1.f);
}

// ---- pose ------------------------------------------------------------------------------------------------------------------------
// out[t, n, :] = w_c (R[t,c] local_c + pos[t,c]) + w_p (R[t,p] local_p + pos[t,p]) in float64.  Grid: point tiles x frame chunks.  A
// thread keeps its point's bind record in registers and walks the chunk's frames; the chunk's K x 12 transforms are staged in LDS as
// float64.  The kernel is bound by its 24 T N bytes of stores, and a thread's own result is three doubles at a 24-byte stride, so
// the tile's 3 x 256 results of a frame pass through a double-buffered LDS stage (one barrier per frame) and leave as one contiguous
// run of 16-byte stores; a run that begins at an odd element (t N odd) peels its first element.
__global__ __launch_bounds__(NM_RT_BLOCK) void retarget_pose_kernel(
    const int32_t* __restrict__ child, const int32_t* __restrict__ parent, const float* __restrict__ w, const double* __restrict__ local,
    const float* __restrict__ R, const float* __restrict__ pos, int T, long long N, int K, double* __restrict__ out) {
    extern __shared__ double s_pose[];
    double* s_tr = s_pose;                                   // [NM_RT_TC][K][12]: R row-major, then the position
    double* s_out = s_pose + (size_t)NM_RT_TC * K * 12;      // [2][3 * NM_RT_BLOCK]
    const int tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * NM_RT_BLOCK, n = n0 + tid;
    const int t0 = blockIdx.y * NM_RT_TC, nt = min(NM_RT_TC, T - t0);
    for (int i = tid; i < nt * K * 12; i += NM_RT_BLOCK) {
        const int tk = i / 12, e = i - 12 * tk;
        const size_t g = (size_t)t0 * K + tk;
        s_tr[i] = e < 9 ? (double)R[g * 9 + e] : (double)pos[g * 3 + (e - 9)];
    }
    const bool valid = n < N;
    int c = 0, p = 0;
    double wc = 0., wp = 0., lc[3] = {0., 0., 0.}, lp[3] = {0., 0., 0.};
    if (valid) {
        c = min(max(child[n], 0), K - 1); p = min(max(parent[n], 0), K - 1);
        const float2 ww = reinterpret_cast<const float2*>(w)[n];
        wc = (double)ww.x; wp = (p == c) ? 0. : (double)ww.y;
        const double2* lo = reinterpret_cast<const double2*>(local + 6 * n);
        const double2 a = lo[0], b = lo[1], d = lo[2];
        lc[0] = a.x; lc[1] = a.y; lc[2] = b.x; lp[0] = b.y; lp[1] = d.x; lp[2] = d.y;
    }
    const int len = 3 * (int)min((long long)NM_RT_BLOCK, N - n0);
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {
        double* st = s_out + (tt & 1) * (3 * NM_RT_BLOCK);
        if (valid) {
            const double* Mc = s_tr + ((size_t)tt * K + c) * 12; const double* Mp = s_tr + ((size_t)tt * K + p) * 12;
            for (int i = 0; i < 3; ++i) {
                const double kc = fma(Mc[3 * i], lc[0], fma(Mc[3 * i + 1], lc[1], fma(Mc[3 * i + 2], lc[2], Mc[9 + i])));
                const double kq = fma(Mp[3 * i], lp[0], fma(Mp[3 * i + 1], lp[1], fma(Mp[3 * i + 2], lp[2], Mp[9 + i])));
                st[3 * tid + i] = fma(wc, kc, wp * kq);
            }
        }
        __syncthreads();
        const size_t e0 = ((size_t)(t0 + tt) * (size_t)N + (size_t)n0) * 3;
        const int head = (int)(e0 & 1), pairs = (len - head) >> 1;
        for (int i = tid; i < pairs; i += NM_RT_BLOCK)
            *reinterpret_cast<double2*>(out + e0 + head + 2 * i) = make_double2(st[head + 2 * i], st[head + 2 * i + 1]);
        if (tid == 0 && head) out[e0] = st[0];
        if (tid == 1 && ((len - head) & 1)) out[e0 + len - 1] = st[len - 1];
    }
}

int retarget_ready(nm_ctx* c, const char* who, int32_t K) {
    if (!c) { nm_set_error("%s: null ctx", who); return NM_ERR_ARG; }
    if (!c->vrnn.has_tree) { nm_set_error("%s: nm_vrnn_set_tree has not been called (the reference builds it in encode())", who); return NM_ERR_STATE; }
    if (K != c->cfg.nkeypoints) { nm_set_error("%s: K = %d, the context has %d keypoints", who, (int)K, (int)c->cfg.nkeypoints); return NM_ERR_ARG; }
    if (K > NM_RT_MAXK) { nm_set_error("%s: K = %d exceeds %d", who, (int)K, NM_RT_MAXK); return NM_ERR_UNSUPPORTED; }
    return nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
}

}  // namespace

extern "C" {

int nm_retarget_bind(nm_ctx* c, const double* points, int64_t N, const float* keypoints, const float* R_bind, int32_t K, double hardness,
                     double threshold, const int32_t* force_child, int32_t* child, int32_t* parent, float* w, double* local,
                     double* margin, float* dense) try { NmScope nm_scope_(c);
    int rc = retarget_ready(c, "retarget_bind", K);
    if (rc) return rc;
    if (N < 1) { nm_set_error("retarget_bind: N = %lld points", (long long)N); return NM_ERR_ARG; }
    if (!points || !keypoints || !child || !parent || !w || !local) { nm_set_error("retarget_bind: null argument"); return NM_ERR_ARG; }
    const long long tiles = ((long long)N + NM_RT_BLOCK - 1) / NM_RT_BLOCK;
    const unsigned grid = (unsigned)std::min<long long>(tiles, 4096);
    hipLaunchKernelGGL(retarget_bind_kernel, dim3(grid), dim3(NM_RT_BLOCK), 0, c->stream, points, (long long)N, keypoints, R_bind,
                       c->vrnn.parents, c->vrnn.order, (int)K, hardness, (float)threshold, force_child, child, parent, w, local, margin, dense);
    return nm_check_hip(hipGetLastError(), "retarget_bind launch");
} catch (...) { return nm_abi_catch("nm_retarget_bind"); }

int nm_retarget_fk(nm_ctx* c, const float* R, const float* root_pos, const float* offset, int32_t T, int32_t K, float* pos) try { NmScope nm_scope_(c);
    int rc = retarget_ready(c, "retarget_fk", K);
    if (rc) return rc;
    if (T < 1) { nm_set_error("retarget_fk: T = %d frames", (int)T); return NM_ERR_ARG; }
    if (!R || !root_pos || !offset || !pos) { nm_set_error("retarget_fk: null argument"); return NM_ERR_ARG; }
    hipLaunchKernelGGL(retarget_fk_kernel, dim3((T + NM_RT_FK_BLOCK - 1) / NM_RT_FK_BLOCK), dim3(NM_RT_FK_BLOCK),
                       (size_t)K * 3 * NM_RT_FK_BLOCK * sizeof(float), c->stream, R, root_pos, offset, c->vrnn.parents, c->vrnn.order, (int)T, (int)K, pos);
    return nm_check_hip(hipGetLastError(), "retarget_fk launch");
} catch (...) { return nm_abi_catch("nm_retarget_fk"); }

int nm_retarget_pose(nm_ctx* c, const int32_t* child, const int32_t* parent, const float* w, const double* local, const float* R,
                     const float* pos, int32_t T, int64_t N, int32_t K, double* out) try { NmScope nm_scope_(c);
    int rc = retarget_ready(c, "retarget_pose", K);
    if (rc) return rc;
    if (N < 1 || T < 1) { nm_set_error("retarget_pose: N = %lld points, T = %d frames", (long long)N, (int)T); return NM_ERR_ARG; }
    if (!child || !parent || !w || !local || !R || !pos || !out) { nm_set_error("retarget_pose: null argument"); return NM_ERR_ARG; }
    const long long tiles = ((long long)N + NM_RT_BLOCK - 1) / NM_RT_BLOCK;
    const int chunks = (T + NM_RT_TC - 1) / NM_RT_TC;
    if (tiles > 0x7fffffffLL || chunks > 65535) { nm_set_error("retarget_pose: N = %lld, T = %d exceed the launch grid", (long long)N, (int)T); return NM_ERR_UNSUPPORTED; }
    const size_t lds = ((size_t)NM_RT_TC * K * 12 + 2 * 3 * NM_RT_BLOCK) * sizeof(double);     // K = 32: 36 KiB
    hipLaunchKernelGGL(retarget_pose_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(NM_RT_BLOCK), lds, c->stream, child, parent, w, local,
                       R, pos, (int)T, (long long)N, (int)K, out);
    return nm_check_hip(hipGetLastError(), "retarget_pose launch");
} catch (...) { return nm_abi_catch("nm_retarget_pose"); }

}  // extern "C"
