// Device surface path: for every point of nm_occupied_write, from the occupancy masks alone - the moments of its lattice neighbourhood,
// a surface normal with the spread along the three principal axes, the [R | centre] rows of drawPlate's transform and the shaded
// colour: what the reference's demo scripts do per decoded frame on the host (vis_generation.py:157-171, vis_interpolation.py:160-177:
// open3d's estimate_normals + orient_normals_consistent_tangent_plane, then a Python loop over the points).
//
// These are NOT open3d's normals.  On a voxel lattice open3d's 30-nearest-neighbour set is cut inside a shell of equidistant points by
// the tie-breaking of its k-d tree, so the contract here is the library's own, in exact integer arithmetic as far as the lattice goes:
//   neighbourhood  the occupied voxels q of the point's own frame, inside the grid, with |q - p|^2 <= radius2 (1 .. 16), p included
//   moments        d = q - p:  n, S = sum d (x, y, z), Q = sum d d^T (xx, xy, xz, yy, yz, zz) - int32, exact
//   normal         C = n Q - S S^T (integer, |entries| < 2^31); the unit eigenvector of C's smallest eigenvalue in float64 (cyclic
//                  Jacobi: backward stable, and an axis that no neighbour leaves is never rotated, so a lattice plane's normal is
//                  exactly +-e); spread = C's eigenvalues, ascending; n < 3 -> (0, 0, 1) like open3d
//   orientation    orient 0: n . o >= 0 for o = -S (away from the local mass); S = 0 -> o = N_f p - sum_f q (away from the frame's
//                  centroid, int64); that 0 too -> (1, 1, 1); a dot product of exactly 0.0 leaves the solver's sign.
//                  orient 1: flipped when n . (orient_point[b] - coords(p)) < 0 (open3d's orient_normals_towards_camera_location)
//   plates         drawPlate (vis_generation.py:30-38) for centre = coords(p) and the oriented normal, rows [R | centre]
//   colours        base[f] * (depth * shade_a + shade_b) (+ add[f]), depth as nm_occupied_write defines it
// (the library is built with -ffp-contract=off: every line is numpy's operation order, unfused.)
//
// A lane per point, a workgroup per chunk of 4096 voxels as in occ_write_kernel, which also gives the rows their order.  k is the
// mask's fastest axis, so row (di, dj) of a neighbourhood is ONE window of 2 hk + 1 <= 9 bits, hk = floor(sqrt(radius2 - di^2 -
// dj^2)), clipped at the row's ends and cut from one or two 64-bit words (rows are word-aligned only when G % 64 == 0).  A table of
// the 512 windows gives sum dk and sum dk^2; the popcount gives the rest.  The window never leaves its row, so it never reads
// another frame's bits or the pad bits.  The i-planes a workgroup's windows can reach are staged in LDS up to the slab bound of
// nm_surface.h and read in place beyond it.  No atomics: results are bit-identical from run to run.
#include "nm_ctx.h"
#include "nm_output.h"
#include "nm_surface.h"

namespace {

// grid F: fsum[3 f ..] = sum of (i, j, k) over the occupied voxels of frame f (orientation's fall-back when S = 0)
__global__ __launch_bounds__(NM_SURF_BLOCK) void surf_frame_sum_kernel(const unsigned long long* __restrict__ bits, int G, int W,
                                                                       long long* __restrict__ fsum) {
    __shared__ long long sh[3 * (NM_SURF_BLOCK / 64)];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long* fb = bits + (size_t)f * (size_t)W;
    long long si = 0, sj = 0, sk = 0;
    for (int w = tid; w < W; w += NM_SURF_BLOCK) {
        unsigned long long word = fb[w];
        while (word) {
            const unsigned p = (unsigned)w * 64u + (unsigned)(__ffsll((long long)word) - 1);
            word &= word - 1ull;
            const unsigned ij = p / (unsigned)G, i = ij / (unsigned)G;
            si += i; sj += ij - i * (unsigned)G; sk += p - ij * (unsigned)G;
        }
    }
    for (int off = 32; off > 0; off >>= 1) { si += __shfl_xor(si, off); sj += __shfl_xor(sj, off); sk += __shfl_xor(sk, off); }
    if (lane == 0) { sh[wave * 3] = si; sh[wave * 3 + 1] = sj; sh[wave * 3 + 2] = sk; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < NM_SURF_BLOCK / 64; ++v) { si += sh[v * 3]; sj += sh[v * 3 + 1]; sk += sh[v * 3 + 2]; }
        fsum[3 * (size_t)f] = si; fsum[3 * (size_t)f + 1] = sj; fsum[3 * (size_t)f + 2] = sk;
    }
}

struct SurfM { int n, sx, sy, sz, qxx, qxy, qxz, qyy, qyz, qzz; };

// n, S (3), Q (6) of the point (i, j, k).  fb: the frame's words; slab: words [ws, ..) of them in LDS (STAGED).  lut[x], x a 9-bit
// window whose bit u is the voxel at dk = u - 4:  65536 * sum dk + sum dk^2
template <bool STAGED>
__device__ __forceinline__ void surf_moments(const unsigned long long* __restrict__ fb, const unsigned long long* slab, int ws,
                                             const int* lut, int G, int r, int radius2, int i, int j, int k, SurfM& m) {
    int n = 0, sx = 0, sy = 0, sz = 0, qxx = 0, qxy = 0, qxz = 0, qyy = 0, qyz = 0, qzz = 0;
    for (int di = -r; di <= r; ++di) {
        const int ii = i + di;
        if ((unsigned)ii >= (unsigned)G) continue;
        for (int dj = -r; dj <= r; ++dj) {
            const int rem = radius2 - di * di - dj * dj, jj = j + dj;
            if (rem < 0 || (unsigned)jj >= (unsigned)G) continue;
            const int hk = rem >= 16 ? 4 : rem >= 9 ? 3 : rem >= 4 ? 2 : rem >= 1 ? 1 : 0;
            const int lo = k - hk > 0 ? k - hk : 0, hi = k + hk < G - 1 ? k + hk : G - 1, len = hi - lo + 1;        // 1 <= len <= 9
            const unsigned pos = ((unsigned)ii * (unsigned)G + (unsigned)jj) * (unsigned)G + (unsigned)lo;        // pos + len <= G^3
            const int wi = (int)(pos >> 6), sh = (int)(pos & 63u);
            unsigned long long v = (STAGED ? slab[wi - ws] : fb[wi]) >> sh;
            if (sh + len > 64) v |= (STAGED ? slab[wi + 1 - ws] : fb[wi + 1]) << (64 - sh);                      // (the row goes on there)
            const unsigned x = ((unsigned)v & ((1u << len) - 1u)) << (lo - k + 4);
            const int c = __popc(x), e = lut[x], m1 = e >> 16, m2 = e & 0xffff;
            n += c; sx += di * c; sy += dj * c; sz += m1;
            qxx += di * di * c; qxy += di * dj * c; qxz += di * m1; qyy += dj * dj * c; qyz += dj * m1; qzz += m2;
        }
    }
    m.n = n; m.sx = sx; m.sy = sy; m.sz = sz; m.qxx = qxx; m.qxy = qxy; m.qxz = qxz; m.qyy = qyy; m.qyz = qyz; m.qzz = qzz;
}

// one Jacobi rotation that annihilates a[p][q] of a symmetric 3 x 3 matrix (r the third index), applied to the columns p, q of V.
// An element that is exactly zero is left alone.
__device__ __forceinline__ void surf_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                         double& v1p, double& v1q, double& v2p, double& v2q, int sweep) {
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }
    const double h = aqq - app;
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), d = t * apq;
    app -= d; aqq += d; apq = 0.0;
    double a = arp, b = arq;
    arp = a - s * (b + a * tau); arq = b + s * (a - b * tau);
    a = v0p; b = v0q; v0p = a - s * (b + a * tau); v0q = b + s * (a - b * tau);
    a = v1p; b = v1q; v1p = a - s * (b + a * tau); v1q = b + s * (a - b * tau);
    a = v2p; b = v2q; v2p = a - s * (b + a * tau); v2q = b + s * (a - b * tau);
}

// eigenvalues (ascending) of the symmetric matrix and the unit eigenvector of the smallest
__device__ __forceinline__ void surf_eigen(double a00, double a01, double a02, double a11, double a12, double a22, double& e0, double& e1, double& e2,
                                           double& nx, double& ny, double& nz) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        surf_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21, sweep);
        surf_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22, sweep);
        surf_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22, sweep);
    }
    // the smallest: the first of equal ones.  Selected by value, component by component (an indexed column would live in scratch)
    const bool s1 = a11 < a00;
    const double m01 = s1 ? a11 : a00;
    const bool s2 = a22 < m01;
    const double x = s2 ? v02 : s1 ? v01 : v00, y = s2 ? v12 : s1 ? v11 : v10, z = s2 ? v22 : s1 ? v21 : v20;
    const double l0 = s2 ? a22 : m01;
    const double p = s1 ? a00 : a11, q = s2 ? m01 : a22;                     // the other two
    const double l1 = q < p ? q : p, l2 = q < p ? p : q;
    const double len = sqrt(x * x + y * y + z * z);              // (1 up to the rotations' rounding)
    nx = x / len; ny = y / len; nz = z / len;
    e0 = l0; e1 = l1; e2 = l2;
}

// grid F * nC: workgroup f * nC + c takes the points of chunk c of frame f, thread r the chunk's r-th point (occ_write_kernel's search)
__global__ __launch_bounds__(NM_SURF_BLOCK) void surf_kernel(const unsigned long long* __restrict__ bits, const long long* __restrict__ offsets,
                                                             const int32_t* __restrict__ coff, const int32_t* __restrict__ z_idx_range,
                                                             const long long* __restrict__ fsum, int T, int G, int V, int W, int nC, int radius2,
                                                             int r, int orient, const double* __restrict__ orient_point,
                                                             const double* __restrict__ base, const double* __restrict__ add, double shade_a,
                                                             double shade_b, double half, long long capacity, int32_t* __restrict__ moments,
                                                             double* __restrict__ normals, double* __restrict__ spread,
                                                             double* __restrict__ plates, double* __restrict__ colors) {
    __shared__ unsigned long long slab[NM_SURF_SLAB_WORDS];
    __shared__ unsigned long long wsh[NM_OUT_CHUNK_WORDS];
    __shared__ int pre[NM_OUT_CHUNK_WORDS + 1];
    __shared__ int lut[512];
    const int f = blockIdx.x / nC, c = blockIdx.x - f * nC, tid = threadIdx.x;
    const long long row0 = offsets[f] + (long long)coff[blockIdx.x];
    if (row0 >= capacity) return;                                // (the same for the whole workgroup)
    const unsigned long long* fb = bits + (size_t)f * (size_t)W;
    if (tid < NM_OUT_CHUNK_WORDS) {
        const long long w = (long long)c * NM_OUT_CHUNK_WORDS + tid;
        const unsigned long long word = w < (long long)W ? fb[w] : 0ull;
        wsh[tid] = word;
        int incl = __popcll(word);
        for (int off = 1; off < 64; off <<= 1) { const int q = __shfl_up(incl, off); if (tid >= off) incl += q; }
        pre[tid + 1] = incl;
        if (tid == 0) pre[0] = 0;
    }
    for (int x = tid; x < 512; x += NM_SURF_BLOCK) {
        int m1 = 0, m2 = 0;
        for (int u = 0; u < 9; ++u)
            if ((x >> u) & 1) { m1 += u - 4; m2 += (u - 4) * (u - 4); }
        lut[x] = m1 * 65536 + m2;
    }
    __syncthreads();
    const int total = pre[NM_OUT_CHUNK_WORDS];
    if (total == 0) return;
    // the slab: the i-planes of the chunk's voxels and r planes on either side, as whole words [ws, we) of the frame
    const unsigned G2 = (unsigned)G * (unsigned)G;
    const unsigned p_first = (unsigned)c * (NM_OUT_CHUNK_WORDS * 64u);
    const unsigned p_last = p_first + (NM_OUT_CHUNK_WORDS * 64u - 1u) < (unsigned)V - 1u ? p_first + (NM_OUT_CHUNK_WORDS * 64u - 1u) : (unsigned)V - 1u;
    const int i_lo = (int)(p_first / G2), i_hi = (int)(p_last / G2);
    const int pl = i_lo - r > 0 ? i_lo - r : 0, ph = i_hi + r < G - 1 ? i_hi + r : G - 1;
    const int ws = (int)(((unsigned)pl * G2) >> 6), we = (int)((((unsigned)ph + 1u) * G2 + 63u) >> 6);          // we <= W
    const bool staged = we - ws <= NM_SURF_SLAB_WORDS;
    if (staged) {
        for (int w = tid; w < we - ws; w += NM_SURF_BLOCK) slab[w] = fb[ws + w];
        __syncthreads();
    }
    const int b = f / T;
    const bool want_n = normals || spread || plates;
    for (int rk = tid; rk < total; rk += NM_SURF_BLOCK) {
        const long long row = row0 + rk;
        if (row >= capacity) break;
        int wi = 0;
#pragma unroll
        for (int s = NM_OUT_CHUNK_WORDS / 2; s > 0; s >>= 1) wi += pre[wi + s] <= rk ? s : 0;       // the last word with pre[wi] <= rk
        const unsigned long long word = wsh[wi];
        int nb = rk - pre[wi], pos = 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const int below = __popcll((word >> pos) & ((1ull << s) - 1ull));
            if (nb >= below) { nb -= below; pos += s; }
        }
        const unsigned p = ((unsigned)c * NM_OUT_CHUNK_WORDS + (unsigned)wi) * 64u + (unsigned)pos;   // flat voxel of the frame, < G^3
        const unsigned ij = p / (unsigned)G;
        const int k = (int)(p - ij * (unsigned)G), i = (int)(ij / (unsigned)G), j = (int)(ij - (unsigned)i * (unsigned)G);
        SurfM m;
        if (staged) surf_moments<true>(fb, slab, ws, lut, G, r, radius2, i, j, k, m);
        else surf_moments<false>(fb, slab, ws, lut, G, r, radius2, i, j, k, m);
        if (moments) {
            int32_t* o = moments + row * 10;
            o[0] = m.n; o[1] = m.sx; o[2] = m.sy; o[3] = m.sz; o[4] = m.qxx; o[5] = m.qxy; o[6] = m.qxz; o[7] = m.qyy; o[8] = m.qyz; o[9] = m.qzz;
        }
        const double ci = (double)i / half - 1.0, cj = (double)j / half - 1.0, ck = (double)k / half - 1.0;
        if (want_n) {
            const int n = m.n;
            double l0, l1, l2, nx, ny, nz;
            surf_eigen((double)(n * m.qxx - m.sx * m.sx), (double)(n * m.qxy - m.sx * m.sy), (double)(n * m.qxz - m.sx * m.sz),
                       (double)(n * m.qyy - m.sy * m.sy), (double)(n * m.qyz - m.sy * m.sz), (double)(n * m.qzz - m.sz * m.sz), l0, l1, l2, nx, ny, nz);
            if (n < 3) { nx = 0.0; ny = 0.0; nz = 1.0; }
            double dot = 0.0;
            if (!normals && !plates) {
                // spread alone: no normal is written, so none is oriented - orient_point and fsum are not read
            } else if (orient == 0) {
                long long ox = -m.sx, oy = -m.sy, oz = -m.sz;
                if (m.sx == 0 && m.sy == 0 && m.sz == 0) {
                    const long long nf = offsets[f + 1] - offsets[f];
                    ox = nf * i - fsum[3 * (size_t)f]; oy = nf * j - fsum[3 * (size_t)f + 1]; oz = nf * k - fsum[3 * (size_t)f + 2];
                    if (ox == 0 && oy == 0 && oz == 0) ox = oy = oz = 1;
                }
                dot = nx * (double)ox + ny * (double)oy + nz * (double)oz;
            } else {
                const double* op = orient_point + 3 * (size_t)b;
                dot = nx * (op[0] - ci) + ny * (op[1] - cj) + nz * (op[2] - ck);
            }
            if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            if (normals) { double* o = normals + row * 3; o[0] = nx; o[1] = ny; o[2] = nz; }
            if (spread) { double* o = spread + row * 3; o[0] = l0; o[1] = l1; o[2] = l2; }
            if (plates) {                                        // drawPlate, line1 = (0, 0, 1): v = (-l_y, l_x, 0)
                const double den = sqrt(nx * nx + ny * ny + nz * nz) + 1e-6;
                const double lx = nx / den, ly = ny / den, lz = nz / den;
                const double cc = lz + 1e-8, fk = 1.0 / (1.0 + cc);
                const bool anti = fabs(cc + 1.0) < 1e-4;         // the normal points along -z: R = diag(-1, 1, -1)
                double* o = plates + row * 12;
                o[0] = anti ? -1.0 : 1.0 + (-(lx * lx)) * fk; o[1] = anti ? 0.0 : (-(lx * ly)) * fk; o[2] = anti ? 0.0 : lx; o[3] = ci;
                o[4] = anti ? 0.0 : (-(ly * lx)) * fk; o[5] = anti ? 1.0 : 1.0 + (-(ly * ly)) * fk; o[6] = anti ? 0.0 : ly; o[7] = cj;
                o[8] = anti ? 0.0 : -lx; o[9] = anti ? 0.0 : -ly; o[10] = anti ? -1.0 : 1.0 + (-(lx * lx) - ly * ly) * fk; o[11] = ck;
            }
        }
        if (colors) {
            const double zlo = (double)z_idx_range[2 * b] / half - 1.0, zlen = ((double)z_idx_range[2 * b + 1] / half - 1.0) - zlo;
            const double t = (ck - zlo) / zlen * shade_a + shade_b;
            double* o = colors + row * 3;
            const double* bc = base + 3 * (size_t)f;
            if (add) {
                const double* ac = add + 3 * (size_t)f;
                o[0] = bc[0] * t + ac[0]; o[1] = bc[1] * t + ac[1]; o[2] = bc[2] * t + ac[2];
            } else {
                o[0] = bc[0] * t; o[1] = bc[1] * t; o[2] = bc[2] * t;
            }
        }
    }
}

}  // namespace

extern "C" {

int nm_occupied_surface(nm_ctx* c, const uint64_t* bits, const int64_t* offsets, const int32_t* z_idx_range, int32_t B, int32_t T, int32_t G,
                        int32_t radius2, int32_t orient, const double* orient_point, const double* base, const double* add, double shade_a,
                        double shade_b, int64_t capacity, int32_t* moments, double* normals, double* spread, double* plates,
                        double* colors) try { NmScope nm_scope_(c);
    if (radius2 < 1 || radius2 > NM_SURF_MAX_R2) {               // (judged before the context, like nm_ctx_set_const_intensity's value)
        nm_set_error("occupied_surface: radius2 = %d, the call takes 1 .. %d", (int)radius2, NM_SURF_MAX_R2);
        return NM_ERR_ARG;
    }
    if (!c) { nm_set_error("occupied_surface: null ctx"); return NM_ERR_ARG; }
    if (!bits || !offsets || !z_idx_range) { nm_set_error("occupied_surface: null argument"); return NM_ERR_ARG; }
    if (orient != NM_SURF_OUTWARD && orient != NM_SURF_TOWARDS) { nm_set_error("occupied_surface: orient %d", (int)orient); return NM_ERR_ARG; }
    if (orient == NM_SURF_TOWARDS && !orient_point && (normals || plates)) { nm_set_error("occupied_surface: orient 1 without orient_point"); return NM_ERR_ARG; }
    if (colors && !base) { nm_set_error("occupied_surface: colors without base"); return NM_ERR_ARG; }
    if (capacity < 0) { nm_set_error("occupied_surface: capacity %lld", (long long)capacity); return NM_ERR_ARG; }
    NmOutGeom g;
    int rc = nm_out_geom("occupied_surface", B, T, G, &g);
    if (rc) return rc;
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    if (capacity == 0 || (!moments && !normals && !spread && !plates && !colors)) return NM_OK;      // nothing to write
    const size_t nchunks = (size_t)g.F * g.nC, coff_bytes = (nchunks * sizeof(int32_t) + 255) & ~(size_t)255, fsum_bytes = 3 * (size_t)g.F * sizeof(long long);
    if ((rc = nm_ctx_reserve(c, coff_bytes + fsum_bytes + 4096))) return rc;
    c->ws.release(0);
    int32_t* coff = static_cast<int32_t*>(c->ws.alloc_bytes(coff_bytes));
    long long* fsum = static_cast<long long*>(c->ws.alloc_bytes(fsum_bytes));
    if (!coff || !fsum) { nm_set_error("occupied_surface: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(bits);
    nm_out_launch_chunk_scan(s, words, g, coff);
    const bool outward = orient == NM_SURF_OUTWARD && (normals || plates);
    if (outward) hipLaunchKernelGGL(surf_frame_sum_kernel, dim3((unsigned)g.F), dim3(NM_SURF_BLOCK), 0, s, words, (int)G, g.W, fsum);
    int r = 1;
    while ((r + 1) * (r + 1) <= radius2) ++r;
    hipLaunchKernelGGL(surf_kernel, dim3((unsigned)nchunks), dim3(NM_SURF_BLOCK), 0, s, words, reinterpret_cast<const long long*>(offsets),
                       (const int32_t*)coff, z_idx_range, (const long long*)fsum, (int)T, (int)G, g.V, g.W, g.nC, (int)radius2, r, (int)orient,
                       orient_point, base, add, shade_a, shade_b, (double)(G - 1) / 2.0, (long long)capacity, moments, normals, spread, plates,
                       colors);
    return nm_check_hip(hipGetLastError(), "occupied_surface launch");
} catch (...) { return nm_abi_catch("nm_occupied_surface"); }

}  // extern "C"
