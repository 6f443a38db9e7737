// Device render path for the retargeting demo (vis_retarget.py:400-557 of the reference): the posed triangle mesh and the skeleton -
// a sphere per visible joint, a double cone per bone - drawn through the plate renderer's pinhole camera, and the skeleton pasted over
// the mesh.  The script does this with open3d's off-screen GL visualiser on the host.
//
// As for the plates this is NOT open3d's image.  The contract is the library's own, written out in include/nm355.h and restated in
// float64 numpy in tests/mesh_ref.py; in short, per pixel (px, py), d = ((px - cx) / fx, (py - cy) / fy, 1):
//   triangle  p'_k = E p_k, n = (p'_1 - p'_0) x (p'_2 - p'_0), q = n . p'_0, X_k = p'_kx / p'_kz, Y_k = p'_ky / p'_kz, iz_k = 1 / p'_kz
//             w0 = (X1 - dx) * (Y2 - dy) - (Y1 - dy) * (X2 - dx), w1, w2 by rotation; covered iff all >= 0 or all <= 0, their sum is
//             not 0 and the pixel lies in the triangle's rectangle;  den = (n_x dx + n_y dy) + n_z, s = q / den >= near
//   sphere    A = (dx^2 + dy^2) + 1, B = d . c', C = |c'|^2 - r^2, D = B B - A C >= 0 and B > 0: s = C / (B + sqrt(D))
//   nappe     apex a, axis v (apex -> base centre), kappa = (v.v + rb^2) / (v.v)^2: kappa ((X - a) . v)^2 = |X - a|^2 along X = s d is
//             c2 s^2 - 2 c1 s + c0 = 0; the nearer root whose (X - a) . v lies in [0, v.v], decided without a square root
//   the winner is the hit of the smallest s, the lowest triangle row / primitive number among equal s
// (the library is built with -ffp-contract=off: every line is numpy's operation order, unfused.)
//
// The mesh is the plates' tiled gather, no atomics on the result:
//   transform  a lane per (frame, triangle): the record, and a pixel rectangle that contains every pixel the triangle can cover
//   tiles      a lane per (frame, triangle) adds one to the count of every (frame, 16 x 16 tile) its rectangle touches; the plates' scan
//              (nm_tiles.h) gives the tile offsets; nm_mesh_draw's fill pass writes the record rows into the tile lists
//   draw       a workgroup per tile, a thread per pixel: the tile's triangles go through LDS NM_MESH_CHUNK at a time, every thread keeps
//              its own (s, row) minimum in registers, fetches the winner's vertex colours and writes its pixel once
//   shade      (nm_mesh_shade, optional) a thread per pixel shades the winner in `index` again, with interpolated vertex normals
// The skeleton is one launch, a workgroup per tile: its first K threads transform the frame's joints and bones into LDS (at most 32
// spheres and 31 bones), then every thread tests its pixel against those whose rectangle holds it.
#include "nm_ctx.h"
#include "nm_mesh.h"
#include "nm_tiles.h"
#include <cmath>

namespace {

// p' = E p in the plates' operation order
__device__ __forceinline__ void mesh_to_camera(const double* e, double x, double y, double z, double& tx, double& ty, double& tz) {
    tx = ((e[0] * x + e[1] * y) + e[2] * z) + e[3];
    ty = ((e[4] * x + e[5] * y) + e[6] * z) + e[7];
    tz = ((e[8] * x + e[9] * y) + e[10] * z) + e[11];
}

// pixel bounds umin .. umax, vmin .. vmax (doubles, either order of a NaN taking the conservative side) -> x0, x1, y0, y1 clamped to the
// image; x0 > x1: no pixel
__device__ __forceinline__ void mesh_clamp_rect(const RenderCam& cam, double umin, double umax, double vmin, double vmax, int* r) {
    int x0 = umin > 0.0 ? (umin < (double)cam.W ? (int)floor(umin) : cam.W) : 0;
    int x1 = umax < (double)(cam.W - 1) ? (umax >= 0.0 ? (int)ceil(umax) : -1) : cam.W - 1;
    int y0 = vmin > 0.0 ? (vmin < (double)cam.H ? (int)floor(vmin) : cam.H) : 0;
    int y1 = vmax < (double)(cam.H - 1) ? (vmax >= 0.0 ? (int)ceil(vmax) : -1) : cam.H - 1;
    if (x0 > x1 || y0 > y1) { x0 = 0; x1 = -1; y0 = 0; y1 = -1; }
    r[0] = x0; r[1] = x1; r[2] = y0; r[3] = y1;
}

// grid ceil(F M / 256): rec[i] and rect[i] of record i = f M + m
__global__ __launch_bounds__(NM_RENDER_BLOCK) void mesh_transform_kernel(const double* __restrict__ vertices, const int* __restrict__ triangles, int V,
                                                                          long long M, long long rows, RenderCam cam, double* __restrict__ rec,
                                                                          int* __restrict__ rect) {
    const long long i = (long long)blockIdx.x * NM_RENDER_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const long long f = i / M, m = i - f * M;
    const int t0 = triangles[m * 3], t1 = triangles[m * 3 + 1], t2 = triangles[m * 3 + 2];
    double o[NM_MESH_REC];
#pragma unroll
    for (int u = 0; u < NM_MESH_REC; ++u) o[u] = 0.0;
    int r[4] = {0, -1, 0, -1};
    if (t0 >= 0 && t0 < V && t1 >= 0 && t1 < V && t2 >= 0 && t2 < V) {     // (an index outside the vertices: not drawn, nothing is read)
        const double* v0 = vertices + ((size_t)f * (size_t)V + (size_t)t0) * 3;
        const double* v1 = vertices + ((size_t)f * (size_t)V + (size_t)t1) * 3;
        const double* v2 = vertices + ((size_t)f * (size_t)V + (size_t)t2) * 3;
        double ax, ay, az, bx, by, bz, cx, cy, cz;
        mesh_to_camera(cam.e, v0[0], v0[1], v0[2], ax, ay, az);
        mesh_to_camera(cam.e, v1[0], v1[1], v1[2], bx, by, bz);
        mesh_to_camera(cam.e, v2[0], v2[1], v2[2], cx, cy, cz);
        const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) && isfinite(cy) &&
                            isfinite(cz);
        if (finite && !(az < cam.near) && !(bz < cam.near) && !(cz < cam.near)) {
            const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const double q = (nx * ax + ny * ay) + nz * az;
            if (isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(q) && !(nx == 0.0 && ny == 0.0 && nz == 0.0)) {
                o[0] = ax / az; o[1] = ay / az; o[2] = bx / bz; o[3] = by / bz; o[4] = cx / cz; o[5] = cy / cz;
                o[6] = nx; o[7] = ny; o[8] = nz; o[9] = q;
                o[10] = 1.0 / az; o[11] = 1.0 / bz; o[12] = 1.0 / cz;
                // The contract's rectangle: floor(min u - 1) .. ceil(max u + 1) in pixels, the same in y.  A covered pixel of a triangle
                // with area lies inside the projected triangle or within ulps of an edge, far inside that rectangle; it is part of the
                // contract for the edge-on triangle, whose edge functions are rounding noise all along its line.
                const double u0 = cam.cx + cam.fx * o[0], u1 = cam.cx + cam.fx * o[2], u2 = cam.cx + cam.fx * o[4];
                const double w0 = cam.cy + cam.fy * o[1], w1 = cam.cy + cam.fy * o[3], w2 = cam.cy + cam.fy * o[5];
                const double umin = fmin(u0, fmin(u1, u2)) - 1.0, umax = fmax(u0, fmax(u1, u2)) + 1.0;
                const double vmin = fmin(w0, fmin(w1, w2)) - 1.0, vmax = fmax(w0, fmax(w1, w2)) + 1.0;
                mesh_clamp_rect(cam, umin, umax, vmin, vmax, r);
            }
        }
    }
    double* dst = rec + i * NM_MESH_REC;
#pragma unroll
    for (int u = 0; u < NM_MESH_REC; ++u) dst[u] = o[u];
    int* rr = rect + i * 4;
    rr[0] = r[0]; rr[1] = r[1]; rr[2] = r[2]; rr[3] = r[3];
}

// grid ceil(F M / 256).  FILL false: counts[tile] += 1 for every tile of the record's rectangle; true: the record's row goes into each of
// those tiles' lists, at tile_offsets[tile] + (the tile's cursor), where that is below the capacity
template <bool FILL>
__global__ __launch_bounds__(NM_RENDER_BLOCK) void mesh_tiles_kernel(const int* __restrict__ rect, long long M, long long rows, int TX, int TY,
                                                                      int* __restrict__ counts, const long long* __restrict__ tile_offsets,
                                                                      long long capacity, int* __restrict__ list) {
    const long long i = (long long)blockIdx.x * NM_RENDER_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const int* r = rect + i * 4;
    const int x0 = r[0], x1 = r[1], y0 = r[2], y1 = r[3];
    if (x0 > x1 || y0 > y1 || x0 < 0 || y0 < 0) return;
    const long long f = i / M;
    const int tx1 = (x1 >> 4) < TX - 1 ? (x1 >> 4) : TX - 1, ty1 = (y1 >> 4) < TY - 1 ? (y1 >> 4) : TY - 1;
    for (int ty = y0 >> 4; ty <= ty1; ++ty)
        for (int tx = x0 >> 4; tx <= tx1; ++tx) {
            const size_t t = ((size_t)f * TY + ty) * TX + tx;
            const int k = atomicAdd(&counts[t], 1);
            if (FILL) {
                const long long pos = tile_offsets[t] + (long long)k;
                if (pos >= 0 && pos < capacity) list[pos] = (int)i;
            }
        }
}

__device__ __forceinline__ unsigned char mesh_byte(double v) {
    if (v != v) v = 0.0;
    v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
    return (unsigned char)(int)(v * 255.0);
}

struct MeshShade {
    double light_a, light_b;
    double color[3];                  // the uniform colour (without vertex colours)
    int bg[3];
};

// grid F * TY * TX: workgroup t draws tile (tx, ty) of frame f, thread (lx, ly) = (tid & 15, tid >> 4) its pixel
__global__ __launch_bounds__(NM_RENDER_BLOCK) void mesh_draw_kernel(const double* __restrict__ rec, const int* __restrict__ rect, const int* __restrict__ triangles,
                                                                     const double* __restrict__ vertex_colors, const long long* __restrict__ tile_offsets,
                                                                     const int* __restrict__ list, long long M, long long rows, long long capacity,
                                                                     RenderCam cam, MeshShade sh, int* __restrict__ index, double* __restrict__ depth,
                                                                     unsigned char* __restrict__ image) {
    __shared__ double sh_rec[NM_MESH_CHUNK][NM_MESH_STAGED];
    __shared__ int sh_idx[NM_MESH_CHUNK];
    __shared__ unsigned sh_box[NM_MESH_CHUNK];
    const int tid = threadIdx.x, lx = tid & (NM_RENDER_TILE - 1), ly = tid >> 4;
    const unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)cam.TX), ty = (int)((t / (unsigned)cam.TX) % (unsigned)cam.TY), f = (int)(t / ((unsigned)cam.TX * (unsigned)cam.TY));
    const int px = tx * NM_RENDER_TILE + lx, py = ty * NM_RENDER_TILE + ly;
    const bool valid = px < cam.W && py < cam.H;                 // (tiles on the right and bottom edges are partial)
    const double dx = ((double)px - cam.cx) / cam.fx, dy = ((double)py - cam.cy) / cam.fy;
    long long lo = tile_offsets[t], hi = tile_offsets[t + 1];
    if (lo < 0) lo = 0;
    if (hi > capacity) hi = capacity;                            // (a list cut by the capacity: the image is incomplete, nothing is read past it)
    double best_s = INFINITY, best_den = 0.0, best_w0 = 0.0, best_w1 = 0.0, best_w2 = 0.0;
    int best_i = -1;
    for (long long base = lo; base < hi; base += NM_MESH_CHUNK) {
        const int n = hi - base < (long long)NM_MESH_CHUNK ? (int)(hi - base) : NM_MESH_CHUNK;
        __syncthreads();                                         // the previous chunk has been read
        if (tid < n) {
            const int j = tid;
            const int i = list[base + j];
            unsigned box = 15u | (15u << 8);                     // x0 = 15 > x1 = 0: no pixel (an entry that is no row)
            if (i >= 0 && (long long)i < rows) {
                const double* s = rec + (size_t)i * NM_MESH_REC;
#pragma unroll
                for (int u = 0; u < NM_MESH_STAGED; ++u) sh_rec[j][u] = s[u];
                const int* r = rect + (size_t)i * 4;
                const int a0 = r[0] - tx * NM_RENDER_TILE, a1 = r[1] - tx * NM_RENDER_TILE, b0 = r[2] - ty * NM_RENDER_TILE, b1 = r[3] - ty * NM_RENDER_TILE;
                const unsigned x0 = a0 < 0 ? 0 : a0 > 15 ? 15 : a0, x1 = a1 < 0 ? 0 : a1 > 15 ? 15 : a1;
                const unsigned y0 = b0 < 0 ? 0 : b0 > 15 ? 15 : b0, y1 = b1 < 0 ? 0 : b1 > 15 ? 15 : b1;
                box = x0 | (x1 << 4) | (y0 << 8) | (y1 << 12);
                if (a1 < 0 || a0 > 15 || b1 < 0 || b0 > 15) box = 15u | (15u << 8);       // (a record of another tile: no pixel)
            }
            sh_idx[j] = i;
            sh_box[j] = box;
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < n; ++j) {
                const unsigned box = sh_box[j];
                if ((unsigned)lx < (box & 15u) || (unsigned)lx > ((box >> 4) & 15u) || (unsigned)ly < ((box >> 8) & 15u) || (unsigned)ly > ((box >> 12) & 15u))
                    continue;                                    // outside the triangle's rectangle: not covered
                const double* r = sh_rec[j];
                const double a0 = r[0] - dx, b0 = r[1] - dy, a1 = r[2] - dx, b1 = r[3] - dy, a2 = r[4] - dx, b2 = r[5] - dy;
                const double w0 = a1 * b2 - b1 * a2, w1 = a2 * b0 - b2 * a0, w2 = a0 * b1 - b0 * a1;
                const bool pos = w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0, neg = w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0;
                if (!(pos || neg)) continue;
                if ((w0 + w1) + w2 == 0.0) continue;
                const double den = (r[6] * dx + r[7] * dy) + r[8];
                if (den == 0.0) continue;
                const double s = r[9] / den;
                if (!(s >= cam.near)) continue;
                const int i = sh_idx[j];
                if (s < best_s || (s == best_s && i < best_i)) { best_s = s; best_i = i; best_den = den; best_w0 = w0; best_w1 = w1; best_w2 = w2; }
            }
        }
    }
    if (!valid) return;
    const size_t o = ((size_t)f * (size_t)cam.H + (size_t)py) * (size_t)cam.W + (size_t)px;
    const long long m = best_i < 0 ? -1 : (long long)best_i - (long long)f * M;
    if (index) index[o] = (int)m;
    if (depth) depth[o] = best_s;
    if (image) {
        unsigned char* im = image + o * 3;
        if (best_i < 0) {
            im[0] = (unsigned char)sh.bg[0]; im[1] = (unsigned char)sh.bg[1]; im[2] = (unsigned char)sh.bg[2];
        } else {
            const double* r = rec + (size_t)best_i * NM_MESH_REC;
            const double nx = r[6], ny = r[7], nz = r[8];
            const double nn = (nx * nx + ny * ny) + nz * nz;
            const double shade = sh.light_a + sh.light_b * fabs(best_den) / (sqrt(nn) * sqrt((dx * dx + dy * dy) + 1.0));
            double c[3] = {sh.color[0], sh.color[1], sh.color[2]};
            if (vertex_colors) {                                 // (the winner was drawn: its three indices are inside the vertices)
                const int* tri = triangles + (size_t)m * 3;
                const double* c0 = vertex_colors + (size_t)tri[0] * 3;
                const double* c1 = vertex_colors + (size_t)tri[1] * 3;
                const double* c2 = vertex_colors + (size_t)tri[2] * 3;
                const double l0 = best_w0 * r[10], l1 = best_w1 * r[11], l2 = best_w2 * r[12];
                const double L = (l0 + l1) + l2;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = ((l0 * c0[ch] + l1 * c1[ch]) + l2 * c2[ch]) / L;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) im[ch] = mesh_byte(c[ch] * shade);
        }
    }
}

// The deferred smooth-shading pass.  grid ceil(F H W / 256), a thread per pixel: the winner mesh_draw_kernel left in index is shaded again
// with the perspective-correct mix of its three vertex normals (nm_vertex_normals' rows) instead of the record's flat n.  a_k, b_k, w_k, l_k
// and L are recomputed from the record exactly as the draw computes them, so the colour mix is the draw's to the bit.  An index outside
// [0, M) or a winner with a vertex outside [0, V) takes the background: nothing is read through either.
__global__ __launch_bounds__(NM_RENDER_BLOCK) void mesh_shade_kernel(const double* __restrict__ rec, const int* __restrict__ index, const int* __restrict__ triangles,
                                                                      const double* __restrict__ normals, const double* __restrict__ vertex_colors, int V,
                                                                      long long M, long long pixels, RenderCam cam, MeshShade sh, unsigned char* __restrict__ image) {
    const long long o = (long long)blockIdx.x * NM_RENDER_BLOCK + threadIdx.x;
    if (o >= pixels) return;
    const long long hw = (long long)cam.H * cam.W;
    const long long f = o / hw, rem = o - f * hw;
    const int py = (int)(rem / cam.W), px = (int)(rem - (long long)py * cam.W);
    unsigned char* im = image + (size_t)o * 3;
    const long long m = index[o];
    int t0 = -1, t1 = -1, t2 = -1;
    if (m >= 0 && m < M) { const int* tri = triangles + (size_t)m * 3; t0 = tri[0]; t1 = tri[1]; t2 = tri[2]; }
    if (!(t0 >= 0 && t0 < V && t1 >= 0 && t1 < V && t2 >= 0 && t2 < V)) {
        im[0] = (unsigned char)sh.bg[0]; im[1] = (unsigned char)sh.bg[1]; im[2] = (unsigned char)sh.bg[2];
        return;
    }
    const double dx = ((double)px - cam.cx) / cam.fx, dy = ((double)py - cam.cy) / cam.fy;
    const double* r = rec + ((size_t)f * (size_t)M + (size_t)m) * NM_MESH_REC;
    const double a0 = r[0] - dx, b0 = r[1] - dy, a1 = r[2] - dx, b1 = r[3] - dy, a2 = r[4] - dx, b2 = r[5] - dy;
    const double w0 = a1 * b2 - b1 * a2, w1 = a2 * b0 - b2 * a0, w2 = a0 * b1 - b0 * a1;
    const double l0 = w0 * r[10], l1 = w1 * r[11], l2 = w2 * r[12];
    const double L = (l0 + l1) + l2;
    const double A = (dx * dx + dy * dy) + 1.0;
    const double* n0 = normals + ((size_t)f * (size_t)V + (size_t)t0) * 3;
    const double* n1 = normals + ((size_t)f * (size_t)V + (size_t)t1) * 3;
    const double* n2 = normals + ((size_t)f * (size_t)V + (size_t)t2) * 3;
    double h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                    // n' = (E[k,0] n_x + E[k,1] n_y) + E[k,2] n_z: a direction, no translation
        const double* e = cam.e + 4 * k;
        const double c0 = (e[0] * n0[0] + e[1] * n0[1]) + e[2] * n0[2];
        const double c1 = (e[0] * n1[0] + e[1] * n1[1]) + e[2] * n1[2];
        const double c2 = (e[0] * n2[0] + e[1] * n2[1]) + e[2] * n2[2];
        h[k] = ((l0 * c0 + l1 * c1) + l2 * c2) / L;
    }
    const double hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    double shade;
    if (hh == 0.0 || !isfinite(hh)) {                                // no usable normal there: the draw's flat shade
        const double den = (r[6] * dx + r[7] * dy) + r[8];
        const double nn = (r[6] * r[6] + r[7] * r[7]) + r[8] * r[8];
        shade = sh.light_a + sh.light_b * fabs(den) / (sqrt(nn) * sqrt(A));
    } else {
        const double hd = (h[0] * dx + h[1] * dy) + h[2];
        shade = sh.light_a + sh.light_b * fabs(hd) / (sqrt(hh) * sqrt(A));
    }
    double c[3] = {sh.color[0], sh.color[1], sh.color[2]};
    if (vertex_colors) {
        const double* c0 = vertex_colors + (size_t)t0 * 3;
        const double* c1 = vertex_colors + (size_t)t1 * 3;
        const double* c2 = vertex_colors + (size_t)t2 * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ((l0 * c0[ch] + l1 * c1[ch]) + l2 * c2[ch]) / L;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) im[ch] = mesh_byte(c[ch] * shade);
}

// ---- skeleton ------------------------------------------------------------------------------------------------------------------------
struct SkelArgs {
    double threshold, radius, bone_radius, light_a, light_b;
    double joint_color[3], bone_color[3];
    int bg[3];
    int K, overlay;
};

constexpr int NM_SKEL_NAPPE = 10;                                // doubles per nappe: apex a (3), axis v (3), v.v, kappa, a.v, a.a

// the plates' rectangle for the ball of `radius` about (tx, ty, tz) with tz - radius >= near: it contains every pixel whose ray meets it
__device__ void skel_ball_rect(const RenderCam& cam, double tx, double ty, double tz, double radius, int* r) {
    const double rb = radius * (1.0 + 1e-9) + 1e-12 * (((tx * tx + ty * ty) + tz * tz) / radius);
    const double zn = tz - rb > cam.near ? tz - rb : cam.near, zf = tz + rb;
    const double xl = tx - rb, xh = tx + rb, yl = ty - rb, yh = ty + rb;
    const double ua = cam.cx + cam.fx * (xl / (xl >= 0.0 ? zf : zn)), ub = cam.cx + cam.fx * (xh / (xh >= 0.0 ? zn : zf));
    const double va = cam.cy + cam.fy * (yl / (yl >= 0.0 ? zf : zn)), vb = cam.cy + cam.fy * (yh / (yh >= 0.0 ? zn : zf));
    mesh_clamp_rect(cam, (ua < ub ? ua : ub) - 1.0, (ua < ub ? ub : ua) + 1.0, (va < vb ? va : vb) - 1.0, (va < vb ? vb : va) + 1.0, r);
}

// the nappe with apex a and base centre b, base radius rb; false: a degenerate one
__device__ bool skel_nappe(const double* a, const double* b, double rb, double* o) {
    const double vx = b[0] - a[0], vy = b[1] - a[1], vz = b[2] - a[2];
    const double vv = (vx * vx + vy * vy) + vz * vz;
    const double kappa = (vv + rb * rb) / (vv * vv);
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = vx; o[4] = vy; o[5] = vz; o[6] = vv; o[7] = kappa;
    o[8] = (a[0] * vx + a[1] * vy) + a[2] * vz;
    o[9] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    return vv > 0.0 && isfinite(kappa);
}

// P + Q sqrt(D) >= 0 for D >= 0, without the square root
__device__ __forceinline__ bool skel_ge0(double P, double Q, double D) {
    if (Q >= 0.0) return P >= 0.0 ? true : (Q * Q) * D >= P * P;
    return P < 0.0 ? false : P * P >= (Q * Q) * D;
}

// the ray s d against one nappe: the nearer root of c2 s^2 - 2 c1 s + c0 = 0 whose axis parameter lies in [0, v.v]
__device__ __forceinline__ bool skel_nappe_hit(const double* o, double dx, double dy, double A, double& s, double& nx, double& ny, double& nz) {
    const double ax = o[0], ay = o[1], az = o[2], vx = o[3], vy = o[4], vz = o[5], vv = o[6], kappa = o[7], av = o[8], aa = o[9];
    const double dv = (dx * vx + dy * vy) + vz, da = (dx * ax + dy * ay) + az;
    const double kd = kappa * dv;
    const double c2 = kd * dv - A, c1 = kd * av - da, c0 = (kappa * av) * av - aa;
    if (c2 == 0.0) return false;
    const double D = c1 * c1 - c2 * c0;
    if (!(D >= 0.0)) return false;
    const double P = c1 * dv - av * c2, P2 = P - vv * c2;
    // the root (c1 + g sqrt(D)) / c2, g = +-1, has (X - a) . v = (P + g dv sqrt(D)) / c2; the nearer root is g = -1 for c2 > 0, +1 otherwise
    const bool up = c2 > 0.0;
    double Q = up ? -dv : dv;
    bool plus = !up;
    bool in = up ? (skel_ge0(P, Q, D) && skel_ge0(-P2, -Q, D)) : (skel_ge0(-P, -Q, D) && skel_ge0(P2, Q, D));
    if (!in) {
        Q = -Q;
        plus = !plus;
        in = up ? (skel_ge0(P, Q, D) && skel_ge0(-P2, -Q, D)) : (skel_ge0(-P, -Q, D) && skel_ge0(P2, Q, D));
        if (!in) return false;
    }
    const double r = sqrt(D);
    const double qq = c1 + (c1 >= 0.0 ? r : -r);                 // (no cancellation: the roots are qq / c2 and c0 / qq)
    if (qq == 0.0) return false;
    s = (plus == (c1 >= 0.0)) ? qq / c2 : c0 / qq;
    const double km = kappa * (s * dv - av);
    nx = (s * dx - ax) - km * vx; ny = (s * dy - ay) - km * vy; nz = (s - az) - km * vz;
    return true;
}

// grid F * TY * TX, a workgroup per tile of a frame
__global__ __launch_bounds__(NM_RENDER_BLOCK) void skeleton_draw_kernel(const float* __restrict__ keypoints, const int* __restrict__ parents,
                                                                         const double* __restrict__ joint_colors, RenderCam cam, SkelArgs a,
                                                                         int* __restrict__ index, double* __restrict__ depth, unsigned char* __restrict__ image) {
    __shared__ double sh_joint[NM_SKEL_MAXK][4];                 // p', visible (1 / 0)
    __shared__ double sh_sphere[NM_SKEL_MAXK][4];                // c', C
    __shared__ double sh_bone[NM_SKEL_MAXK][2 * NM_SKEL_NAPPE];
    __shared__ int sh_rect[2 * NM_SKEL_MAXK][4];                 // spheres 0 .. K-1, bones K .. 2K-1
    const int tid = threadIdx.x, lx = tid & (NM_RENDER_TILE - 1), ly = tid >> 4, K = a.K;
    const unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)cam.TX), ty = (int)((t / (unsigned)cam.TX) % (unsigned)cam.TY), f = (int)(t / ((unsigned)cam.TX * (unsigned)cam.TY));
    if (tid < K) {
        const float* kp = keypoints + ((size_t)f * K + tid) * 4;
        double x, y, z;
        mesh_to_camera(cam.e, (double)kp[0], (double)kp[1], (double)kp[2], x, y, z);
        double al = (double)kp[3];
        al = al < 0.0 ? 0.0 : al > 1.0 ? 1.0 : al;               // (a NaN stays one and is not visible)
        sh_joint[tid][0] = x; sh_joint[tid][1] = y; sh_joint[tid][2] = z;
        sh_joint[tid][3] = (al >= a.threshold && isfinite(x) && isfinite(y) && isfinite(z)) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < K) {
        const double* c = sh_joint[tid];
        int* rs = sh_rect[tid];
        int* rb = sh_rect[K + tid];
        rs[0] = 0; rs[1] = -1; rs[2] = 0; rs[3] = -1;
        rb[0] = 0; rb[1] = -1; rb[2] = 0; rb[3] = -1;
        if (c[3] != 0.0 && !(c[2] - a.radius < cam.near)) {
            sh_sphere[tid][0] = c[0]; sh_sphere[tid][1] = c[1]; sh_sphere[tid][2] = c[2];
            sh_sphere[tid][3] = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) - a.radius * a.radius;
            skel_ball_rect(cam, c[0], c[1], c[2], a.radius, rs);
        }
        const int p = parents[tid];
        if (c[3] != 0.0 && p >= 0 && p < K && p != tid && sh_joint[p][3] != 0.0) {
            const double* pa = sh_joint[p];
            const double bx = c[0] - pa[0], by = c[1] - pa[1], bz = c[2] - pa[2];
            const double bb = (bx * bx + by * by) + bz * bz;
            if (bb > 0.0 && isfinite(bb) && !(c[2] - a.bone_radius < cam.near) && !(pa[2] - a.bone_radius < cam.near)) {
                const double base[3] = {pa[0] + 0.2 * bx, pa[1] + 0.2 * by, pa[2] + 0.2 * bz};
                const bool ok1 = skel_nappe(pa, base, a.bone_radius, sh_bone[tid]);
                const bool ok2 = skel_nappe(c, base, a.bone_radius, sh_bone[tid] + NM_SKEL_NAPPE);
                if (ok1 && ok2) {
                    // every point of the double cone is within bone_radius of the segment: inside the ball about its middle
                    const double mx = 0.5 * (c[0] + pa[0]), my = 0.5 * (c[1] + pa[1]), mz = 0.5 * (c[2] + pa[2]);
                    const double reach = 0.5 * sqrt(bb) * (1.0 + 1e-9) + a.bone_radius;
                    if (mz - reach < cam.near) {                 // (the ball crosses the near plane though the bone does not: every pixel)
                        rb[0] = 0; rb[1] = cam.W - 1; rb[2] = 0; rb[3] = cam.H - 1;
                    } else {
                        skel_ball_rect(cam, mx, my, mz, reach, rb);
                    }
                }
            }
        }
    }
    __syncthreads();
    const int px = tx * NM_RENDER_TILE + lx, py = ty * NM_RENDER_TILE + ly;
    if (!(px < cam.W && py < cam.H)) return;
    const double dx = ((double)px - cam.cx) / cam.fx, dy = ((double)py - cam.cy) / cam.fy;
    const double A = (dx * dx + dy * dy) + 1.0;
    double best_s = INFINITY, best_nx = 0.0, best_ny = 0.0, best_nz = 0.0;
    int best_i = -1;
    for (int k = 0; k < K; ++k) {
        const int* r = sh_rect[k];
        if (px < r[0] || px > r[1] || py < r[2] || py > r[3]) continue;
        const double cx = sh_sphere[k][0], cy = sh_sphere[k][1], cz = sh_sphere[k][2];
        const double B = (dx * cx + dy * cy) + cz;
        const double D = B * B - A * sh_sphere[k][3];
        if (!(D >= 0.0) || !(B > 0.0)) continue;
        const double s = sh_sphere[k][3] / (B + sqrt(D));
        if (s < best_s) { best_s = s; best_i = k; best_nx = s * dx - cx; best_ny = s * dy - cy; best_nz = s - cz; }
    }
    for (int k = 0; k < K; ++k) {
        const int* r = sh_rect[K + k];
        if (px < r[0] || px > r[1] || py < r[2] || py > r[3]) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double s, nx, ny, nz;
            if (skel_nappe_hit(sh_bone[k] + h * NM_SKEL_NAPPE, dx, dy, A, s, nx, ny, nz) && s < best_s) {
                best_s = s; best_i = K + k; best_nx = nx; best_ny = ny; best_nz = nz;
            }
        }
    }
    const size_t o = ((size_t)f * (size_t)cam.H + (size_t)py) * (size_t)cam.W + (size_t)px;
    if (index) index[o] = best_i;
    if (depth) depth[o] = best_s;
    if (image) {
        unsigned char* im = image + o * 3;
        if (best_i < 0) {
            if (!a.overlay) { im[0] = (unsigned char)a.bg[0]; im[1] = (unsigned char)a.bg[1]; im[2] = (unsigned char)a.bg[2]; }
        } else {
            const double den = (best_nx * dx + best_ny * dy) + best_nz;
            const double nn = (best_nx * best_nx + best_ny * best_ny) + best_nz * best_nz;
            const double shade = a.light_a + a.light_b * fabs(den) / (sqrt(nn) * sqrt(A));
            const double* c = best_i >= K ? a.bone_color : joint_colors ? joint_colors + (size_t)best_i * 3 : a.joint_color;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) im[ch] = mesh_byte(c[ch] * shade);
        }
    }
}

// the camera and the sizes every entry point shares; on success cam holds the kernels' copy and *nt the number of (frame, tile) pairs
int mesh_check(const char* who, const nm_ctx* c, int32_t F, const nm_camera* camera, RenderCam* cam, long long* nt) {
    if (!c) { nm_set_error("%s: null ctx", who); return NM_ERR_ARG; }
    if (!camera) { nm_set_error("%s: null camera", who); return NM_ERR_ARG; }
    if (F < 1 || camera->width < 1 || camera->height < 1) {
        nm_set_error("%s: F = %d frames of %d x %d pixels", who, (int)F, (int)camera->width, (int)camera->height);
        return NM_ERR_ARG;
    }
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(camera->extrinsic[k])) { nm_set_error("%s: extrinsic[%d] is not finite", who, k); return NM_ERR_ARG; }
    if (!std::isfinite(camera->fx) || !std::isfinite(camera->fy) || camera->fx == 0.0 || camera->fy == 0.0 || !std::isfinite(camera->cx) ||
        !std::isfinite(camera->cy) || !std::isfinite(camera->near) || !(camera->near > 0.0)) {
        nm_set_error("%s: camera fx %g fy %g cx %g cy %g near %g (finite, fx and fy not 0, near > 0)", who, camera->fx, camera->fy, camera->cx, camera->cy, camera->near);
        return NM_ERR_ARG;
    }
    if ((long long)F * camera->height * camera->width >= (1ll << 31)) {
        nm_set_error("%s: %d frames of %d x %d pixels, one call indexes fewer than 2^31", who, (int)F, (int)camera->width, (int)camera->height);
        return NM_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < 12; ++k) cam->e[k] = camera->extrinsic[k];
    cam->fx = camera->fx; cam->fy = camera->fy; cam->cx = camera->cx; cam->cy = camera->cy; cam->near = camera->near;
    cam->W = camera->width; cam->H = camera->height;
    cam->TX = (cam->W + NM_RENDER_TILE - 1) / NM_RENDER_TILE; cam->TY = (cam->H + NM_RENDER_TILE - 1) / NM_RENDER_TILE;
    *nt = (long long)F * cam->TX * cam->TY;
    return NM_OK;
}

int mesh_sizes(const char* who, int32_t F, int32_t V, int64_t M) {
    if (V < 1 || M < 0) { nm_set_error("%s: V = %d vertices, M = %lld triangles", who, (int)V, (long long)M); return NM_ERR_ARG; }
    if ((long long)F * M >= (1ll << 31)) {
        nm_set_error("%s: %d frames of %lld triangles, the lists hold 32-bit record rows", who, (int)F, (long long)M);
        return NM_ERR_UNSUPPORTED;
    }
    return NM_OK;
}

int mesh_host_byte(double v) {
    if (v != v) v = 0.0;
    v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
    return (int)(v * 255.0);
}

}  // namespace

extern "C" {

int nm_mesh_bin(nm_ctx* c, const double* vertices, const int32_t* triangles, int32_t F, int32_t V, int64_t M, const nm_camera* camera, double* rec,
                int32_t* rect, int64_t* tile_offsets) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = mesh_check("mesh_bin", c, F, camera, &cam, &nt);
    if (rc) return rc;
    if ((rc = mesh_sizes("mesh_bin", F, V, M))) return rc;
    if (!tile_offsets || (M > 0 && (!vertices || !triangles || !rec || !rect))) { nm_set_error("mesh_bin: null argument"); return NM_ERR_ARG; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    const long long nblk = (nt + NM_RENDER_SCAN - 1) / NM_RENDER_SCAN;
    const size_t cnt_bytes = ((size_t)nt * sizeof(int) + 255) & ~(size_t)255, sum_bytes = (size_t)nblk * sizeof(long long);
    if ((rc = nm_ctx_reserve(c, cnt_bytes + sum_bytes + 4096))) return rc;
    c->ws.release(0);
    int* counts = static_cast<int*>(c->ws.alloc_bytes(cnt_bytes));
    long long* bsum = static_cast<long long*>(c->ws.alloc_bytes(sum_bytes));
    if (!counts || !bsum) { nm_set_error("mesh_bin: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    if ((rc = nm_check_hip(hipMemsetAsync(counts, 0, (size_t)nt * sizeof(int), s), "mesh_bin memset"))) return rc;
    const long long rows = (long long)F * M;
    if (rows > 0) {
        const unsigned grid = (unsigned)((rows + NM_RENDER_BLOCK - 1) / NM_RENDER_BLOCK);
        hipLaunchKernelGGL(mesh_transform_kernel, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, vertices, (const int*)triangles, (int)V, (long long)M, rows, cam, rec,
                           (int*)rect);
        hipLaunchKernelGGL(mesh_tiles_kernel<false>, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, (const int*)rect, (long long)M, rows, cam.TX, cam.TY, counts,
                           (const long long*)nullptr, 0ll, (int*)nullptr);
    }
    long long* off = reinterpret_cast<long long*>(tile_offsets);
    hipLaunchKernelGGL(render_scan_local_kernel, dim3((unsigned)nblk), dim3(NM_RENDER_BLOCK), 0, s, (const int*)counts, nt, off, bsum);
    hipLaunchKernelGGL(render_scan_sums_kernel, dim3(1), dim3(NM_RENDER_BLOCK), 0, s, bsum, nblk, nt, off);
    hipLaunchKernelGGL(render_scan_add_kernel, dim3((unsigned)nblk), dim3(NM_RENDER_BLOCK), 0, s, (const long long*)bsum, nt, off);
    return nm_check_hip(hipGetLastError(), "mesh_bin launch");
} catch (...) { return nm_abi_catch("nm_mesh_bin"); }

int nm_mesh_draw(nm_ctx* c, const double* rec, const int32_t* rect, const int64_t* tile_offsets, const int32_t* triangles, const double* vertex_colors,
                 const double* color, int32_t F, int32_t V, int64_t M, const nm_camera* camera, double light_a, double light_b, const double* background,
                 int64_t capacity, int32_t* list, int32_t* index, double* depth, uint8_t* image) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = mesh_check("mesh_draw", c, F, camera, &cam, &nt);
    if (rc) return rc;
    if ((rc = mesh_sizes("mesh_draw", F, V, M))) return rc;
    if (capacity < 0) { nm_set_error("mesh_draw: capacity %lld", (long long)capacity); return NM_ERR_ARG; }
    if (!tile_offsets || (M > 0 && (!rec || !rect)) || (capacity > 0 && !list)) { nm_set_error("mesh_draw: null argument"); return NM_ERR_ARG; }
    if (image && M > 0 && vertex_colors && !triangles) { nm_set_error("mesh_draw: vertex_colors without triangles"); return NM_ERR_ARG; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    if (!index && !depth && !image) return NM_OK;                // nothing to write
    const size_t cur_bytes = (size_t)nt * sizeof(int);
    if ((rc = nm_ctx_reserve(c, cur_bytes + 4096))) return rc;
    c->ws.release(0);
    int* cursor = static_cast<int*>(c->ws.alloc_bytes(cur_bytes));
    if (!cursor) { nm_set_error("mesh_draw: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    const long long* off = reinterpret_cast<const long long*>(tile_offsets);
    const long long rows = (long long)F * M;
    if (rows > 0 && capacity > 0) {
        if ((rc = nm_check_hip(hipMemsetAsync(cursor, 0, cur_bytes, s), "mesh_draw memset"))) return rc;
        const unsigned grid = (unsigned)((rows + NM_RENDER_BLOCK - 1) / NM_RENDER_BLOCK);
        hipLaunchKernelGGL(mesh_tiles_kernel<true>, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, (const int*)rect, (long long)M, rows, cam.TX, cam.TY, cursor, off,
                           (long long)capacity, (int*)list);
    }
    const double white[3] = {1.0, 1.0, 1.0}, grey[3] = {0.7, 0.7, 0.7};
    const double* bg = background ? background : white;
    const double* uc = color ? color : grey;
    MeshShade sh;
    sh.light_a = light_a; sh.light_b = light_b;
    for (int k = 0; k < 3; ++k) { sh.color[k] = uc[k]; sh.bg[k] = mesh_host_byte(bg[k]); }
    hipLaunchKernelGGL(mesh_draw_kernel, dim3((unsigned)nt), dim3(NM_RENDER_BLOCK), 0, s, rec, (const int*)rect, (const int*)triangles, vertex_colors, off,
                       (const int*)list, (long long)M, rows, rows > 0 ? (long long)capacity : 0ll, cam, sh, (int*)index, depth, (unsigned char*)image);
    return nm_check_hip(hipGetLastError(), "mesh_draw launch");
} catch (...) { return nm_abi_catch("nm_mesh_draw"); }

int nm_mesh_shade(nm_ctx* c, const double* rec, const int32_t* index, const int32_t* triangles, const double* normals, const double* vertex_colors,
                  const double* color, int32_t F, int32_t V, int64_t M, const nm_camera* camera, double light_a, double light_b, const double* background,
                  uint8_t* image) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = mesh_check("mesh_shade", c, F, camera, &cam, &nt);
    if (rc) return rc;
    if ((rc = mesh_sizes("mesh_shade", F, V, M))) return rc;
    if (!index || !image || (M > 0 && (!rec || !triangles || !normals))) { nm_set_error("mesh_shade: null argument"); return NM_ERR_ARG; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    const double white[3] = {1.0, 1.0, 1.0}, grey[3] = {0.7, 0.7, 0.7};
    const double* bg = background ? background : white;
    const double* uc = color ? color : grey;
    MeshShade sh;
    sh.light_a = light_a; sh.light_b = light_b;
    for (int k = 0; k < 3; ++k) { sh.color[k] = uc[k]; sh.bg[k] = mesh_host_byte(bg[k]); }
    const long long pixels = (long long)F * cam.H * cam.W;
    hipLaunchKernelGGL(mesh_shade_kernel, dim3((unsigned)((pixels + NM_RENDER_BLOCK - 1) / NM_RENDER_BLOCK)), dim3(NM_RENDER_BLOCK), 0, c->stream, rec,
                       (const int*)index, (const int*)triangles, normals, vertex_colors, (int)V, (long long)M, pixels, cam, sh, (unsigned char*)image);
    return nm_check_hip(hipGetLastError(), "mesh_shade launch");
} catch (...) { return nm_abi_catch("nm_mesh_shade"); }

int nm_skeleton_draw(nm_ctx* c, const float* keypoints, const int32_t* parents, int32_t F, int32_t K, const nm_camera* camera, double threshold,
                     double radius, double bone_radius, const double* joint_colors, const double* joint_color, const double* bone_color, double light_a,
                     double light_b, const double* background, int32_t overlay, int32_t* index, double* depth, uint8_t* image) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = mesh_check("skeleton_draw", c, F, camera, &cam, &nt);
    if (rc) return rc;
    if (K < 1 || K > NM_SKEL_MAXK) { nm_set_error("skeleton_draw: K = %d joints (1 .. %d)", (int)K, NM_SKEL_MAXK); return NM_ERR_ARG; }
    if (!keypoints || !parents) { nm_set_error("skeleton_draw: null argument"); return NM_ERR_ARG; }
    if (!(radius > 0.0) || !std::isfinite(radius) || !(bone_radius > 0.0) || !std::isfinite(bone_radius)) {
        nm_set_error("skeleton_draw: radius %g, bone_radius %g", radius, bone_radius);
        return NM_ERR_ARG;
    }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    if (!index && !depth && !image) return NM_OK;                // nothing to write
    const double white[3] = {1.0, 1.0, 1.0}, red[3] = {0.7, 0.1, 0.0}, green[3] = {0.0, 0.6, 0.1};
    const double* bg = background ? background : white;
    const double* jc = joint_color ? joint_color : red;
    const double* bc = bone_color ? bone_color : green;
    SkelArgs a;
    a.threshold = threshold; a.radius = radius; a.bone_radius = bone_radius; a.light_a = light_a; a.light_b = light_b;
    for (int k = 0; k < 3; ++k) { a.joint_color[k] = jc[k]; a.bone_color[k] = bc[k]; a.bg[k] = mesh_host_byte(bg[k]); }
    a.K = K; a.overlay = overlay != 0;
    hipLaunchKernelGGL(skeleton_draw_kernel, dim3((unsigned)nt), dim3(NM_RENDER_BLOCK), 0, c->stream, keypoints, (const int*)parents, joint_colors, cam, a,
                       (int*)index, depth, (unsigned char*)image);
    return nm_check_hip(hipGetLastError(), "skeleton_draw launch");
} catch (...) { return nm_abi_catch("nm_skeleton_draw"); }

}  // extern "C"
