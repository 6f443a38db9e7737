// Device render path: the plates nm_occupied_surface wrote, drawn as flat discs through an open3d-style pinhole camera - the last step of
// the reference's demo scripts (vis_generation.py:171-190, vis_interpolation.py:177-185: a cylinder mesh per plate into open3d's
// off-screen visualiser, capture_screen_float_buffer, (img * 255).astype(uint8)).
//
// This is NOT open3d's image: its lighting, MSAA and GL rasterisation rules are not reproducible.  The contract is the library's own,
// written out in include/nm355.h and restated in float64 numpy in tests/render_ref.py; in short, per pixel (px, py) and plate i:
//   d = ((px - cx) / fx, (py - cy) / fy, 1);  c' = E c, a' = E a (rotation only), q = a' . c'      (plates outside the view: not drawn)
//   den = (a'_x dx + a'_y dy) + a'_z, s = q / den >= near, h = s d - c', hit iff (h_x^2 + h_y^2) + h_z^2 <= radius^2
//   the winner is the hit of the smallest s, the lowest row among equal s
// (the library is built with -ffp-contract=off: every line is numpy's operation order, unfused.)
//
// A tiled gather, no atomics on the result:
//   transform  a lane per plate: c', a', q, the frame, and a pixel rectangle that contains every pixel the plate can hit
//   bin        a lane per plate adds one to the count of every (frame, 16 x 16 tile) its rectangle touches; an exclusive scan gives the
//              tile offsets; nm_render_draw's fill pass writes the row indices into the tile lists.  Integer atomics decide the ORDER of a
//              list only, and the per-pixel minimum over (s, row) does not depend on it.
//   draw       a workgroup per tile, a thread per pixel: the tile's plates go through LDS NM_RENDER_CHUNK at a time, every thread keeps
//              its own (s, row) minimum in registers and writes its pixel once.  Bit-identical from run to run.
#include "nm_ctx.h"
#include "nm_render.h"
#include "nm_tiles.h"
#include <cmath>

namespace {

// grid ceil(rows / 256): xf[i] = c' (3), a' (3), q, the plate's frame (-1: none); rect[i] = x0, x1, y0, y1 in pixels, x0 > x1: not drawn
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_transform_kernel(const double* __restrict__ plates, const long long* __restrict__ offsets, int F,
                                                                            long long rows, RenderCam cam, double radius,
                                                                            double* __restrict__ xf, int* __restrict__ rect) {
    const long long i = (long long)blockIdx.x * NM_RENDER_BLOCK + threadIdx.x;
    if (i >= rows) return;
    int lo = 0, hi = F - 1;                                      // the last frame with offsets[f] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const bool framed = offsets[lo] <= i && i < offsets[lo + 1];
    const double* p = plates + i * 12;
    const double ax = p[2], ay = p[6], az = p[10], cx = p[3], cy = p[7], cz = p[11];
    const double* e = cam.e;
    const double tx = ((e[0] * cx + e[1] * cy) + e[2] * cz) + e[3];
    const double ty = ((e[4] * cx + e[5] * cy) + e[6] * cz) + e[7];
    const double tz = ((e[8] * cx + e[9] * cy) + e[10] * cz) + e[11];
    const double rx = (e[0] * ax + e[1] * ay) + e[2] * az;
    const double ry = (e[4] * ax + e[5] * ay) + e[6] * az;
    const double rz = (e[8] * ax + e[9] * ay) + e[10] * az;
    const double q = (rx * tx + ry * ty) + rz * tz;
    double* o = xf + i * NM_RENDER_XF;
    o[0] = tx; o[1] = ty; o[2] = tz; o[3] = rx; o[4] = ry; o[5] = rz; o[6] = q; o[7] = framed ? (double)lo : -1.0;
    const bool finite = isfinite(tx) && isfinite(ty) && isfinite(tz) && isfinite(rx) && isfinite(ry) && isfinite(rz);
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    if (framed && finite && !(tz - radius < cam.near)) {
        // Every hit point h' = s d has |h' - c'| <= rb, where rb is the radius with room for the rounding of m (a few ulps of |c'|^2
        // against radius^2), and its depth is s >= near.  So s lies in [zn, zf], h'_x in [c'_x - rb, c'_x + rb], and dx = h'_x / s between
        // the quotients below; the same along y.  One pixel on either side covers the rounding of dx itself.
        const double rb = radius * (1.0 + 1e-9) + 1e-12 * (((tx * tx + ty * ty) + tz * tz) / radius);
        const double zn = tz - rb > cam.near ? tz - rb : cam.near, zf = tz + rb;
        const double xl = tx - rb, xh = tx + rb, yl = ty - rb, yh = ty + rb;
        const double ua = cam.cx + cam.fx * (xl / (xl >= 0.0 ? zf : zn)), ub = cam.cx + cam.fx * (xh / (xh >= 0.0 ? zn : zf));
        const double va = cam.cy + cam.fy * (yl / (yl >= 0.0 ? zf : zn)), vb = cam.cy + cam.fy * (yh / (yh >= 0.0 ? zn : zf));
        const double umin = (ua < ub ? ua : ub) - 1.0, umax = (ua < ub ? ub : ua) + 1.0;
        const double vmin = (va < vb ? va : vb) - 1.0, vmax = (va < vb ? vb : va) + 1.0;
        // clamped to the image while still doubles; a NaN takes the conservative side
        x0 = umin > 0.0 ? (umin < (double)cam.W ? (int)floor(umin) : cam.W) : 0;
        x1 = umax < (double)(cam.W - 1) ? (umax >= 0.0 ? (int)ceil(umax) : -1) : cam.W - 1;
        y0 = vmin > 0.0 ? (vmin < (double)cam.H ? (int)floor(vmin) : cam.H) : 0;
        y1 = vmax < (double)(cam.H - 1) ? (vmax >= 0.0 ? (int)ceil(vmax) : -1) : cam.H - 1;
        if (x0 > x1 || y0 > y1) { x0 = 0; x1 = -1; y0 = 0; y1 = -1; }
    }
    int* r = rect + i * 4;
    r[0] = x0; r[1] = x1; r[2] = y0; r[3] = y1;
}

// grid ceil(rows / 256).  FILL false: counts[tile] += 1 for every tile of the plate's rectangle; true: the plate's row goes into each of
// those tiles' lists, at tile_offsets[tile] + (the tile's cursor), where that is below the capacity
template <bool FILL>
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_bin_kernel(const double* __restrict__ xf, const int* __restrict__ rect, long long rows, int F,
                                                                      int TX, int TY, int* __restrict__ counts,
                                                                      const long long* __restrict__ tile_offsets, long long capacity,
                                                                      int* __restrict__ list) {
    const long long i = (long long)blockIdx.x * NM_RENDER_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const int* r = rect + i * 4;
    const int x0 = r[0], x1 = r[1], y0 = r[2], y1 = r[3];
    if (x0 > x1 || y0 > y1 || x0 < 0 || y0 < 0) return;
    const double fd = xf[i * NM_RENDER_XF + 7];
    if (!(fd >= 0.0 && fd < (double)F)) return;
    const int f = (int)fd;
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

// grid F * TY * TX: workgroup t draws tile (tx, ty) of frame f, thread (lx, ly) = (tid & 15, tid >> 4) its pixel
__global__ __launch_bounds__(NM_RENDER_BLOCK) void render_draw_kernel(const double* __restrict__ xf, const int* __restrict__ rect, const double* __restrict__ colors,
                                                                       const long long* __restrict__ tile_offsets, const int* __restrict__ list,
                                                                       long long rows, long long capacity, RenderCam cam, double r2, double light_a,
                                                                       double light_b, int bg0, int bg1, int bg2, int* __restrict__ index,
                                                                       double* __restrict__ depth, unsigned char* __restrict__ image) {
    __shared__ double sh_xf[NM_RENDER_CHUNK][7];
    __shared__ int sh_idx[NM_RENDER_CHUNK];
    __shared__ unsigned sh_box[NM_RENDER_CHUNK];
    const int tid = threadIdx.x, lx = tid & (NM_RENDER_TILE - 1), ly = tid >> 4;
    const unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)cam.TX), ty = (int)((t / (unsigned)cam.TX) % (unsigned)cam.TY), f = (int)(t / ((unsigned)cam.TX * (unsigned)cam.TY));
    const int px = tx * NM_RENDER_TILE + lx, py = ty * NM_RENDER_TILE + ly;
    const bool valid = px < cam.W && py < cam.H;                 // (tiles on the right and bottom edges are partial)
    const double dx = ((double)px - cam.cx) / cam.fx, dy = ((double)py - cam.cy) / cam.fy;
    long long lo = tile_offsets[t], hi = tile_offsets[t + 1];
    if (lo < 0) lo = 0;
    if (hi > capacity) hi = capacity;                            // (a list cut by the capacity: the image is incomplete, nothing is read past it)
    double best_s = INFINITY, best_den = 0.0;
    int best_i = -1;
    for (long long base = lo; base < hi; base += NM_RENDER_CHUNK) {
        const int n = hi - base < (long long)NM_RENDER_CHUNK ? (int)(hi - base) : NM_RENDER_CHUNK;
        __syncthreads();                                         // the previous chunk has been read
        for (int j = tid; j < n; j += NM_RENDER_BLOCK) {
            const int i = list[base + j];
            unsigned box = 15u | (15u << 8);                     // x0 = 15 > x1 = 0: no pixel (an entry that is no row)
            if (i >= 0 && (long long)i < rows) {
                const double* s = xf + (size_t)i * NM_RENDER_XF;
#pragma unroll
                for (int u = 0; u < 7; ++u) sh_xf[j][u] = s[u];
                const int* r = rect + (size_t)i * 4;
                const int a0 = r[0] - tx * NM_RENDER_TILE, a1 = r[1] - tx * NM_RENDER_TILE, b0 = r[2] - ty * NM_RENDER_TILE, b1 = r[3] - ty * NM_RENDER_TILE;
                const unsigned x0 = a0 < 0 ? 0 : a0 > 15 ? 15 : a0, x1 = a1 < 0 ? 0 : a1 > 15 ? 15 : a1;
                const unsigned y0 = b0 < 0 ? 0 : b0 > 15 ? 15 : b0, y1 = b1 < 0 ? 0 : b1 > 15 ? 15 : b1;
                box = x0 | (x1 << 4) | (y0 << 8) | (y1 << 12);
            }
            sh_idx[j] = i;
            sh_box[j] = box;
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < n; ++j) {
                const unsigned box = sh_box[j];
                if ((unsigned)lx < (box & 15u) || (unsigned)lx > ((box >> 4) & 15u) || (unsigned)ly < ((box >> 8) & 15u) || (unsigned)ly > ((box >> 12) & 15u))
                    continue;                                    // outside the plate's rectangle: no hit is possible
                const double cx = sh_xf[j][0], cy = sh_xf[j][1], cz = sh_xf[j][2];
                const double den = (sh_xf[j][3] * dx + sh_xf[j][4] * dy) + sh_xf[j][5];
                if (den == 0.0) continue;
                const double s = sh_xf[j][6] / den;
                if (!(s >= cam.near)) continue;
                const double hx = s * dx - cx, hy = s * dy - cy, hz = s - cz;
                const double m = (hx * hx + hy * hy) + hz * hz;
                if (!(m <= r2)) continue;
                const int i = sh_idx[j];
                if (s < best_s || (s == best_s && i < best_i)) { best_s = s; best_i = i; best_den = den; }
            }
        }
    }
    if (!valid) return;
    const size_t o = ((size_t)f * (size_t)cam.H + (size_t)py) * (size_t)cam.W + (size_t)px;
    if (index) index[o] = best_i;
    if (depth) depth[o] = best_s;
    if (image) {
        unsigned char* im = image + o * 3;
        if (best_i < 0) {
            im[0] = (unsigned char)bg0; im[1] = (unsigned char)bg1; im[2] = (unsigned char)bg2;
        } else {
            const double shade = light_a + light_b * fabs(best_den) / sqrt((dx * dx + dy * dy) + 1.0);
            const double* c = colors + (size_t)best_i * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                double v = c[ch] * shade;
                if (v != v) v = 0.0;
                v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
                im[ch] = (unsigned char)(int)(v * 255.0);
            }
        }
    }
}

// the arguments both entry points share; on success cam holds the kernels' copy and *nt the number of (frame, tile) pairs
int render_check(const char* who, const nm_ctx* c, const int64_t* offsets, int32_t F, int64_t rows, const nm_camera* camera, double radius,
                 RenderCam* cam, long long* nt) {
    if (!c) { nm_set_error("%s: null ctx", who); return NM_ERR_ARG; }
    if (!offsets || !camera) { nm_set_error("%s: null argument", who); return NM_ERR_ARG; }
    if (F < 1 || camera->width < 1 || camera->height < 1) {
        nm_set_error("%s: F = %d frames of %d x %d pixels", who, (int)F, (int)camera->width, (int)camera->height);
        return NM_ERR_ARG;
    }
    if (rows < 0) { nm_set_error("%s: rows %lld", who, (long long)rows); return NM_ERR_ARG; }
    if (!(radius > 0.0) || !std::isfinite(radius)) { nm_set_error("%s: radius %g", who, radius); return NM_ERR_ARG; }
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
    if (rows >= (1ll << 31)) { nm_set_error("%s: %lld rows, the lists hold 32-bit row indices", who, (long long)rows); return NM_ERR_UNSUPPORTED; }
    for (int k = 0; k < 12; ++k) cam->e[k] = camera->extrinsic[k];
    cam->fx = camera->fx; cam->fy = camera->fy; cam->cx = camera->cx; cam->cy = camera->cy; cam->near = camera->near;
    cam->W = camera->width; cam->H = camera->height;
    cam->TX = (cam->W + NM_RENDER_TILE - 1) / NM_RENDER_TILE; cam->TY = (cam->H + NM_RENDER_TILE - 1) / NM_RENDER_TILE;
    *nt = (long long)F * cam->TX * cam->TY;
    return NM_OK;
}

int render_byte(double v) {
    if (v != v) v = 0.0;
    v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
    return (int)(v * 255.0);
}

}  // namespace

extern "C" {

int nm_render_bin(nm_ctx* c, const double* plates, const int64_t* offsets, int32_t F, int64_t rows, const nm_camera* camera, double radius,
                  double* xf, int32_t* rect, int64_t* tile_offsets) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = render_check("render_bin", c, offsets, F, rows, camera, radius, &cam, &nt);
    if (rc) return rc;
    if (!tile_offsets || (rows > 0 && (!plates || !xf || !rect))) { nm_set_error("render_bin: null argument"); return NM_ERR_ARG; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    const long long nblk = (nt + NM_RENDER_SCAN - 1) / NM_RENDER_SCAN;
    const size_t cnt_bytes = ((size_t)nt * sizeof(int) + 255) & ~(size_t)255, sum_bytes = (size_t)nblk * sizeof(long long);
    if ((rc = nm_ctx_reserve(c, cnt_bytes + sum_bytes + 4096))) return rc;
    c->ws.release(0);
    int* counts = static_cast<int*>(c->ws.alloc_bytes(cnt_bytes));
    long long* bsum = static_cast<long long*>(c->ws.alloc_bytes(sum_bytes));
    if (!counts || !bsum) { nm_set_error("render_bin: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    if ((rc = nm_check_hip(hipMemsetAsync(counts, 0, (size_t)nt * sizeof(int), s), "render_bin memset"))) return rc;
    if (rows > 0) {
        const unsigned grid = (unsigned)((rows + NM_RENDER_BLOCK - 1) / NM_RENDER_BLOCK);
        hipLaunchKernelGGL(render_transform_kernel, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, plates, reinterpret_cast<const long long*>(offsets), (int)F,
                           (long long)rows, cam, radius, xf, rect);
        hipLaunchKernelGGL(render_bin_kernel<false>, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, (const double*)xf, (const int*)rect, (long long)rows, (int)F,
                           cam.TX, cam.TY, counts, (const long long*)nullptr, 0ll, (int*)nullptr);
    }
    long long* off = reinterpret_cast<long long*>(tile_offsets);
    hipLaunchKernelGGL(render_scan_local_kernel, dim3((unsigned)nblk), dim3(NM_RENDER_BLOCK), 0, s, (const int*)counts, nt, off, bsum);
    hipLaunchKernelGGL(render_scan_sums_kernel, dim3(1), dim3(NM_RENDER_BLOCK), 0, s, bsum, nblk, nt, off);
    hipLaunchKernelGGL(render_scan_add_kernel, dim3((unsigned)nblk), dim3(NM_RENDER_BLOCK), 0, s, (const long long*)bsum, nt, off);
    return nm_check_hip(hipGetLastError(), "render_bin launch");
} catch (...) { return nm_abi_catch("nm_render_bin"); }

int nm_render_draw(nm_ctx* c, const double* xf, const int32_t* rect, const int64_t* offsets, const int64_t* tile_offsets, const double* colors,
                   int32_t F, int64_t rows, const nm_camera* camera, double radius, double light_a, double light_b, const double* background,
                   int64_t capacity, int32_t* list, int32_t* index, double* depth, uint8_t* image) try { NmScope nm_scope_(c);
    RenderCam cam;
    long long nt = 0;
    int rc = render_check("render_draw", c, offsets, F, rows, camera, radius, &cam, &nt);
    if (rc) return rc;
    if (capacity < 0) { nm_set_error("render_draw: capacity %lld", (long long)capacity); return NM_ERR_ARG; }
    if (!tile_offsets || (rows > 0 && (!xf || !rect)) || (capacity > 0 && !list)) { nm_set_error("render_draw: null argument"); return NM_ERR_ARG; }
    if (image && rows > 0 && !colors) { nm_set_error("render_draw: image without colors"); return NM_ERR_ARG; }
    if ((rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice"))) return rc;
    if (!index && !depth && !image) return NM_OK;                // nothing to write
    const size_t cur_bytes = (size_t)nt * sizeof(int);
    if ((rc = nm_ctx_reserve(c, cur_bytes + 4096))) return rc;
    c->ws.release(0);
    int* cursor = static_cast<int*>(c->ws.alloc_bytes(cur_bytes));
    if (!cursor) { nm_set_error("render_draw: workspace"); return NM_ERR_INTERNAL; }
    hipStream_t s = c->stream;
    const long long* off = reinterpret_cast<const long long*>(tile_offsets);
    if (rows > 0 && capacity > 0) {
        if ((rc = nm_check_hip(hipMemsetAsync(cursor, 0, cur_bytes, s), "render_draw memset"))) return rc;
        const unsigned grid = (unsigned)((rows + NM_RENDER_BLOCK - 1) / NM_RENDER_BLOCK);
        hipLaunchKernelGGL(render_bin_kernel<true>, dim3(grid), dim3(NM_RENDER_BLOCK), 0, s, xf, (const int*)rect, (long long)rows, (int)F, cam.TX, cam.TY,
                           cursor, off, (long long)capacity, (int*)list);
    }
    const double white[3] = {1.0, 1.0, 1.0};
    const double* bg = background ? background : white;
    hipLaunchKernelGGL(render_draw_kernel, dim3((unsigned)nt), dim3(NM_RENDER_BLOCK), 0, s, xf, (const int*)rect, colors, off, (const int*)list,
                       (long long)rows, rows > 0 ? (long long)capacity : 0ll, cam, radius * radius, light_a, light_b, render_byte(bg[0]),
                       render_byte(bg[1]), render_byte(bg[2]), (int*)index, depth, (unsigned char*)image);
    return nm_check_hip(hipGetLastError(), "render_draw launch");
} catch (...) { return nm_abi_catch("nm_render_draw"); }

}  // extern "C"
