// Device render path (nm_render.hip): constants shared by the kernels and their entry points.
#pragma once

constexpr int NM_RENDER_TILE = 16;                                   // a tile is 16 x 16 pixels: a workgroup per tile, a thread per pixel
constexpr int NM_RENDER_BLOCK = NM_RENDER_TILE * NM_RENDER_TILE;     // 256 threads = four wavefronts, a wavefront = four pixel rows
constexpr int NM_RENDER_XF = 8;                                      // doubles per transformed plate: c' (3), a' (3), q, one of padding
// The chunk.  draw_kernel stages a tile's plates through LDS NM_RENDER_CHUNK at a time: c', a', q as seven doubles, the row index and
// the plate's pixel box inside the tile as two 32-bit words - 64 bytes a plate, 16 KiB a workgroup at 256.  The eight workgroups that
// fill a CU's 32 wavefront slots then hold 128 KiB of its 160 KiB together, so LDS never limits residency; twice the chunk would
// (5 workgroups).  256 is also the workgroup's size: every thread fetches one plate per chunk.
constexpr int NM_RENDER_CHUNK = 256;
static_assert(NM_RENDER_CHUNK * 64 * (2048 / NM_RENDER_BLOCK) <= 160 * 1024, "eight resident workgroups' chunks fit a CU's LDS");
constexpr int NM_RENDER_SCAN = 1024;                                 // tile counts per workgroup of the scan's first pass
