// Device render path for posed meshes and skeletons (nm_mesh.hip): constants shared by the kernels and their entry points.  The tiles,
// the workgroup and the scan are the plate renderer's (nm_render.h).
#pragma once
#include "nm_render.h"

constexpr int NM_MESH_REC = 16;                                      // doubles per triangle record: X0 Y0 X1 Y1 X2 Y2, n (3), q, iz (3), three of padding
constexpr int NM_MESH_STAGED = 10;                                   // of which the draw loop reads the first ten; iz is fetched for the winner only
// The chunk.  mesh_draw_kernel stages a tile's triangles through LDS NM_MESH_CHUNK at a time: ten doubles of the record, the record's
// row and the triangle's pixel box inside the tile as two 32-bit words - 88 bytes a triangle, 11 KiB a workgroup at 128.  The eight
// workgroups that fill a CU's 32 wavefront slots then hold 88 KiB of its 160 KiB together, so LDS never limits residency.  256, the
// plates' chunk, would: 22 KiB a workgroup lets seven be resident, not eight.  (232 is the most that fits eight; 128 keeps the staging
// loop at one record per thread of the workgroup's first two wavefronts and costs two barriers per 128 triangles, against some twenty
// float64 operations per triangle and pixel.)
constexpr int NM_MESH_CHUNK = 128;
constexpr int NM_MESH_STAGED_BYTES = NM_MESH_STAGED * 8 + 4 + 4;
static_assert(NM_MESH_CHUNK * NM_MESH_STAGED_BYTES * (2048 / NM_RENDER_BLOCK) <= 160 * 1024, "eight resident workgroups' chunks fit a CU's LDS");
static_assert(NM_MESH_CHUNK <= NM_RENDER_BLOCK, "a thread stages at most one triangle per chunk");
constexpr int NM_SKEL_MAXK = 32;                                     // joints of a skeleton: at most 32 spheres and 31 bones a frame, all in LDS
