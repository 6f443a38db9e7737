// Device output path (nm_output.hip): launch geometry shared by the kernels and their entry points.
#pragma once

constexpr int NM_OUT_BLOCK = 256;          // threads per workgroup (four wavefronts)
constexpr int NM_OUT_TILE_WORDS = 4;       // occupancy words per wavefront and step: 64 lanes x one 16-byte load = 256 voxels
constexpr int NM_OUT_STEPS = 4;            // steps of a workgroup of occ_mask_kernel
constexpr int NM_OUT_CHUNK_WORDS = (NM_OUT_BLOCK / 64) * NM_OUT_TILE_WORDS * NM_OUT_STEPS;      // 64 words = 4096 voxels per chunk
static_assert(NM_OUT_CHUNK_WORDS == 64, "occ_write_kernel scans a chunk's words with one wavefront");
