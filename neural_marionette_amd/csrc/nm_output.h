// Device output path (nm_output.hip): launch geometry shared by the kernels and their entry points.
#pragma once

constexpr int NM_OUT_BLOCK = 256;          // threads per workgroup (four wavefronts)
constexpr int NM_OUT_TILE_WORDS = 4;       // occupancy words per wavefront and step: 64 lanes x one 16-byte load = 256 voxels
constexpr int NM_OUT_STEPS = 4;            // steps of a workgroup of occ_mask_kernel
constexpr int NM_OUT_CHUNK_WORDS = (NM_OUT_BLOCK / 64) * NM_OUT_TILE_WORDS * NM_OUT_STEPS;      // 64 words = 4096 voxels per chunk
static_assert(NM_OUT_CHUNK_WORDS == 64, "occ_write_kernel scans a chunk's words with one wavefront");

// what nm_surface.hip shares with nm_occupied_write: the shapes' verdict and launch geometry, and the launch of occ_chunk_scan_kernel
// (coff[f * nC + c] = set bits in the chunks before c of frame f, from the mask words alone)
struct NmOutGeom { int F, V, W, nC; };
int nm_out_geom(const char* who, int B, int T, int G, NmOutGeom* g);
void nm_out_launch_chunk_scan(hipStream_t s, const unsigned long long* bits, const NmOutGeom& g, int32_t* coff);
