// Device surface path (nm_surface.hip): constants shared by the kernels and their entry point.
#pragma once

constexpr int NM_SURF_BLOCK = 256;          // threads per workgroup: a lane per point, a workgroup per chunk of nm_output.h
constexpr int NM_SURF_MAX_R2 = 16;          // largest squared radius: offsets of at most 4 along an axis, a 9-bit window per row
// The slab bound.  A workgroup's points lie in the i-planes its chunk of 4096 voxels touches; with the r = floor(sqrt(radius2)) planes
// on either side these are the only mask words its neighbourhoods can reach.  A slab of at most this many 64-bit words is staged in
// LDS; a longer one is read in place, through L2.  2048 words = 16 KiB: with the tables below a workgroup holds 19 KiB, so the eight
// workgroups that fill a CU's 32 wavefront slots fit its 160 KiB together.  At radius2 = 16 a chunk of two planes needs ten:
// 10 G^2 / 64 + 1 <= 2048 up to G = 114; at 64^3 (one plane per chunk) the slab is 576 words.
constexpr int NM_SURF_SLAB_WORDS = 2048;
