// Body models on the device (nm_body.hip): constants shared by the kernels and their entry points.
#pragma once

constexpr int NM_BODY_MAX_JOINTS = 64;                               // the parent table travels as a kernel argument (256 bytes)
constexpr int NM_BODY_BLOCK = 128;                                   // the vertex kernel: a lane per vertex, two wavefronts a workgroup
// Frames per table read.  posedirs (9 (J - 1) rows of 3 V doubles, 34 MB at SMPL's size) is the same for every frame, so a lane reads
// its vertex's three columns of a row once and feeds NM_BODY_FRAMES frames' accumulators from it (24 doubles in registers); the frames'
// pose features (R - I, 9 (J - 1) doubles a frame) come from LDS, laid out [row][frame] so that one row's eight values are 64
// contiguous bytes that every lane reads at the same address (a broadcast, no bank conflict).  The same LDS then holds the frames'
// J skinning transforms (12 doubles each): NM_BODY_FRAMES * J * 12 * 8 bytes = 18 432 at J = 24 and 49 152 at the limit of 64 joints,
// which keeps a workgroup under 64 KiB at every J the library accepts.
constexpr int NM_BODY_FRAMES = 8;
constexpr int NM_BODY_CHAIN_LDS = 48 * 1024;                           // the chain kernel keeps J * 4 doubles a lane in LDS: its workgroup is sized to fit
constexpr int NM_BODY_SMALL = 256;                                   // workgroup of the shape, rotation and regression kernels, the chain kernel's at most

struct NmBodyParents { int p[NM_BODY_MAX_JOINTS]; };
