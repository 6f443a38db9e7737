// Loop subdivision and smooth vertex normals on the device (nm_subdiv.hip): constants shared by the kernels and their entry points.
#pragma once

constexpr int NM_SUBDIV_BLOCK = 256;                                 // a lane per output row (a vertex), four wavefronts a workgroup
// Frames per lane.  The index tables (edge rows, rings, the vertex -> triangle lists) are the same for every frame, so a lane reads its
// row's entries once and applies them to NM_SUBDIV_FRAMES consecutive frames, the per-frame sums in registers (12 doubles); blockIdx.y
// walks the groups of frames.  Four keeps the accumulators of the normals kernel (12 doubles and three vertices' worth of temporaries)
// far from any register limit and still leaves ten workgroup rows for the demo's 40 frames at the coarsest level, whose 50 000 rows
// alone would not fill the device.
constexpr int NM_SUBDIV_FRAMES = 4;
constexpr int NM_SUBDIV_MAXY = 65535;                                // blockIdx.y's limit: more groups of frames take further launches
