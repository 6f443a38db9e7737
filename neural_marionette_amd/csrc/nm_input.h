// Device input path for batches (nm_input.hip): launch geometry and limits shared by the kernels and their entry point.
#pragma once

constexpr int NM_IN_BLOCK = 256;       // threads per workgroup = points per tile
constexpr int NM_IN_MAXPARTS = 64;     // box partials per clip (workgroups of clip_bbox_kernel along x)
constexpr int NM_IN_MAXTILES = 64;     // point tiles per frame of voxelize_batch_kernel (a workgroup strides over its frame by tiles x 256)
constexpr int NM_IN_MAXB = 65535;      // clips per call (grid y)
