// Motion retargeting on the device (nm_retarget.hip): launch geometry and limits shared by the kernels and their entry points.
#pragma once

constexpr int NM_RT_MAXK = 32;      // joints (the limit of nm_ctx_create): lane k of a workgroup's first wave builds joint k's table entry
constexpr int NM_RT_BLOCK = 256;    // threads per workgroup = points per tile
constexpr int NM_RT_TC = 8;         // frames per workgroup of the pose kernel (their K x 12 transforms sit in LDS as float64)
constexpr int NM_RT_FK_BLOCK = 64;  // frames per workgroup of the forward-kinematics kernel (a thread per frame)
