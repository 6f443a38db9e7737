// The launch plan of a forward conv: which of the kernels of nm_conv.hip / nm_up2c.hip takes a call, its instantiation, grid, LDS bytes,
// every integer of ConvParams, the XCD super-tile, the profiler's variant and the GroupNorm partial rows per frame the kernel writes -
// decided once, here.  nm_launch_conv validates its arguments, plans, refuses or fills ConvParams, and launches by the plan's enum;
// nm_conv_blocks_per_frame is the plan's part_rows; nm_net.hip asks its routing questions (pool_on_pool_kernels, k3_on_f16r,
// up2c_eligible) with the predicates plan() itself routes by.  Plain integer C++ (no HIP headers, no globals: the launch switches come
// in as a struct): tests/cpp/conv_plan.cpp pins the plans of the network's layers and sweeps the sizing properties on the host.
//
// Routing, in this order: a fused-upsample layer with composite weights -> conv_up2c (nm_up2c.hip).  A k2 s2 p0 conv on 4 x 8 x 8 output
// bricks -> the pool kernels (conv_pool_f16q: bfloat16 storage, or NM355_POOL_Q with at most 128 channels; else conv_pool_f16s).  The
// persistent producer / consumer kernels take k3 s1 p1 layers of whole 4 x 8 x 8 bricks, at least four of them along z: Cout % 64 == 0 ->
// conv_f16p2 (one-product modes: conv_f16q2); Cout == 32 in the one-product modes -> conv_f16r; Cout == 32 with three products, fp32
// storage and OD % 8 == 0 -> conv_f16p8 (8 x 8 x 8 bricks); what is left of Cout == 32 (OD % 8 == 4, bfloat16 storage, conv_f16r
// switched off) and conv mode 2's Cout % 32 == 0 -> conv_f16p.  Other k1 / k3 s1 layers on 4 x 8 x 8 bricks whose re-pitched halo fits
// 80 KB -> conv_f16s.  Everything else -> conv_mfma (exact fp32; split-fp16 weights on tiny volumes).  Every bfloat16 refusal is made
// here, before any launch.
//
// part_rows: the rows per frame of `part` the chosen kernel writes - the tiling's nbz nby nbx (conv_mfma, conv_f16s, pool kernels), the
// 4 x 8 x 8 bricks (OD / 4)(OH / 8)(OW / 8) of the persistent kernels (conv_f16p8 writes two rows per 8 x 8 x 8 brick), 8 bricks + 4 face
// groups + edge items of conv_up2c.  The conv mode 0 plan of a call never has more rows than the plan of any other mode (the sweep of
// tests/cpp/conv_plan.cpp): nm_op_conv3d's fp32 retry writes into the rows reserved for the first launch.
#pragma once
#include <cstddef>
#include "nm_brick_walk.h"
#include "nm_f16p8_plan.h"

namespace nm_conv_plan {

constexpr int ERR_ARG = -1, ERR_UNSUPPORTED = -4;      // NM_ERR_ARG / NM_ERR_UNSUPPORTED of include/nm355.h (asserted in nm_conv.hip)
constexpr size_t LDS_MAX = 160 * 1024;                 // gfx950: 163 840 B of LDS per workgroup

// ---- LDS layouts of the persistent producer / consumer kernels (the kernels' pointers and the plan's byte count both come from here;
// conv_f16p8: nm_f16p8_plan.h), in this order: halo tiles and weights (16-byte slots), GroupNorm scratch (floats), the bias [Cout], TAIL bytes
template <int HALO_SLOTS, int WEIGHT_SLOTS, int RED_FLOATS, int TAIL = 0>
struct PcLds {
    static constexpr int kHaloSlots = HALO_SLOTS, kWeightSlots = WEIGHT_SLOTS, kRedFloats = RED_FLOATS;
    static constexpr size_t bytes(int Cout) { return (size_t)(HALO_SLOTS + WEIGHT_SLOTS) * 16 + (size_t)(RED_FLOATS + Cout) * sizeof(float) + TAIL; }
};
using F16pLds = PcLds<2 * 4 * 600, 3 * 9 * 4 * 32, 4 * 32 * 2>;     // halo [2][hi h0 | hi h1 | lo h0 | lo h1][600], weights [3][9 taps][4 planes][32], red [4 waves][32][2]
using F16p2Lds = PcLds<2 * 4 * 600, 2 * 9 * 4 * 64, 4 * 64 * 2>;    // weights [2][9 taps][4 planes][64], red [4 waves][64][2]
using F16q2Lds = PcLds<2 * 2 * 600, 2 * 27 * 2 * 64, 4 * 64 * 2>;   // halo [2][h0 | h1][600], weights [2][27 taps][h0 | h1][64]
// conv_f16r's tail, behind the bias: the store slots of the MFMA-wave lanes that hold no total (nobody reads them).  A lane's slot is
// kLane bytes at tid * kLane, a channel's totals go kChannels' worth of compile-time offsets further, and the parity of the brick moves
// every store by kParity = one parity of `red`, so that one address register serves the real rows and the dummy slots alike.
struct F16rTail { static constexpr int kLane = 8, kChannels = 256, kParity = 4 * 32 * 2 * (int)sizeof(float), kBytes = 256 * kLane + kChannels + kParity; };
static_assert(((15 & 3) + 8 * (15 >> 2)) * 8 + 8 <= F16rTail::kChannels, "the largest channel offset of a totals store (register r = 15) stays inside the span");
template <int C16T>                                                 // weights [27 taps][C16T][h0 | h1][32], red [2 brick parities][4 waves][32][2]
using F16rLds = PcLds<2 * 2 * 600, 27 * C16T * 64, 2 * 4 * 32 * 2, F16rTail::kBytes>;
static_assert(F16rTail::kParity * 2 == F16rLds<2>::kRedFloats * (int)sizeof(float) && F16rTail::kBytes == 2048 + 256 + 1024, "conv_f16r tail");
// Cout is a launch parameter of the first three: 512 channels is more than any layer has (conv_f16q2 is routed at most 1024)
static_assert(F16pLds::bytes(32) == 133248 && F16pLds::bytes(512) <= LDS_MAX, "conv_f16p LDS");
static_assert(F16p2Lds::bytes(64) == 152832 && F16p2Lds::bytes(512) <= LDS_MAX, "conv_f16p2 LDS");
static_assert(F16q2Lds::bytes(64) == 151296 && F16q2Lds::bytes(1024) <= LDS_MAX, "conv_f16q2 LDS");
static_assert(F16rLds<2>::bytes(32) == 99200 && F16rLds<4>::bytes(32) == 154496 && F16rLds<4>::bytes(32) <= LDS_MAX, "conv_f16r LDS");

// ---- conv_up2c (nm_up2c.hip): coarse cells of a brick, LDS of the main and face kernels, shell items
namespace up2c {
constexpr int BZ = 2, BY = 8, BX = 8;                  // coarse cells of a brick (per parity class: 128 GEMM rows)
constexpr int HZ = BZ + 2, HY = BY + 2, HX = BX + 2;   // coarse halo tile
constexpr int ZP = 104;                                // z-plane pitch in 16-byte slots: >= HY*HX and = 8 (mod 16)
constexpr int HVP = HZ * ZP + 1;                       // slots per (chunk, hi|lo, lane half) plane; odd: staging writes spread over the banks
constexpr int CG = 32;                                 // input channels per LDS buffer (two buffers: one read by the MFMAs, one being staged)
constexpr int NPLANES = CG / 16 * 4;
constexpr size_t LDS_BYTES = (size_t)2 * NPLANES * HVP * 16 + 2 * CG * sizeof(float);      // + the next tile's GroupNorm scale / shift
constexpr int YT = HY;                                 // row tiles of a brick of conv_up2y_kernel
constexpr int FP = 36;                                 // slots per staged line of the face kernels (34 used)
constexpr int face_fpv(int R) { return (R + 2) * FP + 1; }          // slots per plane of a face workgroup of R lines (odd)
static_assert(LDS_BYTES <= LDS_MAX, "conv_up2c LDS");

struct Shell { int TZ, TY, TX, face_groups, edge_items; };          // 32-cell tiles of the faces, items per frame
constexpr Shell shell(int ID, int IH, int IW) {
    const int TZ = (ID + 31) / 32, TY = (IH + 31) / 32, TX = (IW + 31) / 32;
    return {TZ, TY, TX, 2 * ID * TY + 2 * ID * TX + 2 * IH * TX, 8 * (TZ + TY + TX)};
}
// GroupNorm partial rows per frame the launches write: 8 per brick, 4 per face group, 1 per edge item
constexpr int part_rows(int ID, int IH, int IW) {
    return 8 * (ID / BZ) * (IH / BY) * (IW / BX) + 4 * shell(ID, IH, IW).face_groups + shell(ID, IH, IW).edge_items;
}
}  // namespace up2c

enum Kernel { CONV_MFMA, CONV_F16S, CONV_POOL_F16S, CONV_POOL_F16Q, CONV_F16P, CONV_F16P2, CONV_F16P8, CONV_F16Q2, CONV_F16R, CONV_UP2C };
constexpr const char* kernel_name(Kernel k) {
    constexpr const char* names[] = {"conv (fp32 MFMA kernel)", "conv_f16s", "conv_pool_f16s", "conv_pool_f16q", "conv_f16p", "conv_f16p2", "conv_f16p8", "conv_f16q2", "conv_f16r", "conv_up2c"};
    return names[k];
}
enum Refusal {
    TAKEN,
    SPARSE_NOT_POOL,    // a brick-sparse input that does not go to the pool kernels (ERR_ARG)
    IN2_NOT_POOL,       // an un-materialised residual pair that does not go to the pool kernels (ERR_ARG)
    LDS_TILE,           // the tiling's halo tile exceeds the LDS
    BF16_NO_KERNEL,     // no instantiation of Plan::kernel for this bfloat16 input / output in this conv mode
    BF16_UP2C           // conv_up2c: bfloat16 storage outside the one-product modes
};
// conv_up2c's launches
enum Up2cMain { UP2C_ONE, UP2C_X16, UP2Y, UP2Y_MARCH };    // conv_up2c_kernel<IO> | conv_up2c_x16_kernel | conv_up2y_kernel<false | true>
enum Up2cFace { FACE, FACE_R };                            // conv_up2c_face_kernel | conv_up2c_face_r_kernel<R, R == 2 ? 9 : 6>
enum Up2cEdge { EDGE, EDGE_P };                            // conv_up2c_edge_kernel | conv_up2c_edge_p_kernel

// the switches the decision reads (NmLaunchState): conv mode 1 / 2 / 3,4 and the NM355_* switches of the same names
struct Switches {
    int conv_mode;              // 0: exact fp32 MFMA everywhere, 1: split-fp16 where the layer shape allows
    bool f16p_all, single;      // conv mode 2 / the one-product modes 3 and 4 (single implies conv_mode 1)
    int pool_q, f16r, up2y, up2y_march, up2y_ypad, up2c_shell;
};

struct Call {
    int N, ID, IH, IW;          // frames, STORED input extents (up2: the coarse grid)
    int Cin, cin_real;          // padded / real input channels
    int Cout, Co_pad, ks, stride, pad;
    bool up2;                   // the input's trilinear x2 upsampling is convolved
    bool have_w16, have_up2c;   // split-fp16 weights / composite weight sets exist
    bool in_h, out_h;           // the tensor is stored as bfloat16
    bool has_in2;               // the input is an un-materialised residual pair (TensorRef::p2)
    bool has_map, has_alt;      // brick-sparse input (TensorRef::brickmap, alt)
    int wgs_cap, cus;           // this launch's workgroup cap (0: none), compute units of the device
};

struct Up2cPlan {
    int io;                                             // storage of the call: bit 0 bfloat16 input, bit 1 bfloat16 output
    Up2cMain main; bool march, ypad; int main_grid;
    Up2cFace face; int R, face_grid; size_t face_lds;
    Up2cEdge edge; int edge_grid, slot0;                // slot0: the edge items' first partial row, 8 bricks + 4 face groups
    up2c::Shell sh;
    int nbz, nby, nbx;
};

struct Plan {
    Refusal why;
    int status;                 // 0, or the error code of the refusal
    Kernel kernel;
    int MT, NT, KS; bool UP2, SINGLE; int IO, C16T; bool IN2;       // instantiation (what the kernel's template takes of it)
    int grid_x, grid_y, threads;                        // (conv_up2c: the main launch's)
    size_t lds;
    int OD, OH, OW;
    int bz_l2, by_l2, bx_l2, nbz, nby, nbx, KC, HZ, HY, HX, HV, HVp, CVp, ZP, ksplit;      // ConvParams
    nm_walk::SuperTile st;
    bool w_f16;                 // ConvParams::w is the split-fp16 pack (else the fp32 pack)
    bool w16;                   // ConvParams::w16 is set: conv_mfma<1, NT> on split-fp16 weights
    int work, variant;          // work items of a persistent launch; the profiler's family
    int taps; double flops_factor;                      // the profiler's FLOPs: conv_flops(taps) * flops_factor
    int part_rows;
    Up2cPlan up;
};

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
inline size_t smax(size_t a, size_t b) { return a > b ? a : b; }
inline int ceil_log2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

inline Plan refuse(Plan q, Refusal why) { q.why = why; q.status = why == SPARSE_NOT_POOL || why == IN2_NOT_POOL ? ERR_ARG : ERR_UNSUPPORTED; return q; }

// ---- eligibility: the predicates plan() routes by ------------------------------------------------------------------------------------
// conv_up2c takes the fused-upsample layer of this COARSE input: the 64 -> 32 layer, and in the product form (split-fp16, NM355_UP2Y) also
// Cin <= 128, Cout <= 64 - the one-product modes and NM355_UP2Y=0 keep the wider layer on conv_f16s
inline bool up2c_eligible(const Switches& sw, int ID, int IH, int IW, int Cin, int Cout, int ks, int stride, int pad) {
    return ks == 3 && stride == 1 && pad == 1 && ID % up2c::BZ == 0 && IH % up2c::BY == 0 && IW % up2c::BX == 0 && Cin % up2c::CG == 0 && Cout % 32 == 0 &&
           ((Cin == 64 && Cout == 32) || (sw.up2y && !sw.single && Cin <= 128 && Cout <= 64));
}
// the split-fp16 mode runs conv_up2c's main launch in the product-then-interpolate form along y (4 x 27 instead of 8 x 27 products per
// coarse voxel)
inline bool up2y_main(const Switches& sw, int io) { return io == 0 && sw.conv_mode == 1 && !sw.single && sw.up2y != 0; }

// the output tiling of conv_mfma / conv_f16s / the pool kernels: 256 (128 below 256 voxels) output voxels per brick
struct Tiling { int MT, NT, bz_l2, by_l2, bx_l2, nbz, nby, nbx, KC, HZ, HY, HX, HV, HVp, CVp; size_t lds_bytes; };
inline Tiling choose_tiling(int OD, int OH, int OW, int Co_pad, int ks, int stride, bool up2, int Cin) {
    Tiling t;
    t.MT = OD * OH * OW >= 256 ? 2 : 1;
    t.NT = (Co_pad % 64 == 0) ? 2 : 1;
    t.bx_l2 = imin(3, ceil_log2(OW));
    t.by_l2 = imin(3, ceil_log2(OH));
    t.bz_l2 = (t.MT == 2 ? 8 : 7) - t.bx_l2 - t.by_l2;
    const int BX = 1 << t.bx_l2, BY = 1 << t.by_l2, BZ = imin(1 << t.bz_l2, OD);
    t.nbx = (OW + BX - 1) / BX; t.nby = (OH + BY - 1) / BY; t.nbz = (OD + (1 << t.bz_l2) - 1) >> t.bz_l2;
    t.HX = (imin(BX, OW) - 1) * stride + ks;
    t.HY = (imin(BY, OH) - 1) * stride + ks;
    t.HZ = (BZ - 1) * stride + ks;
    t.HV = t.HX * t.HY * t.HZ;
    t.HVp = t.HV + ((2 - (t.HV & 7)) & 7);
    t.CVp = 0;
    if (up2) {
        const int cv = ((t.HZ >> 1) + 2) * ((t.HY >> 1) + 2) * ((t.HX >> 1) + 2);
        t.CVp = cv + ((2 - (cv & 7)) & 7);
    }
    // channels staged per pass: 16 by default; more when the halo tile is small (<= 48 KB of LDS in total), 8 when
    // even 16 do not fit in 72 KB
    const size_t per16 = (size_t)4 * (t.HVp + t.CVp) * 16;
    t.KC = (Cin % 16 == 0) ? 16 : 8;
    if (per16 > 72 * 1024) t.KC = 8;
    else {
        const int k = (int)((48 * 1024) / per16) * 16;
        if (k > 16) t.KC = imin(k, (Cin + 15) & ~15);
        if (t.KC > Cin) t.KC = Cin;
        if (t.KC % 8) t.KC = (Cin % 16 == 0) ? 16 : 8;
    }
    t.lds_bytes = smax((size_t)(t.KC / 4) * (t.HVp + t.CVp) * 16, (size_t)4 * 64 * 2 * sizeof(float));
    return t;
}
inline bool bricks_4x8x8(const Tiling& t) { return t.MT == 2 && t.bx_l2 == 3 && t.by_l2 == 3 && t.bz_l2 == 2; }

// a k2 s2 p0 conv to these output extents goes to the pool kernels: split-fp16 weights, whole 16-channel chunks, 4 x 8 x 8 output bricks
inline bool pool_on_pool_kernels(const Switches& sw, int Cin, int OD, int OH, int OW, bool have_w16) {
    return sw.conv_mode == 1 && have_w16 && Cin % 16 == 0 && bricks_4x8x8(choose_tiling(OD, OH, OW, (Cin + 31) & ~31, 2, 2, false, Cin));
}
// a plain k3 s1 p1 conv on whole 4 x 8 x 8 bricks, at least four of them along z: the persistent kernels' layers
inline bool k3_bricks(int Cin, int ks, int stride, int pad, bool up2, int OD, int OH, int OW, bool have_w16) {
    return have_w16 && Cin % 16 == 0 && ks == 3 && stride == 1 && pad == 1 && !up2 && OD % 4 == 0 && OH % 8 == 0 && OW % 8 == 0 && OD >= 16;
}
// a plain (not fused-upsample) conv to this output, both tensors of one storage, runs on conv_f16r (one-product modes, 32 output channels: the
// layer's weights stay in LDS)
inline bool k3_on_f16r(const Switches& sw, int Cin, int Cout, int ks, int stride, int pad, int OD, int OH, int OW, bool have_w16) {
    return sw.conv_mode == 1 && sw.single && sw.f16r && k3_bricks(Cin, ks, stride, pad, false, OD, OH, OW, have_w16) && (Cin == 32 || Cin == 64) && Cout == 32;
}

// ---- the persistent kernels' grid -------------------------------------------------------------------------------------------------
// One workgroup per CU, the bricks in XCD super-tile order where a brick is one work item.  wgs_cap > 0 is the cap of THIS launch (a conv
// that runs beside another stream's chain of small dependent launches leaves it CUs), rounded down to a multiple of 8 so that every XCD
// keeps the same number of workgroups; a workgroup walks a contiguous run of ceil(items / grid) work items, whatever the grid.  The XCD
// super-tile exists for grids of 256 and 512 only (choose_super_tile: grid / 8 = 32 or 64), so a capped launch walks its bricks in
// linear order - part of what the cap costs the capped conv itself.
inline int persistent_wgs(int wgs_cap, int cus) { return wgs_cap > 0 && wgs_cap < cus ? imin(cus, imax(8, wgs_cap & ~7)) : cus; }
inline void persistent(Plan& q, const Call& c, Kernel k, int brick_z, int cout_groups, bool super_tile, size_t lds, int variant) {
    q.kernel = k; q.threads = 512; q.lds = lds; q.variant = variant; q.taps = 27; q.w_f16 = true;
    q.work = c.N * (q.OD / brick_z) * (q.OH / 8) * (q.OW / 8) * cout_groups;
    q.grid_x = imin(q.work, persistent_wgs(c.wgs_cap, c.cus)); q.grid_y = 1;
    if (super_tile) q.st = nm_walk::choose_super_tile(c.N, q.grid_x, q.OD / brick_z, q.OH / 8, q.OW / 8);
    q.part_rows = (q.OD / 4) * (q.OH / 8) * (q.OW / 8);
}

inline Up2cPlan plan_up2c(const Call& c, const Switches& sw, int io) {
    Up2cPlan u = {};
    u.io = io;
    u.nbz = c.ID / up2c::BZ; u.nby = c.IH / up2c::BY; u.nbx = c.IW / up2c::BX;
    const int bricks = u.nbz * u.nby * u.nbx, total = c.N * bricks, columns = c.N * u.nbz * u.nbx;
    // conv_up2y_kernel: whole columns of bricks along y per workgroup where that leaves no CU without one (NM355_UP2Y_MARCH=2: always),
    // zero padding along y in its epilogue (NM355_UP2Y_YPAD)
    const bool y_main = up2y_main(sw, io);
    // row tiles of the busiest workgroup: 10 per brick, or 10 + 8 (nby - 1) per column
    const long long tiles_bricks = (long long)((total + c.cus - 1) / c.cus) * up2c::YT;
    const long long tiles_columns = (long long)((columns + c.cus - 1) / c.cus) * (up2c::YT + (up2c::YT - 2) * (u.nby - 1));
    u.march = y_main && u.nby > 1 && (sw.up2y_march >= 2 || (sw.up2y_march == 1 && columns >= c.cus && tiles_columns < tiles_bricks));
    u.ypad = y_main && sw.up2y_ypad != 0;
    // (the one-product modes keep ONE kernel in fp32 and in bfloat16 storage: the instantiations are bit-compared with one another,
    //  tests/test_storage16_gpu.py)
    u.main = sw.single ? UP2C_ONE : !y_main ? UP2C_X16 : u.march ? UP2Y_MARCH : UP2Y;
    u.main_grid = imin(u.march ? columns : total, c.cus);
    u.sh = up2c::shell(c.ID, c.IH, c.IW);
    // NM355_UP2C_SHELL (split-fp16, fp32 storage only; the one-product and 16-bit-storage instantiations keep the plain kernels):
    // units 0 the plain kernels (A/B), 1 the face form (default), 2 the face and the edge form, 3 the edge form alone; tens: lines
    // per face workgroup (2 or 4; else 4 at Cin <= 64 and 2 above: DESIGN 5).  The face form fixes a thread's channel octet across
    // its staging items, so it takes the channel counts whose octets divide 256; any other keeps the plain kernel.
    const int shell = (io == 0 && !sw.single) ? sw.up2c_shell : 0;
    u.face = (shell % 10 == 1 || shell % 10 == 2) && 256 % (c.Cin / 8) == 0 ? FACE_R : FACE;
    // (the edge form's one output half: the ring's registers leave one wave per SIMD, and 1.5 items per SIMD then run in two rounds -
    //  measured slower than conv_up2c_edge_kernel on the 64 -> 32 layer, which keeps it)
    u.edge = (shell % 10 == 2 || shell % 10 == 3) && c.Cout == 64 ? EDGE_P : EDGE;
    if (u.face == FACE_R) {
        u.R = shell / 10 == 2 ? 2 : shell / 10 == 4 ? 4 : c.Cin <= 64 ? 4 : 2;
        const int GD = (c.ID + u.R - 1) / u.R, GH = (c.IH + u.R - 1) / u.R;
        u.face_grid = c.N * (2 * GD * u.sh.TY + (u.ypad ? 0 : 2 * GD * u.sh.TX) + 2 * GH * u.sh.TX);
    } else { u.R = 1; u.face_grid = c.N * u.sh.face_groups; }
    u.face_lds = (size_t)(c.Cin / 16 * 4) * up2c::face_fpv(u.R) * 16;
    u.edge_grid = (int)(((long long)c.N * u.sh.edge_items + 3) / 4);
    u.slot0 = 8 * bricks + 4 * u.sh.face_groups;
    return u;
}

inline Plan plan(const Call& c, const Switches& sw) {
    Plan q = {};
    const int us = c.up2 ? 2 : 1;
    q.OD = (us * c.ID + 2 * c.pad - c.ks) / c.stride + 1; q.OH = (us * c.IH + 2 * c.pad - c.ks) / c.stride + 1; q.OW = (us * c.IW + 2 * c.pad - c.ks) / c.stride + 1;
    const int io = (c.in_h ? 1 : 0) | (c.out_h ? 2 : 0);
    const bool f16 = sw.conv_mode == 1;
    q.KS = c.ks; q.UP2 = c.up2; q.SINGLE = sw.single; q.ksplit = 1; q.grid_y = 1; q.flops_factor = 1.0; q.taps = c.ks * c.ks * c.ks;
    if ((c.has_map || c.has_in2) && c.up2) return refuse(q, SPARSE_NOT_POOL);

    // the fused-upsample layers on the coarse grid with composite weights (nm_up2c.hip): main + shell launches, timed together
    if (c.up2 && c.have_up2c && f16 && up2c_eligible(sw, c.ID, c.IH, c.IW, c.Cin, c.Cout, c.ks, c.stride, c.pad)) {
        q.kernel = CONV_UP2C; q.IO = io; q.variant = 12; q.threads = 512; q.lds = up2c::LDS_BYTES;
        q.up = plan_up2c(c, sw, io);
        q.grid_x = q.up.main_grid;
        if (up2y_main(sw, io)) q.flops_factor = 0.5;    // the products conv_up2y_kernel PERFORMS: 4 x 27 per coarse voxel instead of the fine conv's 8 x 27 (halo rows not counted)
        q.part_rows = up2c::part_rows(c.ID, c.IH, c.IW);
        return io && !sw.single ? refuse(q, BF16_UP2C) : q;
    }

    const Tiling t = choose_tiling(q.OD, q.OH, q.OW, c.Co_pad, c.ks, c.stride, c.up2, c.Cin);
    q.MT = t.MT; q.NT = t.NT; q.bz_l2 = t.bz_l2; q.by_l2 = t.by_l2; q.bx_l2 = t.bx_l2; q.nbz = t.nbz; q.nby = t.nby; q.nbx = t.nbx;
    q.KC = t.KC; q.HZ = t.HZ; q.HY = t.HY; q.HX = t.HX; q.HV = t.HV; q.HVp = t.HVp; q.CVp = t.CVp; q.ZP = t.HY * t.HX;
    q.lds = t.lds_bytes; q.threads = 256;
    q.part_rows = t.nbz * t.nby * t.nbx;
    q.grid_x = c.N * q.part_rows; q.grid_y = c.Co_pad / (t.NT * 32);
    if (t.lds_bytes > LDS_MAX) return refuse(q, LDS_TILE);
    const bool pool = c.ks == 2 && c.stride == 2 && c.pad == 0 && !c.up2 && pool_on_pool_kernels(sw, c.Cin, q.OD, q.OH, q.OW, c.have_w16);
    if (c.has_in2 && !(pool && !c.has_map)) return refuse(q, IN2_NOT_POOL);
    if (c.has_map && !(pool && c.has_alt && c.ID % 4 == 0 && c.IH % 8 == 0 && c.IW % 8 == 0)) return refuse(q, SPARSE_NOT_POOL);

    if (pool) {
        // 16-bit storage: the pool convs of the training path (one-product modes, input always bfloat16); the affine table of
        // conv_pool_f16q holds 128 channels
        const bool qk = io || (sw.pool_q && c.Cin <= 128);
        q.kernel = qk ? CONV_POOL_F16Q : CONV_POOL_F16S; q.IO = io; q.IN2 = qk && !io && c.has_in2;
        q.lds = 0; q.variant = 8; q.w_f16 = true;
        return io && (!sw.single || c.Cin > 128 || c.has_in2 || c.has_map || !(io & 1)) ? refuse(q, BF16_NO_KERNEL) : q;
    }
    if (f16 && k3_bricks(c.Cin, c.ks, c.stride, c.pad, c.up2, q.OD, q.OH, q.OW, c.have_w16)) {
        // (conv_f16q2 keeps a whole step's weights in LDS: a one-product call with more than 1024 output channels - no layer has more
        // than 256 - goes on to conv_f16s, which has no bfloat16 form for k3)
        if (c.Cout % 64 == 0 && !(sw.single && c.Cout > 1024)) {
            // 16-bit storage: both tensors bfloat16 (layers at >= 32^3 and their data gradients), one-product modes only (refused in
            // the family's name, conv_f16p2)
            const bool no16 = io && (io != 3 || !sw.single);
            if (sw.single && !no16) { persistent(q, c, CONV_F16Q2, 4, c.Cout / 64, c.Cout == 64, F16q2Lds::bytes(c.Cout), 14); q.IO = io; }
            else persistent(q, c, CONV_F16P2, 4, c.Cout / 64, c.Cout == 64, F16p2Lds::bytes(c.Cout), 9);
            return no16 ? refuse(q, BF16_NO_KERNEL) : q;
        }
        if (k3_on_f16r(sw, c.Cin, c.Cout, c.ks, c.stride, c.pad, q.OD, q.OH, q.OW, c.have_w16) && c.in_h == c.out_h) {
            q.C16T = c.Cin / 16; q.IO = io;
            persistent(q, c, CONV_F16R, 4, 1, true, q.C16T == 2 ? F16rLds<2>::bytes(32) : F16rLds<4>::bytes(32), 15);
            return q;
        }
        // three products, fp32 in and out, exactly 32 output channels, whole 8 x 8 x 8 bricks: conv_f16p8 (twice the MFMAs per staged
        // step; bit-identical to conv_f16p, which keeps OD % 8 == 4, the one-product / bfloat16 forms and conv mode 2's several cout
        // groups).  Profiler variant 7: it files under the conv_f16p family (all 16 variant slots are taken).
        if (!sw.single && c.Cout == 32 && q.OD % 8 == 0 && !io) {
            persistent(q, c, CONV_F16P8, 8, 1, true, (size_t)nm_f16p8::kLdsBytes, 7);
            return q;
        }
        // (with more cout groups per brick conv_f16p re-stages the input per group and measures a little slower than conv_f16s: only
        // conv mode 2, the parity tests of that path, sends every eligible layer here)
        if (c.Cout % 32 == 0 && (sw.f16p_all || c.Cout == 32)) {
            persistent(q, c, CONV_F16P, 4, c.Cout / 32, c.Cout == 32, F16pLds::bytes(c.Cout), 7); q.IO = io;
            // 16-bit storage: both tensors bfloat16 (layers at >= 32^3 and their data gradients)
            return io && (io != 3 || !sw.single) ? refuse(q, BF16_NO_KERNEL) : q;
        }
    }
    if (f16 && c.have_w16 && c.Cin % 16 == 0 && bricks_4x8x8(t) && c.stride == 1 && (c.ks == 1 || c.ks == 3) && t.HZ == c.ks + 3 && t.HY * t.HX * 2 <= 256) {
        // conv_f16s: halo planes padded to a pitch of 4 (mod 16) 16-B slots: conflict-free A reads.  (The pitch stays in ZP where the
        // call goes on to conv_mfma, which does not read it.)
        const int area = t.HY * t.HX;
        q.ZP = area + ((4 - (area & 15)) & 15);
        const int hv = t.HZ * q.ZP, HVp = hv + ((2 - (hv & 7)) & 7);
        const bool blds = t.NT == 1 && c.ks == 3;                   // two 9-tap weight groups in LDS (Cout = 32 layers)
        const size_t lds = smax(blds ? (size_t)4 * HVp * 16 + (size_t)2 * 9 * 4 * 32 * 16 : (size_t)4 * (HVp + t.CVp) * 16, (size_t)4 * 64 * 2 * sizeof(float));
        if (lds <= 80 * 1024 && !(c.ks == 1 && c.up2)) {
            q.kernel = CONV_F16S; q.HVp = HVp; q.lds = lds; q.w_f16 = true; q.variant = (c.up2 ? 10 : 5) + (t.NT - 1);      // the fused-upsample layers are families of their own
            q.grid_x = imin(q.grid_x, 512);                         // persistent: ~2 resident workgroups per CU
            q.st = nm_walk::choose_super_tile(c.N, q.grid_x, t.nbz, t.nby, t.nbx);
            // 16-bit storage: the instantiations the training path of conv mode 4 needs - k1 layers at >= 32^3 (both tensors bfloat16)
            // and the fused-upsample layer that crosses the storage threshold (fp32 in, bfloat16 out)
            q.IO = io;
            const bool have = !io || (sw.single && ((c.ks == 1 && io == 3) || (c.ks == 3 && c.up2 && t.NT == 2 && io == 2)));
            return have ? q : refuse(q, BF16_NO_KERNEL);
        }
    }
    // conv_mfma: exact fp32; MT == 1 (tiny volumes) on split-fp16 weights where they exist
    q.kernel = CONV_MFMA; q.variant = (t.MT - 1) * 2 + (t.NT - 1); q.SINGLE = false;
    q.w16 = f16 && c.have_w16 && c.Cin % 8 == 0 && !c.up2 && t.MT == 1 && (t.KC % 16 == 0 || t.KC == c.Cin);
    if (q.w16) {
        q.lds = smax(q.lds, (size_t)(((t.KC + 15) & ~15) / 4) * (t.HVp + t.CVp) * 16);
        // tiny volumes: how many of the 4 row tiles (32 rows each) of the brick hold voxels at all
        const int top = ((imin(q.OD, 1 << t.bz_l2) - 1) << (t.bx_l2 + t.by_l2)) + ((imin(q.OH, 1 << t.by_l2) - 1) << t.bx_l2) + imin(q.OW, 1 << t.bx_l2) - 1;
        const int rw = top / 32 + 1;
        q.ksplit = rw == 1 ? 4 : (rw == 2 ? 2 : 1);
        if (q.ksplit > 1) q.lds = smax(q.lds, (size_t)4 * t.NT * 16 * 64 * sizeof(float));
    }
    return io ? refuse(q, BF16_NO_KERNEL) : q;
}

}  // namespace nm_conv_plan
