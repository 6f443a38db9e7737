// The launch plan of a weight gradient: which of the seven kernels of nm_grad.hip takes a call, its grid, LDS bytes, brick and halo,
// partial-sum slots and the floats of workspace behind them - decided once, here.  nm_launch_wgrad plans, refuses or launches by the
// plan's enum, and reduces; nm_wgrad_ws_floats is the largest ws_floats over the plans a caller can reach.  Plain integer C++ (no HIP
// headers, no globals: the launch switches come in as a struct): tests/cpp/wgrad_plan.cpp pins the plans of the network's layers and
// sweeps the sizing properties on the host.
#pragma once
#include <cstddef>

namespace nm_wgrad {

constexpr int ERR_ARG = -1, ERR_UNSUPPORTED = -4;      // NM_ERR_ARG / NM_ERR_UNSUPPORTED of include/nm355.h (asserted in nm_grad.hip)
constexpr size_t LDS_MAX = 160 * 1024;

// wgrad16z_kernel keeps the per-frame scale / shift rows of its input in LDS (256 B per frame) behind its tiles.  The bound of 96
// frames is the one its predecessors' larger tiles left room for in the 163840 B (DESIGN_HISTORY.md); at 96 frames wgrad16z asks
// for 134464 B.  Bfloat16 operands exist on wgrad16z_kernel only, so above that count the plan runs it once per group of at most
// W16_TAB_FRAMES frames (balanced groups: 97 frames are 49 + 48, not 96 + 1), every group on its own range of partial-sum slots
// (Plan::group).
#define W16_TAB_FRAMES 96
// wgrad_k1_kernel's grid: one serial brick chain per workgroup
// (256 / 512 / 1024 workgroups: 2.36 / 1.92 / 1.84 ms per step over the three instantiations; the reduce grows with it)
constexpr int K1_WGS = 512;
constexpr int K5S_CHUNK_VOXELS = 8192;                 // voxels per workgroup of the first layer's gather form

// LDS bytes of the split-fp16 kernels (their tile layouts are nm_grad.hip's; asserted equal there)
constexpr size_t w16_lds() { return 2 * 32 * (40 * 32 + 16) + 2 * 32 * (16 * 16 + 16); }
// tiles, X affine table (256 B per frame), dummy item, dY affine table
constexpr size_t w16z_lds(int frames) { return 2 * 6 * 100 * 64 + 2 * 2 * 128 * 64 + (size_t)frames * 64 * sizeof(float) + 64 + 256; }
constexpr size_t w16k2_lds(int mt, bool single) { return (size_t)(single ? 1 : 2) * (32 * (32 * 32 + 16) + (size_t)mt * 32 * (8 * 16 + 16)); }

enum Kernel {
    WGRAD_TAPS,       // wgrad_kernel<0>: taps dealt to the waves (k2, k3)
    WGRAD_POINT,      // wgrad_kernel<1>: ks = 1, the waves split the voxels
    WGRAD_FIRST,      // wgrad_kernel<2>: first layer, cat[occ, x1, x2, x3] rebuilt from the occupancy
    WGRAD_K1,         // wgrad_k1_kernel: 1x1 layers, all tile pairs per workgroup
    WGRAD16,          // wgrad16_kernel: split-fp16 k3 s1, VALU transposition
    WGRAD16Z,         // wgrad16z_kernel: split-fp16 k3 s1, transposing LDS reads, bricks walked along z
    WGRAD16K2         // wgrad16k2_kernel: split-fp16 k2 s2
};
enum Refusal { TAKEN, LDS_TILE, BF16_NO_KERNEL, BF16_WGRAD16, K1_MIXED_STORAGE, ITEM_TABLES, KS_UNSUPPORTED };

// the switches the decision reads (NmLaunchState): NM355_WGRAD_TR, NM355_WGRAD_ASYNC, one-product conv modes, 16-bit storage mode
struct Switches { int wgrad_tr, wgrad_async; bool single, store16; };

// dW[m][c][tap] = sum_{n,v} dy[n, v, m] * act(in)[n, stride * v + tap - pad, c]
struct Call {
    int N;                      // frames
    int OD, OH, OW;             // dY extents
    int ID, IH, IW;             // input extents
    int M, Nc;                  // dY channels / input channels
    int ks, stride, pad;
    bool allow_f16;             // the split-fp16 kernels may take it
    bool in_h, dy_h;            // the operand is stored as bfloat16
    bool first;                 // first layer (k5 on the occupancy grid, Nc = 4)
};

struct Group { int frame0, frames, S, slot0; };

struct Plan {
    Refusal why;
    int status;                 // 0, or the error code of the refusal
    Kernel kernel;
    int ntw, mt;                // instantiation: wgrad_kernel / wgrad_k1_kernel NTW (tiles <= 4: 1, <= 8: 2, else 6), wgrad16k2_kernel MT
    bool single, hx, hd;        //   one-product form, bfloat16 input / dY
    int grid_x, grid_y, threads;     // (wgrad16z over several frame groups: the first group's; group i launches group(i).S x grid_y with w16z_lds(frames))
    size_t lds;
    int BZ, BY, BX, nbz, nby, nbx, HZ, HY, HX;      // brick, bricks per frame, halo (WgradParams)
    int S, m_tiles, n_tiles, groups;                // workgroups per tile pair, tile counts, tap groups per tile
    int slots, taps, k5occ;     // the reduce: slots filled (each m_tiles * n_tiles * groups tiles of 1024 floats), taps per weight, first-layer form
    size_t ws_floats;           // what the caller must reserve
    int n_groups, N, cols;      // frame groups of wgrad16z (1 unless bfloat16 operands at more than W16_TAB_FRAMES frames)

    // Group i of n_groups: the frames split as evenly as they go, the larger groups first; a group has no more workgroups per tile pair
    // than (frame, y, x) columns, and its partial sums sit behind those of the groups before it.
    Group group(int i) const {
        const int q = N / n_groups, r = N % n_groups, lead = i < r ? i : r;
        auto s_of = [&](int frames) { const int c = frames * cols; return c < S ? (c > 1 ? c : 1) : S; };
        return {i * q + lead, q + (i < r ? 1 : 0), s_of(q + (i < r ? 1 : 0)), lead * s_of(q + 1) + (i - lead) * s_of(q)};
    }
};

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }

inline Plan refuse(Plan q, Refusal why) { q.why = why; q.status = why == ITEM_TABLES ? ERR_ARG : ERR_UNSUPPORTED; return q; }

inline Plan plan(const Call& c, const Switches& sw) {
    Plan q = {};
    q.N = c.N; q.n_groups = 1; q.threads = 256; q.single = sw.single;
    q.m_tiles = (c.M + 31) / 32; q.n_tiles = c.first ? 1 : (c.Nc + 31) / 32;
    const int tiles = q.m_tiles * q.n_tiles;
    const bool h16 = c.in_h || c.dy_h;
    const bool same = c.ID == c.OD && c.IH == c.OH && c.IW == c.OW, twice = c.ID == 2 * c.OD && c.IH == 2 * c.OH && c.IW == 2 * c.OW;

    // 1x1 layers whose voxels are whole 64-voxel bricks: every tile pair in one workgroup, both operands through LDS once
    if (!c.first && c.ks == 1 && c.stride == 1 && c.pad == 0 && same && (c.OD * c.OH * c.OW) % 64 == 0 && tiles <= 24 &&
        (size_t)64 * (q.m_tiles * 32 + q.n_tiles * 32 + 8) * 4 <= 150 * 1024) {
        q.kernel = WGRAD_K1; q.ntw = tiles <= 4 ? 1 : tiles <= 8 ? 2 : 6; q.hx = q.hd = c.in_h;
        q.S = imin(c.N * (c.OD * c.OH * c.OW / 64), K1_WGS);
        q.grid_x = q.S; q.grid_y = 1; q.lds = (size_t)64 * (q.m_tiles * 32 + 4 + q.n_tiles * 32 + 4) * sizeof(float);
        q.groups = 1; q.slots = q.S; q.taps = 1;
        q.ws_floats = (size_t)K1_WGS * tiles * 1024;            // (the full grid's, whatever the brick count)
        return c.in_h != c.dy_h ? refuse(q, K1_MIXED_STORAGE) : q;
    }
    // k2 s2 p0 layers whose fine grid is exactly twice the coarse one, whole 8 x 8 coarse (y, x) bricks, <= 128 dY channels; bfloat16
    // operands in the one-product modes only, whole 8-channel granules, and bfloat16 dY with bfloat16 X only
    if (c.allow_f16 && !c.first && c.ks == 2 && c.stride == 2 && c.pad == 0 && twice && c.OH % 8 == 0 && c.OW % 8 == 0 && c.OD > 0 && c.M <= 128 &&
        (!c.in_h || c.Nc % 8 == 0) && (!c.dy_h || (c.M % 8 == 0 && c.in_h)) && (!h16 || sw.single)) {
        q.kernel = WGRAD16K2; q.mt = q.m_tiles <= 2 ? 2 : 4; q.hx = c.in_h; q.hd = c.dy_h;
        q.S = imax(1, imin(c.N * c.OD * (c.OH / 8) * (c.OW / 8), 512 / q.n_tiles));
        q.grid_x = q.S; q.grid_y = q.n_tiles; q.lds = w16k2_lds(q.mt, sw.single);
        q.groups = 8; q.slots = q.S; q.taps = 8;
        q.ws_floats = (size_t)q.slots * tiles * 8 * 1024;
        return q;
    }
    // split-fp16 k3: stride 1, "same" padding, output extents multiples of the 2 x 8 x 8 brick
    if (c.allow_f16 && !c.first && c.ks == 3 && c.stride == 1 && c.pad == 1 && same && c.OD % 2 == 0 && c.OH % 8 == 0 && c.OW % 8 == 0) {
        q.BZ = 2; q.BY = 8; q.BX = 8; q.nbz = c.OD / 2; q.nby = c.OH / 8; q.nbx = c.OW / 8; q.HZ = 4; q.HY = 10; q.HX = 10;
        q.groups = 27; q.taps = 27; q.cols = q.nby * q.nbx;
        // workgroups of a launch: one per CU, or - when the weight gradients run on their own stream beside the main stream's walk
        // (nm_net.hip conv_bwd) - 224, which leaves 32 CUs to the GroupNorm passes and small kernels of the walk: a whole-CU kernel on
        // every CU admits nothing beside it until it ends (73.0 -> 71.3 ms per training step; 208: 71.7, 240: 72.9, 192: 72.7; in the
        // reduced-precision mode 256 stays better: 53.4 vs 53.9).
        const int wgs = sw.wgrad_async == 1 && !sw.single ? 224 : 256;
        q.S = imax(1, imin(c.N * q.nbz * q.cols, imax(tiles, wgs) / tiles));
        // wgrad16z_kernel needs a column of at least two bricks (nbz >= 2: the ring of z-planes) and a frame table that fits - or, above
        // W16_TAB_FRAMES frames, bfloat16 operands in the 16-bit storage mode, which run as frame groups.  Everything else is
        // wgrad16_kernel: more than 96 frames of fp32 operands, NM355_WGRAD_TR=0, and a volume one brick deep (2 x 8k x 8k voxels) - no
        // layer of the network has one (cubes whose y and x extents are multiples of 8 have nbz >= 4), only the op-level entry point
        // reaches it.
        const bool z = sw.wgrad_tr && q.nbz >= 2 && (c.N <= W16_TAB_FRAMES || (h16 && sw.store16));
        q.kernel = z ? WGRAD16Z : WGRAD16; q.hx = q.hd = c.in_h;
        q.slots = q.S; q.lds = w16_lds();
        if (z) {
            q.threads = 512;
            q.n_groups = (c.N + W16_TAB_FRAMES - 1) / W16_TAB_FRAMES;
            const Group last = q.group(q.n_groups - 1);
            if (q.n_groups == 1) q.S = last.S;                  // (whole (frame, y, x) columns: no more workgroups per tile pair than columns)
            q.slots = last.slot0 + last.S;
        }
        q.grid_x = z ? q.group(0).S : q.S; q.grid_y = tiles;
        if (z) q.lds = w16z_lds(q.group(0).frames);
        q.ws_floats = (size_t)q.slots * tiles * 27 * 1024;
        // 16-bit storage: both operands bfloat16, on the z-walking kernel only (every layer of >= 32^3 voxels has nbz >= 16)
        return h16 && !(c.in_h && c.dy_h && sw.single && z) ? refuse(q, BF16_WGRAD16) : q;
    }
    // wgrad_kernel: exact fp32 MFMA
    q.kernel = c.first ? WGRAD_FIRST : c.ks == 1 ? WGRAD_POINT : WGRAD_TAPS;
    q.ntw = q.kernel == WGRAD_POINT ? 1 : c.ks == 2 ? 2 : 7; q.hx = q.kernel == WGRAD_TAPS && h16; q.hd = c.dy_h;
    const bool s2 = c.stride == 2;
    q.BX = imin(8, (c.OW + 1) & ~1); q.BY = imin(s2 ? 4 : 8, c.OH); q.BZ = imin(s2 ? 2 : 4, c.OD);
    q.nbx = (c.OW + q.BX - 1) / q.BX; q.nby = (c.OH + q.BY - 1) / q.BY; q.nbz = (c.OD + q.BZ - 1) / q.BZ;
    q.HZ = (q.BZ - 1) * c.stride + c.ks; q.HY = (q.BY - 1) * c.stride + c.ks; q.HX = (q.BX - 1) * c.stride + c.ks;
    q.groups = c.first ? 25 : c.ks * c.ks * c.ks; q.taps = c.ks * c.ks * c.ks; q.k5occ = c.first;
    q.S = imax(1, imin(c.N * q.nbz * q.nby * q.nbx, 512 / tiles));
    q.slots = q.kernel == WGRAD_POINT ? q.S * 4 : q.S;
    q.grid_x = q.S; q.grid_y = tiles;
    const int BV = q.BZ * q.BY * q.BX, HV = q.HZ * q.HY * q.HX;
    q.lds = ((size_t)BV * 32 + (size_t)HV * (c.first ? 4 : 32)) * sizeof(float);
    q.ws_floats = (size_t)q.slots * tiles * q.groups * 1024;
    if (q.lds > LDS_MAX) return refuse(q, LDS_TILE);
    if (h16 && !((q.kernel == WGRAD_TAPS && c.ks == 2 && c.in_h) || (c.first && !c.in_h))) return refuse(q, BF16_NO_KERNEL);
    if (!c.first && c.ks > 3) return refuse(q, KS_UNSUPPORTED);
    // the kernel's per-thread item tables: 8 dY items, 20 input items (5 in the first layer's form)
    if (BV > 256 || (c.first ? HV > 5 * 256 : HV * 8 > 20 * 256) || q.HX > 255 || q.HY > 255 || q.HZ > 255) return refuse(q, ITEM_TABLES);
    return q;
}

// What a caller that knows the geometry but not yet the operands reserves: the largest ws_floats over the plans it can reach - with
// and without the split-fp16 kernels, every storage combination, and the (pad, input extent) variants the conditions above tell apart
// (pad 1 / same extents, pad 0 / same extents, pad 0 / twice the extents; everything else plans like one of them).  Refused plans count:
// they are sized like the kernel that would have run.
inline size_t reserve_floats(int N, int OD, int OH, int OW, int M, int Nc, int ks, int stride, const Switches& sw) {
    size_t a = 0;
    for (int v = 0; v < 24; ++v) {
        const int geom = v % 3, us = geom == 2 ? 2 : 1;
        const Call c = {N, OD, OH, OW, us * OD, us * OH, us * OW, M, Nc, ks, stride, geom == 0 ? 1 : 0, (v / 3 & 1) != 0, (v / 6 & 1) != 0, (v / 12 & 1) != 0, false};
        const size_t f = plan(c, sw).ws_floats;
        if (f > a) a = f;
    }
    return a;
}

// ---- first layer ---------------------------------------------------------------------------------------------------------------------
inline Call first_call(int N, int G, int M, bool dy_h) { return {N, G, G, G, G, G, G, M, 4, 5, 1, 2, false, false, dy_h, true}; }

// The sparse forms' workspace (float offsets): dysum [G^3][M], the frame sum of dY | zocc [G^3], an empty occupancy grid | dense_ws, the
// partial sums of the dense kernel on that one frame | part [N * chunks][125][M], the occupancy channel's partial sums
struct FirstLayout {
    size_t dysum, zocc, dense_ws, part, total;
    int chunks;
};
inline FirstLayout first_layout(int N, int G, int M, const Switches& sw) {
    auto r64 = [](size_t n) { return (n + 63) & ~(size_t)63; };
    const size_t G3 = (size_t)G * G * G;
    FirstLayout l;
    l.chunks = (int)((G3 + K5S_CHUNK_VOXELS - 1) / K5S_CHUNK_VOXELS);
    l.dysum = 0; l.zocc = G3 * M; l.dense_ws = l.zocc + r64(G3); l.part = l.dense_ws + r64(plan(first_call(1, G, M, false), sw).ws_floats);
    l.total = l.part + (size_t)N * l.chunks * 125 * M;
    return l;
}
// the sparse forms' layout, or the dense form over all frames (other channel counts, sparse_occ 0)
inline size_t first_reserve_floats(int N, int G, int M, const Switches& sw) {
    const size_t dense = plan(first_call(N, G, M, false), sw).ws_floats, sparse = first_layout(N, G, M, sw).total;
    return dense > sparse ? dense : sparse;
}

}  // namespace nm_wgrad
