// conv3(upsample2(x)) evaluated on the coarse grid: the decoder's two resolution-doubling layers
// (model/kypt_detector.py:425-447: nn.Upsample(x2, trilinear, align_corners=False) followed by Conv3d(k3, p1)).
//
// Trilinear x2 is linear and, away from the volume border, periodic with period 2: a fine output voxel o = 2i + p (parity
// p per axis) reads the three coarse voxels i-1, i, i+1 along each axis.  Per axis the fine taps t = -1, 0, +1 of the conv
// land on coarse offsets d = -1, 0, +1 with the weights
//      p = 0:  t=-1 -> (.75, .25, 0)    t=0 -> (.25, .75, 0)    t=+1 -> (0, .75, .25)
//      p = 1:  t=-1 -> (.25, .75, 0)    t=0 -> (0, .75, .25)    t=+1 -> (0, .25, .75)
// so  out[2i+p] = sum_{d, c} C_p[d][c] * a[i+d][c]  with the composite weights  C_p[d] = sum_t Uz[pz][tz][dz] Uy[..] Ux[..] w[t]:
// eight 3x3x3 convolutions of the ACTIVATED COARSE tensor, one per parity class, and no interpolation arithmetic at all.  That is
// the fine convolution's MAC count, 8 x 27 products per coarse voxel - of which the result needs 27: the channel contraction commutes
// with the interpolation, so the products can be taken once per coarse voxel and RAW tap and interpolated afterwards.  The split-fp16
// mode does that along y (conv_up2y_kernel below: 4 x 27 per coarse voxel + one halo cell per side of a COLUMN of bricks along y:
// a workgroup marches along y and carries the halo products from brick to brick).  Two composite kernels remain, each with one kind of
// arithmetic: conv_up2c_kernel is the main kernel of the one-product modes (fp32 and bfloat16 storage), conv_up2c_x16_kernel the
// split-fp16 composite form behind NM355_UP2Y=0 (the A/B arm and the tests' exact reference of the product form).  The coarse halo
// tile of a brick is 8x smaller than the fine one: the input channels of a (2+2) x (8+2) x (8+2) coarse tile sit in LDS, 32 at a
// time in two buffers (split fp16 hi/lo), staged while the previous group's k-steps run, and the k-steps of the brick's eight parity
// classes run from it with two barriers per 32-channel group.
//
// Machine mapping: one 512-thread workgroup per CU, wave w = parity class (pz,py,px) = bits of w, 2z x 8y x 8x coarse cells = 128
// rows x 32 output channels per wave.  conv_up2c_kernel: 4 row tiles of v_mfma_f32_32x32x16_f16, one hi x hi product per MAC;
// conv_up2c_x16_kernel: 8 row tiles x 2 column blocks of v_mfma_f32_16x16x32_f16 with the 3-product hi/lo split of nm_conv.hip
// (fp32-equivalent products, fp32 accumulate) in one accumulator.  Each wave streams ITS parity's weights from L2, prefetched ahead
// of their k-step; the row tiles are dealt to the lanes so that each lane group of a ds_read_b128 hits 16 distinct 16-byte slots
// (z-plane pitch = 8 mod 16 slots).
//
// Volume border.  The coarse tile is staged with clamped indices, which reproduces torch's clamped interpolation for every fine
// position INSIDE the volume.  The fine convolution, however, zero-pads: taps that leave the fine volume must contribute nothing,
// whereas the composite form gives them the interpolated value f~ of the clamped tile.  For the outer one-voxel shell of the output
//      true = composite - sum_{taps t that leave the volume} w[t] f~[o+t]
// and by inclusion-exclusion over the border axes S of the voxel the subtracted sum is a signed sum of small convolutions of the
// coarse tensor (axes in S: the single outward tap, which reads the voxel's own coarse cell with weight 1; the other axes: the
// interior composite) - 9, 3 or 1 coarse taps.  conv_up2c_shell_kernel applies them to the shell (9 % of the voxels, 3 % of the
// MACs) after the main kernel and owns the shell's GroupNorm partial sums; the main kernel leaves the shell out of its own.
// Along an axis with RAW taps the padding needs no correction: the outward tap's products are simply left out of the interpolation.
// conv_up2y_kernel does that along y, so with it as the main kernel the y faces are final after the main launch (and counted in
// its partial sums): the shell keeps the z and x faces, and on the edges and corners every subset of border axes except {y}.
#include "nm_up2c.h"

namespace {

#define UP2C_SB() __builtin_amdgcn_sched_barrier(0)
#define UP2C_SPLIT_SCALE 2048.0f          // same hi/lo split as nm_conv.hip: v = hi + lo * 2^-11
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// the brick (BZ, BY, BX), its halo tile and LDS planes (HZ, HY, HX, ZP, HVP, CG, NPLANES, LDS_BYTES), the face kernels' line pitch (FP,
// face_fpv) and conv_up2y_kernel's row tiles (YT): nm_conv_plan.h, where the launch plan reads them too
using namespace nm_conv_plan::up2c;

// (16-byte aligned: 128 bytes of kernel arguments, so the shell kernels' trailing ints start on a 16-byte boundary and arrive in one
//  aligned scalar load)
struct alignas(16) Up2cParams {
    const float* in; const float* in_scale; const float* in_shift; float in_slope;
    int N, ID, IH, IW, Cin;
    const half8* wc;             // composite sets (see set_offset)
    const half8* wy;             // the four (pz, px) sets of conv_up2y_kernel (behind the composite sets)
    const float* bias; float* out; float* part;
    int Cout, Co_pad;
    int nbz, nby, nbx;           // bricks per frame
    int nblk;                    // partial blocks per frame (bricks + shell items)
    int march;                   // conv_up2y_kernel<true> is launched: workgroups take whole columns of bricks along y and carry the two halo row tiles
    int ypad;                    // conv_up2y_kernel is the main kernel and zero-pads along y itself: the y faces are not the shell kernels'
};

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, half8& hi, half8& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v0 = (j < 2) ? a[2 * j] : b[2 * j - 4], v1 = (j < 2) ? a[2 * j + 1] : b[2 * j - 3];
        half2v hh = __builtin_convertvector(f32x2{v0, v1}, half2v);
        asm volatile("" : "+v"(hh));
        const float t0 = v0 * UP2C_SPLIT_SCALE, t1 = v1 * UP2C_SPLIT_SCALE;
        hi[2 * j] = hh[0]; hi[2 * j + 1] = hh[1];
        lo[2 * j] = (_Float16)__builtin_fmaf((float)hh[0], -UP2C_SPLIT_SCALE, t0);
        lo[2 * j + 1] = (_Float16)__builtin_fmaf((float)hh[1], -UP2C_SPLIT_SCALE, t1);
    }
}

// pending GroupNorm affine + LeakyReLU of the producer (TensorRef semantics of nm_common.h)
__device__ __forceinline__ f32x4 act4(f32x4 v, const f32x4& sc, const f32x4& sh, bool affine, float slope) {
    if (affine) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(v[j], sc[j], sh[j]);
    }
    if (slope != 1.0f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], v[j] * slope);
    }
    return v;
}

// 16-bit storage (conv mode 4): eight bfloat16 channels arrive as ONE 16-byte load (kept raw in an f32x4) and are widened where
// they are used; IH = false: the two fp32 quads as before
template <bool IH>
__device__ __forceinline__ void ld8_raw(const float* base, size_t e, f32x4& a, f32x4& b) {
    if constexpr (IH) a = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned short*>(base) + e);
    else { a = *reinterpret_cast<const f32x4*>(base + e); b = *reinterpret_cast<const f32x4*>(base + e + 4); }
}
template <bool IH>
__device__ __forceinline__ void widen8(f32x4& a, f32x4& b) {
    if constexpr (IH) {
        const unsigned u0 = nm_fbits(a[0]), u1 = nm_fbits(a[1]), u2 = nm_fbits(a[2]), u3 = nm_fbits(a[3]);
        a = f32x4{nm_bf_lo(u0), nm_bf_hi(u0), nm_bf_lo(u1), nm_bf_hi(u1)};
        b = f32x4{nm_bf_lo(u2), nm_bf_hi(u2), nm_bf_lo(u3), nm_bf_hi(u3)};
    }
}

// ---- composite weight sets -------------------------------------------------------------------------------------------------
// set e: e < 8: S = {} (main), parity p = e (pz = e>>2, py = (e>>1)&1, px = e&1); else S = 1 + (e-8)/8 as a bit mask
// (x = 1, y = 2, z = 4) of the axes whose tap leaves the volume, p = (e-8) % 8.  A set holds 3^(free axes) coarse taps (z, y, x
// order over the free axes, d = -1, 0, +1) as [Cin/16][tap][hi h0 | hi h1 | lo h0 | lo h1][Co_pad][8 halves]: the k-steps of a
// set (channel chunk outer, tap inner) are one linear walk through memory.
__host__ __device__ inline int set_axes(int e) { return e < 8 ? 0 : 1 + (e - 8) / 8; }
__host__ __device__ inline int set_parity(int e) { return e < 8 ? e : (e - 8) % 8; }
__host__ __device__ inline int axes_taps(int S) { int t = 27; if (S & 1) t /= 3; if (S & 2) t /= 3; if (S & 4) t /= 3; return t; }
// offset of set e in units of one tap (C16 * 4 * Co_pad half8)
__host__ __device__ inline int set_tap_offset(int e) {
    int off = 0;
    for (int i = 0; i < e; ++i) off += axes_taps(set_axes(i));
    return off;
}
constexpr int TOTAL_TAPS = 8 * 27 + 8 * (3 * 9 + 3 * 3 + 1);      // 512

__device__ __forceinline__ double ucoef(int p, int t, int d) {      // weight of coarse offset d-1 in fine tap t-1, parity p
    // in quarters; p = 0: rows t = (3 1 0) (1 3 0) (0 3 1);  p = 1: (1 3 0) (0 3 1) (0 1 3)
    const int T0[9] = {3, 1, 0, 1, 3, 0, 0, 3, 1}, T1[9] = {1, 3, 0, 0, 3, 1, 0, 1, 3};
    int v = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) if (i == t * 3 + d) v = p ? T1[i] : T0[i];
    return 0.25 * (double)v;
}

__global__ void up2c_compose_kernel(const float* __restrict__ w, int Cout, int Cin, int Co_pad, _Float16* __restrict__ packed) {
    const int C16 = Cin >> 4;
    const size_t per_tap = (size_t)C16 * 2 * Co_pad * 8;          // (cb, hh, co, j) elements, each writing hi and lo
    const size_t total = (size_t)TOTAL_TAPS * per_tap;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = i & 7; size_t r = i >> 3;
        const int co = r % Co_pad; r /= Co_pad;
        const int hh = r & 1; r >>= 1;
        const int cb = r % C16; int gt = (int)(r / C16);             // global tap index over all sets
        int e = 0;
        for (;; ++e) { const int nt = axes_taps(set_axes(e)); if (gt < nt) break; gt -= nt; }
        const int S = set_axes(e), p = set_parity(e);
        const int pa[3] = {p & 1, (p >> 1) & 1, (p >> 2) & 1};       // x, y, z parities
        int d[3] = {1, 1, 1};                                        // coarse offsets + 1 (x, y, z); axes in S stay at 0 offset
        {   // decode the tap over the free axes, z slowest
            int q = gt;
            for (int a = 0; a < 3; ++a) if (!((S >> a) & 1)) { d[a] = q % 3; q /= 3; }
        }
        const int ci = cb * 16 + hh * 8 + j;
        double v = 0.0;
        if (co < Cout && ci < Cin) {
            const float* wk = w + ((size_t)co * Cin + ci) * 27;
            for (int tz = 0; tz < 3; ++tz) for (int ty = 0; ty < 3; ++ty) for (int tx = 0; tx < 3; ++tx) {
                const int t[3] = {tx, ty, tz};
                double c = 1.0;
                for (int a = 0; a < 3; ++a) {
                    if ((S >> a) & 1) { if (t[a] != (pa[a] ? 2 : 0)) c = 0.0; }      // the single tap that leaves the volume
                    else c *= ucoef(pa[a], t[a], d[a]);
                }
                if (c != 0.0) v += c * (double)wk[(tz * 3 + ty) * 3 + tx];
            }
            const int bits = (S & 1) + ((S >> 1) & 1) + ((S >> 2) & 1);
            if (bits & 1) v = -v;                                    // inclusion-exclusion sign (-1)^|S|
        }
        const float vf = (float)v;
        const _Float16 hi = (_Float16)vf;
        const _Float16 lo = (_Float16)((vf - (float)hi) * UP2C_SPLIT_SCALE);
        // position inside the set: [chunk][tap], taps in the order they were decoded (gt)
        const size_t base = (((size_t)set_tap_offset(e) * C16) + (size_t)cb * axes_taps(S) + gt) * 4 * Co_pad * 8;
        packed[base + ((size_t)hh * Co_pad + co) * 8 + j] = hi;
        packed[base + ((size_t)(2 + hh) * Co_pad + co) * 8 + j] = lo;
    }
}

// The four sets of conv_up2y_kernel, behind the TOTAL_TAPS composite ones: class (pz, px), composite along z and x only, the RAW
// taps along y.  Same layout as a composite set with the 27 'taps' u = (dz * 3 + dx) * 3 + ty.
constexpr int YSETS = 4;
__global__ void up2y_compose_kernel(const float* __restrict__ w, int Cout, int Cin, int Co_pad, _Float16* __restrict__ packed) {
    const int C16 = Cin >> 4;
    const size_t per_tap = (size_t)C16 * 2 * Co_pad * 8;
    const size_t total = (size_t)YSETS * 27 * per_tap;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = i & 7; size_t r = i >> 3;
        const int co = r % Co_pad; r /= Co_pad;
        const int hh = r & 1; r >>= 1;
        const int cb = r % C16; const int gu = (int)(r / C16);
        const int cls = gu / 27, u = gu % 27, ty = u % 3, dx = (u / 3) % 3, dz = u / 9;
        const int pz = cls >> 1, px = cls & 1;
        const int ci = cb * 16 + hh * 8 + j;
        double v = 0.0;
        if (co < Cout && ci < Cin) {
            const float* wk = w + ((size_t)co * Cin + ci) * 27;
            for (int tz = 0; tz < 3; ++tz) for (int tx = 0; tx < 3; ++tx) {
                const double c = ucoef(pz, tz, dz) * ucoef(px, tx, dx);
                if (c != 0.0) v += c * (double)wk[(tz * 3 + ty) * 3 + tx];
            }
        }
        const float vf = (float)v;
        const _Float16 hi = (_Float16)vf;
        const _Float16 lo = (_Float16)((vf - (float)hi) * UP2C_SPLIT_SCALE);
        const size_t base = (((size_t)(TOTAL_TAPS + cls * 27) * C16) + (size_t)cb * 27 + u) * 4 * Co_pad * 8;
        packed[base + ((size_t)hh * Co_pad + co) * 8 + j] = hi;
        packed[base + ((size_t)(2 + hh) * Co_pad + co) * 8 + j] = lo;
    }
}

// ---- main kernel -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ constexpr int tap_off(int t) { return (t / 9) * ZP + ((t / 3) % 3) * HX + (t % 3); }

// One STEP = (brick, 32-output-channel group, 32-input-channel group): 2 chunks x 27 taps = 54 k-steps of 4 MFMAs per wave on
// the LDS buffer `cur`.  The tile of the NEXT step is staged into the other buffer from inside the k-loop: each thread owns up to
// four (voxel, channel octet) items; an item's global loads are issued a dozen k-steps before its activate / split / LDS write,
// so neither the load latency nor the conversion VALU is exposed - they run in the shadow of the two waves' MFMAs (a loop that
// only issues MFMAs and LDS reads keeps the pipe ~100 % busy; staged as a separate phase the same work cost 22 % of the kernel:
// one workgroup per CU has nothing else to run meanwhile).  Two workgroup barriers per step.
struct StepPos { int n, br, nh, cg, cz0, cy0, cx0; };

// The main kernel of the one-product modes (conv modes 3 / 4): ONE fp16 product per MAC, so only the hi planes of the LDS image and
// the hi halves of the packed weights are touched.
// IO: bit 0 = bfloat16 input, bit 1 = bfloat16 output (16-bit storage; the shell kernels then read-modify-write bfloat16 values)
template <int IO>
__global__ __launch_bounds__(512, 1) void conv_up2c_kernel(Up2cParams p) {
    constexpr bool IH16 = (IO & 1) != 0, OH16 = (IO & 2) != 0;
    extern __shared__ f32x4 lds_raw[];
    half8* tile = reinterpret_cast<half8*>(lds_raw);               // [buffer][chunk*4 + hl*2 + h][HVP] x 16 B, slot = hz*ZP + hy*HX + hx

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const int pz = wave >> 2, py = (wave >> 1) & 1, px = wave & 1;
    const int C16 = p.Cin >> 4, NCG = p.Cin / CG, NH = p.Cout >> 5;
    const size_t plane = (size_t)p.Co_pad;
    const size_t kstride = 4 * plane;                             // half8 units between consecutive k-steps of a set
    const half8* __restrict__ wset = p.wc + (size_t)wave * 27 * C16 * kstride;      // wave-uniform
    const unsigned wlane = (unsigned)(h * (int)plane + l31) * 16u;                  // per-lane byte offset of every weight load
    const size_t kbytes = kstride * 16;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    // A rows of this lane (16-byte slots, lane half's plane included): tile j covers y in {2j, 2j+1}.  A ds_read_b128 is served in
    // the lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} (quads {0,3,5,6} / {1,2,4,7} of a lane half): a group's four quads are
    // the four (x half, z) combinations of ONE y, i.e. slot bases 0, 4, 8, 12 (+10 for the other y) mod 16 - conflict-free.
    //   row l31:  x = 4 * bit3 + (l31 & 3),  z = bit4,  y = 2j + ((0x96 >> (l31 >> 2)) & 1)
    int arow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        arow[j] = h * HVP + ((l31 >> 4) & 1) * ZP + (2 * j + ((0x96 >> (l31 >> 2)) & 1)) * HX + 4 * ((l31 >> 3) & 1) + (l31 & 3);
    // staging role: channel octet tid & 3 of the 32-channel group, tile voxels tid/4 + 128 k
    const int s_oct = tid & 3;
    const int s_plane = (s_oct >> 1) * 4 + (s_oct & 1);
    constexpr int NV = HZ * HY * HX, SITEMS = (NV * 4 + 511) / 512;       // 4 items per thread (the last one for 64 threads only)
    const bool affine = p.in_scale != nullptr;

    const int bricks = p.nbz * p.nby * p.nbx, total = p.N * bricks;
    const int per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int item0 = (int)blockIdx.x * per, item_end = min(total, item0 + per);
    if (item0 >= item_end) return;
    auto pos_of = [&](int item, int nh, int cg) {
        StepPos s; s.n = item / bricks; s.br = item % bricks; s.nh = nh; s.cg = cg;
        s.cx0 = (s.br % p.nbx) * BX; s.cy0 = ((s.br / p.nbx) % p.nby) * BY; s.cz0 = (s.br / (p.nbx * p.nby)) * BZ;
        return s;
    };
    // staging of one item: loads (issue) and activate / split / write (commit)
    f32x4 pr_a, pr_b, sca, scb, sha, shb;
    sca = scb = sha = shb = pr_a = pr_b = f32x4{0.f, 0.f, 0.f, 0.f};
    auto issue_affine = [&](const StepPos& s) {
        if (affine) {
            const int cbase = s.cg * CG + s_oct * 8;
            const float* ps = p.in_scale + (size_t)s.n * p.Cin + cbase; const float* ph = p.in_shift + (size_t)s.n * p.Cin + cbase;
            sca = *reinterpret_cast<const f32x4*>(ps); scb = *reinterpret_cast<const f32x4*>(ps + 4);
            sha = *reinterpret_cast<const f32x4*>(ph); shb = *reinterpret_cast<const f32x4*>(ph + 4);
        }
    };
    auto issue = [&](const StepPos& s, int k) {
        // the item's voxel index (tid >> 2) + 128 k, computed HERE by an opaque instruction pair: as a plain expression it is
        // loop-invariant, hipcc hoists it, keeps the four of them (k = 0..3) alive across the k-loop and - at 256 registers - spills
        // them; every reload was followed by s_waitcnt vmcnt(0), i.e. drained the weight loads in flight (8 drains per step)
        int v;
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < NV) {
            const int hx = v % HX, hy = (v / HX) % HY, hz = v / (HX * HY);
            const int gz = min(max(s.cz0 - 1 + hz, 0), p.ID - 1), gy = min(max(s.cy0 - 1 + hy, 0), p.IH - 1), gx = min(max(s.cx0 - 1 + hx, 0), p.IW - 1);
            ld8_raw<IH16>(p.in, ((((size_t)s.n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + s.cg * CG + s_oct * 8, pr_a, pr_b);
        }
    };
    auto commit = [&](half8* buf, int k) {
        int v;
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < NV) {
            const int hx = v % HX, hy = (v / HX) % HY, hz = v / (HX * HY);
            half8 hi, lo;
            widen8<IH16>(pr_a, pr_b);
            split8(act4(pr_a, sca, sha, affine, p.in_slope), act4(pr_b, scb, shb, affine, p.in_slope), hi, lo);
            const int slot = hz * ZP + hy * HX + hx;
            buf[s_plane * HVP + slot] = hi;      // (the lo planes keep their place in the image and stay unwritten: nothing reads them)
        }
    };
    auto ldw = [&](const char* base, size_t extra) { return *reinterpret_cast<const half8*>(base + extra + wlane); };

    // first tile: staged in the open
    StepPos cs = pos_of(item0, 0, 0);
    issue_affine(cs);
#pragma unroll
    for (int k = 0; k < SITEMS; ++k) { issue(cs, k); commit(tile, k); }
    lds_barrier();
    int cur = 0, item = item0;
    f32x16 acc[4];
    // The k-steps of consecutive steps form ONE software-pipelined stream: the B operands (two k-steps ahead) and the A operands
    // (one ahead) of a step's first k-steps are fetched during the last k-steps of the step before it, so a step boundary costs no
    // pipeline refill.  Two workgroup barriers per step keep the two LDS buffers apart: at k-step 10 (before this step's first
    // write into the other buffer: every wave has left the previous step, which read that buffer) and at k-step 51 (after the last
    // write: the other buffer is complete before the first read of the next step is issued at k-step 53).
    constexpr int KS = CG / 16 * 27;                                  // k-steps per step (54)
    const char* wk = reinterpret_cast<const char*>(wset);              // (cs.nh = cs.cg = 0)
    half8 bh[3], ah[4];
    bh[0] = ldw(wk, 0);
    bh[1] = ldw(wk, kbytes);
#pragma unroll
    for (int j = 0; j < 4; ++j) ah[j] = tile[arow[j]];
    for (;;) {
        // the step after this one
        StepPos ns = cs; bool have_next = true;
        if (cs.cg + 1 < NCG) ns.cg = cs.cg + 1;
        else if (cs.nh + 1 < NH) { ns.nh = cs.nh + 1; ns.cg = 0; }
        else if (item + 1 < item_end) ns = pos_of(item + 1, 0, 0);
        else have_next = false;
        if (cs.cg == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        }
        const half8* tb = tile + cur * (NPLANES * HVP);
        half8* nb = tile + (cur ^ 1) * (NPLANES * HVP);
        // weights of the next step's first k-steps (a finished workgroup reads its own first set again: any valid address)
        const char* wnext = reinterpret_cast<const char*>(wset + (size_t)ns.nh * 32 + (size_t)(ns.cg * (CG / 16)) * 27 * kstride);
        if (have_next) issue_affine(ns);
#pragma unroll
        for (int c = 0; c < CG / 16; ++c) {
#pragma unroll
            for (int t = 0; t < 27; ++t) {
                const int ks = c * 27 + t, s = ks % 3, s2 = (ks + 2) % 3;
                if (ks + 2 < KS) bh[s2] = ldw(wk, 2 * kbytes);
                else bh[s2] = ldw(wnext, (size_t)(ks + 2 - KS) * kbytes);
                wk += kbytes;
                // staging pieces of the next tile: item i loaded at k-step 1 + 13 i, written at 11 + 13 i
                if (have_next) {
#pragma unroll
                    for (int i = 0; i < SITEMS; ++i) {
                        if (ks == 1 + 13 * i) issue(ns, i);
                        if (ks == 11 + 13 * i) commit(nb, i);
                    }
                }
                if (have_next && (ks == 10 || ks == 51)) lds_barrier();
                UP2C_SB();
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bh[s], acc[j], 0, 0, 0);
                UP2C_SB();
                // A operands of the next k-step (after the last one: tap 0 of the other buffer)
                const half8* xb = (ks == KS - 1) ? nb : tb;
                const int nof = (ks == KS - 1) ? 0 : ((t < 26) ? c * 4 * HVP + tap_off((t + 1) % 27) : (c + 1) * 4 * HVP);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ah[j] = xb[arow[j] + nof];
                    UP2C_SB();
                }
            }
        }
        wk = wnext;
        if (cs.cg == NCG - 1) {
            // ---- epilogue of this 32-channel group: bias, store, GroupNorm partials
            // without the shell (one slot per wave)
            const int co = cs.nh * 32 + l31;
            const float bv = p.bias ? p.bias[co] : 0.f;
            float s = 0.f, ss = 0.f;
            const size_t sX = (size_t)p.Cout, sY = (size_t)OW * sX, sZ = (size_t)OH * sY;
            const bool border_brick = cs.cz0 == 0 || cs.cz0 + BZ == p.ID || cs.cy0 == 0 || cs.cy0 + BY == p.IH || cs.cx0 == 0 || cs.cx0 + BX == p.IW;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float* base = nm_eptr(p.out, ((((size_t)cs.n * OD + 2 * cs.cz0 + pz) * OH + 2 * (cs.cy0 + 2 * j) + py) * OW + 2 * cs.cx0 + px) * sX + co, OH16);
                if constexpr (OH16) {
                    // bfloat16: the lanes of neighbouring channels exchange values so that each stores ONE packed dword per register pair
                    // (even lanes the channel pair of row r, odd lanes of row r + 1 - one x step further)
                    const bool odd = (l31 & 1) != 0;
                    unsigned short* bq = reinterpret_cast<unsigned short*>(base) - (odd ? 1 : 0);
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const int x = 4 * ((r >> 2) & 1) + (r & 3), zb = (r >> 3) & 1, yb = (0x96 >> (h + 2 * (r >> 2))) & 1;
                        const float v0 = acc[j][r] + bv;
                        const float v1 = acc[j][r + 1] + bv;
                        const float send = odd ? v0 : v1;
                        const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xf, 0xf, true));
                        const unsigned pk = odd ? nm_pk_bf16(recv, v1) : nm_pk_bf16(v0, recv);
                        *reinterpret_cast<unsigned*>(bq + (size_t)(2 * zb) * sZ + (size_t)(2 * yb) * sY + (size_t)(2 * (x + (odd ? 1 : 0))) * sX) = pk;
                        float m0 = v0, m1 = v1;
                        if (border_brick) {
                            const int oz = 2 * (cs.cz0 + zb) + pz, oy = 2 * (cs.cy0 + 2 * j + yb) + py, ox0 = 2 * (cs.cx0 + x) + px, ox1 = ox0 + 2;
                            const bool zy = oz == 0 || oz == OD - 1 || oy == 0 || oy == OH - 1;
                            if (zy || ox0 == 0 || ox0 == OW - 1) m0 = 0.f;
                            if (zy || ox1 == 0 || ox1 == OW - 1) m1 = 0.f;
                        }
                        s += m0; ss = __builtin_fmaf(m0, m0, ss);
                        s += m1; ss = __builtin_fmaf(m1, m1, ss);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else if (!border_brick) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // register r of lane half h is row (r & 3) + 4 h + 8 (r >> 2) of the tile (see arow)
                        const int x = 4 * ((r >> 2) & 1) + (r & 3), zb = (r >> 3) & 1, yb = (0x96 >> (h + 2 * (r >> 2))) & 1;
                        const float v = acc[j][r] + bv;
                        base[(size_t)(2 * zb) * sZ + (size_t)(2 * yb) * sY + (size_t)(2 * x) * sX] = v;
                        s += v; ss = __builtin_fmaf(v, v, ss);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int x = 4 * ((r >> 2) & 1) + (r & 3), zb = (r >> 3) & 1, yb = (0x96 >> (h + 2 * (r >> 2))) & 1;
                        const float v = acc[j][r] + bv;
                        base[(size_t)(2 * zb) * sZ + (size_t)(2 * yb) * sY + (size_t)(2 * x) * sX] = v;
                        const int oz = 2 * (cs.cz0 + zb) + pz, oy = 2 * (cs.cy0 + 2 * j + yb) + py, ox = 2 * (cs.cx0 + x) + px;
                        const bool shell = oz == 0 || oz == OD - 1 || oy == 0 || oy == OH - 1 || ox == 0 || ox == OW - 1;
                        const float mv = shell ? 0.f : v;
                        s += mv; ss = __builtin_fmaf(mv, mv, ss);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (p.part) {
                s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
                if (h == 0) { float* dst = p.part + (((size_t)cs.n * p.nblk + cs.br * 8 + wave) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
            }
        }
        if (!have_next) break;
        if (ns.cg == 0 && ns.nh == 0) ++item;
        cs = ns; cur ^= 1;
    }
}

// ---- the split-fp16 composite kernel, on v_mfma_f32_16x16x32_f16 (NM355_UP2Y=0) ------------------------------------------------
// Same bricks, same LDS image (hi AND lo planes), same packed weights as conv_up2c_kernel; 3-product arithmetic, and another
// MFMA shape: K = 32 takes BOTH 16-channel chunks of the 32-channel LDS buffer in one instruction, a row tile is 16 rows, a
// column block 16 output channels.  Per wave and tap: 8 row tiles x 2 column blocks x 3 products = 48 MFMAs of 16 cycles (on
// 32x32x16 it would be 2 chunks x 4 tiles x 3 = 24 of 32 cycles) - the same FLOPs, the same operand bytes (16 A reads + 4 B loads
// per tap), a step is 27 k-steps instead of 54.  MI355X_MICROARCH.md 'DVFS give-back' item 7: where the chip holds its clock down under
// matrix load (the three products on 32x32x16: 1.49 GHz, profiles/r05_pmc_mfma.json) it holds a higher one on this shape
// (profiles/r06_mfma_shape_ab.txt; the 32x32x16 arm is retired: DESIGN_HISTORY.md).
//   lane = 16 q + r:  A row r of the tile, k = 8 q + j -> channel (q >> 1) * 16 + (q & 1) * 8 + j of the 32-channel group, i.e. LDS
//   plane (q >> 1) * 4 + hl * 2 + (q & 1);  B column r of the block, the same k -> weight chunk 2 cg + (q >> 1), half q & 1.
// Row tile j = (x parity j & 1, y pair j >> 1):  row r -> x = 2 (r & 3) + (j & 1),  z = r >> 3,  y = 2 (j >> 1) + (bit 2 ^ bit 3 of r).
// A ds_read_b128 is served in the lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} (+32): a group takes rows {0-3,12-15} of one
// plane and rows {4-11} of the NEXT plane (or the other way round); each of the two row sets covers the eight even slots (mod 16)
// - x stride 2, z-plane pitch = 8 (mod 16), y pitch 10 - and consecutive planes are HVP = 1 (mod 16) slots apart: 16 distinct slots.
// C/D: column = lane & 15 (output channel of the block), row = 4 q + reg:  x = 2 reg + (j & 1),  z = q >> 1,  y = 2 (j >> 1) + ((q ^ (q >> 1)) & 1).
__global__ __launch_bounds__(512, 1) void conv_up2c_x16_kernel(Up2cParams p) {
    extern __shared__ f32x4 lds_raw[];
    half8* tile = reinterpret_cast<half8*>(lds_raw);               // [buffer][chunk*4 + hl*2 + h][HVP] x 16 B, slot = hz*ZP + hy*HX + hx

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, r16 = lane & 15;
    const int pz = wave >> 2, py = (wave >> 1) & 1, px = wave & 1;
    const int C16 = p.Cin >> 4, NCG = p.Cin / CG, NH = p.Cout >> 5;
    const size_t plane = (size_t)p.Co_pad;
    const size_t kstride = 4 * plane;                             // half8 units between consecutive taps of a chunk
    const half8* __restrict__ wset = p.wc + (size_t)wave * 27 * C16 * kstride;      // wave-uniform
    const unsigned wlane = (unsigned)((q >> 1) * 27 * (int)kstride + (q & 1) * (int)plane + r16) * 16u;      // per-lane byte offset of every weight load
    const size_t kbytes = kstride * 16, lobytes = 2 * plane * 16;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    // A rows of this lane: tile j adds the compile-time offset 2 (j >> 1) HX + (j & 1)
    const int abase = ((q >> 1) * 4 + (q & 1)) * HVP + (r16 >> 3) * ZP + (((r16 >> 2) ^ (r16 >> 3)) & 1) * HX + 2 * (r16 & 3);
    // staging role: channel octet tid & 3 of the 32-channel group, tile voxels tid/4 + 128 k
    const int s_oct = tid & 3;
    const int s_plane = (s_oct >> 1) * 4 + (s_oct & 1);
    constexpr int NV = HZ * HY * HX, SITEMS = (NV * 4 + 511) / 512;
    const bool affine = p.in_scale != nullptr;

    const int bricks = p.nbz * p.nby * p.nbx, total = p.N * bricks;
    const int per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int item0 = (int)blockIdx.x * per, item_end = min(total, item0 + per);
    if (item0 >= item_end) return;
    auto pos_of = [&](int item, int nh, int cg) {
        StepPos s; s.n = item / bricks; s.br = item % bricks; s.nh = nh; s.cg = cg;
        s.cx0 = (s.br % p.nbx) * BX; s.cy0 = ((s.br / p.nbx) % p.nby) * BY; s.cz0 = (s.br / (p.nbx * p.nby)) * BZ;
        return s;
    };
    // the pending GroupNorm scale / shift of the tile being staged sit in LDS ([scale 32][shift 32] floats behind the two tile
    // buffers; 16 registers less than holding them): written by the first wave's lanes at k-step 3 (loaded at k-step 0), i.e. behind
    // the previous step's barrier at k-step 25 (its last commit was at 24) and before this step's barrier at k-step 4 (first commit at 5)
    float* aff = reinterpret_cast<float*>(tile + 2 * NPLANES * HVP);
    f32x4 pr_a, pr_b;
    pr_a = pr_b = f32x4{0.f, 0.f, 0.f, 0.f};
    float aff_v = 0.f;
    auto aff_load = [&](const StepPos& s) {
        if (affine && tid < 64) aff_v = (tid < 32 ? p.in_scale : p.in_shift)[(size_t)s.n * p.Cin + s.cg * CG + (tid & 31)];
    };
    auto aff_store = [&]() { if (affine && tid < 64) aff[tid] = aff_v; };
    auto issue = [&](const StepPos& s, int k) {
        int v;      // (opaque: see conv_up2c_kernel)
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < NV) {
            const int hx = v % HX, hy = (v / HX) % HY, hz = v / (HX * HY);
            const int gz = min(max(s.cz0 - 1 + hz, 0), p.ID - 1), gy = min(max(s.cy0 - 1 + hy, 0), p.IH - 1), gx = min(max(s.cx0 - 1 + hx, 0), p.IW - 1);
            ld8_raw<false>(p.in, ((((size_t)s.n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + s.cg * CG + s_oct * 8, pr_a, pr_b);
        }
    };
    auto commit = [&](half8* buf, int k) {
        int v;
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < NV) {
            const int hx = v % HX, hy = (v / HX) % HY, hz = v / (HX * HY);
            half8 hi, lo;
            f32x4 sca = {0.f, 0.f, 0.f, 0.f}, scb = sca, sha = sca, shb = sca;
            if (affine) {
                sca = *reinterpret_cast<const f32x4*>(aff + s_oct * 8); scb = *reinterpret_cast<const f32x4*>(aff + s_oct * 8 + 4);
                sha = *reinterpret_cast<const f32x4*>(aff + 32 + s_oct * 8); shb = *reinterpret_cast<const f32x4*>(aff + 32 + s_oct * 8 + 4);
            }
            split8(act4(pr_a, sca, sha, affine, p.in_slope), act4(pr_b, scb, shb, affine, p.in_slope), hi, lo);
            const int slot = hz * ZP + hy * HX + hx;
            buf[s_plane * HVP + slot] = hi;
            buf[(s_plane + 2) * HVP + slot] = lo;
        }
    };
    auto ldw = [&](const char* base, size_t extra) { return *reinterpret_cast<const half8*>(base + extra + wlane); };

    // first tile: staged in the open
    StepPos cs = pos_of(item0, 0, 0);
    aff_load(cs); aff_store();
    lds_barrier();
#pragma unroll
    for (int k = 0; k < SITEMS; ++k) { issue(cs, k); commit(tile, k); }
    lds_barrier();
    int cur = 0, item = item0;
    f32x4 acc[8][2];
    // One software-pipelined stream over the steps as in conv_up2c_kernel: B operands one k-step ahead (three register sets by name,
    // two live: 27 % 3 == 0 keeps the set of a step's first k-step fixed), A operands refilled right after their last use.  Barriers
    // at k-step 4 (before the first write into the other buffer) and 25 (after the last one, before the first read of it at 26).
    constexpr int KS = 27;
    const char* wk = reinterpret_cast<const char*>(wset);              // (cs.nh = cs.cg = 0)
    // A operands: a ring of PAIR slots (pair u = row tiles 2u, 2u + 1: the two x parities of one y pair, one slot apart in LDS); pair
    // u of tap t lives in ring slot (4 t + u) % NRING and is refilled with the pair NRING places further on right after its last MFMA
    constexpr int NRING = 2;
    half8 bh[3][2], bl[3][2], ah[NRING][2], al[NRING][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) { bh[0][nb] = ldw(wk, nb * 256); bl[0][nb] = ldw(wk, nb * 256 + lobytes); }
#pragma unroll
    for (int u = 0; u < NRING; ++u)
#pragma unroll
        for (int x = 0; x < 2; ++x) { ah[u][x] = tile[abase + 2 * u * HX + x]; al[u][x] = tile[abase + 2 * u * HX + x + 2 * HVP]; }
    for (;;) {
        StepPos ns = cs; bool have_next = true;
        if (cs.cg + 1 < NCG) ns.cg = cs.cg + 1;
        else if (cs.nh + 1 < NH) { ns.nh = cs.nh + 1; ns.cg = 0; }
        else if (item + 1 < item_end) ns = pos_of(item + 1, 0, 0);
        else have_next = false;
        if (cs.cg == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[j][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const half8* tb = tile + cur * (NPLANES * HVP);
        half8* nb_ = tile + (cur ^ 1) * (NPLANES * HVP);
        const char* wnext = reinterpret_cast<const char*>(wset + (size_t)ns.nh * 32 + (size_t)(ns.cg * (CG / 16)) * 27 * kstride);
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            const int s = t % 3, s1 = (t + 1) % 3;
            // staging pieces of the next tile: item i loaded at k-step 0 / 7 / 13 / 19, written at 5 / 12 / 18 / 24
            if (have_next) {
                if (t == 0) aff_load(ns);
                if (t == 3) aff_store();
#pragma unroll
                for (int i = 0; i < SITEMS; ++i) {
                    if (t == (i == 0 ? 0 : 6 * i + 1)) issue(ns, i);
                    if (t == (i == 0 ? 5 : 6 * i + 6)) commit(nb_, i);
                }
            }
            if (have_next && (t == 4 || t == 25)) lds_barrier();
            // B operands of the next k-step - requested BEHIND the staging code: a commit waits for its item with vmcnt(0) (the item's
            // loads sit under a condition, so hipcc does not count), which then finds only loads that are a k-step old
            {
                const char* wsrc = (t + 1 < KS) ? wk + kbytes : wnext;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) { bh[s1][nb] = ldw(wsrc, nb * 256); bl[s1][nb] = ldw(wsrc, nb * 256 + lobytes); }
                wk += kbytes;
            }
            // ONE accumulator for the three products: x w 2^11 = x_hi (2^11 w_hi) + x_hi w_lo' + x_lo' w_hi with the lo parts stored
            // times 2^11 as everywhere; 2^11 w_hi is exact in fp16 (|w| < 32) and made here from w_hi (four packed multiplies per block)
            half8 b2k[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) b2k[nb] = bh[s][nb] * (_Float16)UP2C_SPLIT_SCALE;
            UP2C_SB();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rs = (4 * t + u) % NRING;
                // the pair this slot receives next: NRING pairs on, possibly in the next tap (after the last tap: tap 0 of the other buffer)
                const int un = (u + NRING) % 4, tn = t + (u + NRING) / 4;
                const half8* xb = (tn == KS) ? nb_ : tb;
                const int nof = (tn == KS) ? 0 : tap_off(tn);
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc[2 * u + x][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rs][x], b2k[nb], acc[2 * u + x][nb], 0, 0, 0);
                UP2C_SB();
#pragma unroll
                for (int x = 0; x < 2; ++x) {
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc[2 * u + x][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rs][x], bl[s][nb], acc[2 * u + x][nb], 0, 0, 0);
                    ah[rs][x] = xb[abase + 2 * un * HX + x + nof];
                    UP2C_SB();
                }
#pragma unroll
                for (int x = 0; x < 2; ++x) {
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc[2 * u + x][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rs][x], bh[s][nb], acc[2 * u + x][nb], 0, 0, 0);
                    al[rs][x] = xb[abase + 2 * un * HX + x + 2 * HVP + nof];
                    UP2C_SB();
                }
            }
        }
        wk = wnext;
        if (cs.cg == NCG - 1) {
            // ---- epilogue of this 32-channel group: bias, store, GroupNorm partials without the shell (one slot per wave)
            const size_t sX = (size_t)p.Cout;
            const bool border_brick = cs.cz0 == 0 || cs.cz0 + BZ == p.ID || cs.cy0 == 0 || cs.cy0 + BY == p.IH || cs.cx0 == 0 || cs.cx0 + BX == p.IW;
            const int zb = q >> 1, yb = (q ^ (q >> 1)) & 1;
            const int oz = 2 * (cs.cz0 + zb) + pz;
            const bool zshell = oz == 0 || oz == OD - 1;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int co = cs.nh * 32 + nb * 16 + r16;
                const float bv = p.bias ? p.bias[co] : 0.f;
                float s = 0.f, ss = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int oy = 2 * (cs.cy0 + 2 * (j >> 1) + yb) + py;
                    float* base = p.out + ((((size_t)cs.n * OD + oz) * OH + oy) * OW + 2 * (cs.cx0 + (j & 1)) + px) * sX + co;
                    const bool zy = zshell || oy == 0 || oy == OH - 1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[j][nb][r] * (1.0f / UP2C_SPLIT_SCALE) + bv;
                        base[(size_t)(4 * r) * sX] = v;
                        float mv = v;
                        if (border_brick) {
                            const int ox = 2 * (cs.cx0 + 2 * r + (j & 1)) + px;
                            if (zy || ox == 0 || ox == OW - 1) mv = 0.f;
                        }
                        s += mv; ss = __builtin_fmaf(mv, mv, ss);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (p.part) {
                    s += __shfl_xor(s, 16); ss += __shfl_xor(ss, 16);
                    s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
                    if (q == 0) { float* dst = p.part + (((size_t)cs.n * p.nblk + cs.br * 8 + wave) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
                }
            }
        }
        if (!have_next) break;
        if (ns.cg == 0 && ns.nh == 0) ++item;
        cs = ns; cur ^= 1;
    }
}

// ---- the product-then-interpolate form along y ------------------------------------------------------------------------------
// Trilinear upsampling acts per channel and the conv's channel contraction is linear, so along any one axis the two commute:
//      out[2i + p] = sum_d sum_t U[p][t][d] P_t[i + d],     P_t[r] = sum_c W_t[c] a[r][c]   (t the fine tap, r a COARSE cell)
// with U the table at the top of this file.  The composite form spends 2 (parities) x 3 (coarse offsets) products per coarse cell
// and axis; this form spends 3 (the raw taps) on the cells of the brick plus one halo cell per side and pays for it with fp32
// interpolation of the products (weights 1/4, 3/4: exact).  conv_up2y_kernel applies it along y and keeps composite weights along z
// and x: per (pz, px) class 3 x 9 x (BY + 2) products replace 2 x 27 x BY - 10/16 of the MFMAs, the same bricks, the same LDS
// image (staging code shared verbatim with conv_up2c_x16_kernel), the same A-operand reads per brick for FEWER B operands.
//
// Mapping: wave = (pz, px, column block of 16 output channels); a row tile of v_mfma_f32_16x16x32_f16 is ONE coarse y of the halo
// tile (row r -> x = r & 7, z = r >> 3), so the 10 tiles x 3 taps of a lane's accumulators are the SAME (z, x, channel) at the ten
// coarse y's: the interpolation along y is twelve in-lane FMAs per cell and needs no LDS and no cross-lane traffic.  A k-step is one
// coarse (dz, dx) tap of a 32-channel group: 20 A reads, 6 B loads, 90 MFMAs.
// The halo tile is staged with clamped indices, so the halo products at the volume border are those of the clamped cell.  Along z
// and x the kernel computes what the composite kernel computes (zero padding ignored) and the shell kernels below correct it as
// before; along y the epilogue leaves the outward tap's terms out at oy = 0 and oy = OH - 1 (p.ypad; NM355_UP2Y_YPAD=0: the shell
// kernels correct the y faces too), so a voxel on a y face and on no other is final here and part of this kernel's partial sums.
//
// Marching (p.march).  Tiles 8 and 9 of a brick are the cells, the operands and the MFMA sequence of tiles 0 and 1 of its successor
// along y.  A workgroup therefore takes a contiguous range of whole COLUMNS (frame, brick z, brick x) and walks each along y: a
// column's first brick runs all ten tiles, every further one copies acc[..][8..9] to acc[..][0..1] after its predecessor's
// epilogue, stages the rows hy = 2 .. 9 only (320 of 400 cells) and runs tiles 2 .. 9 - (10 + 8 (nby - 1)) / (10 nby) of the MFMAs
// and of the staging, bit for bit the same result.  With two output groups (128 -> 64) the column is marched once per group (step
// order: column, output group, brick, channel group).  Where there are fewer columns than CUs (small extents) every brick is its own
// item as before, and so where whole columns would give the busiest workgroup more row tiles than single bricks do (config 4's
// 128 -> 64 layer: 288 columns on 256 CUs).  NM355_UP2Y_MARCH: 0 never, 2 always marches.
// The GroupNorm partials of class (pz, px), parity py go to slot 8 brick + 4 pz + 2 px + py: the class's two waves fill its two
// column blocks - every slot is written once, in a fixed order.
struct StepPosY : StepPos { int iy; };      // iy: the brick's place in its column (0: all ten row tiles; else tiles 0 and 1 are carried)

template <bool MARCH>
__global__ __launch_bounds__(512, 1) void conv_up2y_kernel(Up2cParams p) {
    extern __shared__ f32x4 lds_raw[];
    half8* tile = reinterpret_cast<half8*>(lds_raw);               // [buffer][chunk*4 + hl*2 + h][HVP] x 16 B, slot = hz*ZP + hy*HX + hx

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, r16 = lane & 15;
    const int cls = wave >> 1, nbw = wave & 1, pz = cls >> 1, px = cls & 1;
    const int C16 = p.Cin >> 4, NCG = p.Cin / CG, NH = p.Cout >> 5;
    const size_t plane = (size_t)p.Co_pad;
    const size_t kstride = 4 * plane;                             // half8 units between consecutive (tap, ty) units of a chunk
    const half8* __restrict__ wset = p.wy + (size_t)cls * 27 * C16 * kstride;       // wave-uniform
    const unsigned wlane = (unsigned)((q >> 1) * 27 * (int)kstride + (q & 1) * (int)plane + nbw * 16 + r16) * 16u;
    const size_t kbytes = kstride * 16, lobytes = 2 * plane * 16;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    // A row of this lane in tile 0, tap 0: tile j adds j * HX, tap (dz, dx) adds dz * ZP + dx.  A lane group of a ds_read_b128 takes
    // rows {0-3, 12-15} of one plane and {4-11} of the next (HVP = 1 mod 16 slots on): 15 distinct slots of 16
    const int abase = ((q >> 1) * 4 + (q & 1)) * HVP + (r16 >> 3) * ZP + (r16 & 7);
    const int s_oct = tid & 3;
    const int s_plane = (s_oct >> 1) * 4 + (s_oct & 1);
    constexpr int NV = HZ * HY * HX, SITEMS = (NV * 4 + 511) / 512;
    const bool affine = p.in_scale != nullptr;

    // an item is a column (frame, brick z, brick x) of L = nby bricks when marching, else one brick (x-fastest, L = 1)
    const int bricks = p.nbz * p.nby * p.nbx, ncol = p.nbz * p.nbx, L = MARCH ? p.nby : 1;
    const int per_frame = MARCH ? ncol : bricks, total = p.N * per_frame;
    const int per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int item0 = (int)blockIdx.x * per, item_end = min(total, item0 + per);
    if (item0 >= item_end) return;
    auto pos_of = [&](int item, int iy, int nh, int cg) {
        StepPosY s; s.n = item / per_frame; s.nh = nh; s.cg = cg; s.iy = iy;
        const int c = item % per_frame;
        s.br = MARCH ? ((c / p.nbx) * p.nby + iy) * p.nbx + c % p.nbx : c;
        s.cx0 = (s.br % p.nbx) * BX; s.cy0 = ((s.br / p.nbx) % p.nby) * BY; s.cz0 = (s.br / (p.nbx * p.nby)) * BZ;
        return s;
    };
    // a carried brick (iy > 0) needs the rows hy = 2 .. 9 only: 320 cells in three items.  The cell of a staging thread follows from
    // five per-step scalars (kept opaque: as selects of constants they were threaded into branches all through the staging code)
    // cells, rows per z plane, 2^16 / (rows * HX) rounded up, first row, slot of cell v = v + hz * zs + y0 * HX
    struct StageMap { int nv, rows, rcp, y0, zs; };
    auto stage_map = [&](bool cr) {
        StageMap m = {cr ? HZ * BY * HX : NV, cr ? BY : HY, cr ? 65536 / (BY * HX) + 1 : 65536 / (HY * HX) + 1, cr ? 2 : 0, cr ? ZP - BY * HX : ZP - HY * HX};
        if constexpr (MARCH) asm volatile("" : "+s"(m.nv), "+s"(m.rows), "+s"(m.rcp), "+s"(m.y0), "+s"(m.zs));
        return m;
    };
    auto cell_of = [&](int v, const StageMap& m, int& hz, int& hy, int& hx) {
        if constexpr (MARCH) { const int vx = v / HX; hx = v - vx * HX; hz = (v * m.rcp) >> 16; hy = vx - hz * m.rows + m.y0; }      // (v < 512)
        else { hx = v % HX; hy = (v / HX) % HY; hz = v / (HX * HY); }
    };
    // staging: as in conv_up2c_x16_kernel (scale / shift of the tile being staged behind the two tile buffers)
    float* aff = reinterpret_cast<float*>(tile + 2 * NPLANES * HVP);
    f32x4 pr_a, pr_b;
    pr_a = pr_b = f32x4{0.f, 0.f, 0.f, 0.f};
    // (both values per lane, selected at the store: a per-lane POINTER select is loop-invariant, 64 bits wide and was spilled)
    float aff_a = 0.f, aff_b = 0.f;
    auto aff_load = [&](const StepPosY& s) {
        if (affine && tid < 64) { const size_t e = (size_t)s.n * p.Cin + s.cg * CG + (tid & 31); aff_a = p.in_scale[e]; aff_b = p.in_shift[e]; }
    };
    auto aff_store = [&]() { if (affine && tid < 64) aff[tid] = tid < 32 ? aff_a : aff_b; };
    auto issue = [&](const StepPosY& s, int k, const StageMap& m) {
        int v;      // (opaque: see conv_up2c_kernel)
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < (MARCH ? m.nv : NV)) {
            int hz, hy, hx; cell_of(v, m, hz, hy, hx);
            const int gz = min(max(s.cz0 - 1 + hz, 0), p.ID - 1), gy = min(max(s.cy0 - 1 + hy, 0), p.IH - 1), gx = min(max(s.cx0 - 1 + hx, 0), p.IW - 1);
            ld8_raw<false>(p.in, ((((size_t)s.n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + s.cg * CG + s_oct * 8, pr_a, pr_b);
        }
    };
    auto commit = [&](half8* buf, int k, const StageMap& m) {
        int v;
        asm volatile("v_lshrrev_b32 %0, 2, %1\n\tv_add_u32 %0, %2, %0" : "=v"(v) : "v"(tid), "s"(128 * k));
        if (v < (MARCH ? m.nv : NV)) {
            half8 hi, lo;
            f32x4 sca = {0.f, 0.f, 0.f, 0.f}, scb = sca, sha = sca, shb = sca;
            if (affine) {
                sca = *reinterpret_cast<const f32x4*>(aff + s_oct * 8); scb = *reinterpret_cast<const f32x4*>(aff + s_oct * 8 + 4);
                sha = *reinterpret_cast<const f32x4*>(aff + 32 + s_oct * 8); shb = *reinterpret_cast<const f32x4*>(aff + 32 + s_oct * 8 + 4);
            }
            split8(act4(pr_a, sca, sha, affine, p.in_slope), act4(pr_b, scb, shb, affine, p.in_slope), hi, lo);
            int slot;
            if constexpr (MARCH) slot = v + ((v * m.rcp) >> 16) * m.zs + m.y0 * HX;
            else { int hz, hy, hx; cell_of(v, m, hz, hy, hx); slot = hz * ZP + hy * HX + hx; }
            buf[s_plane * HVP + slot] = hi;
            buf[(s_plane + 2) * HVP + slot] = lo;
        }
    };
    auto ldw = [&](const char* base, size_t extra) { return *reinterpret_cast<const half8*>(base + extra + wlane); };

    // first tile (a column's first brick, or any brick when not marching: all ten rows): staged in the open
    StepPosY cs = pos_of(item0, 0, 0, 0);
    aff_load(cs); aff_store();
    lds_barrier();
#pragma unroll
    for (int k = 0; k < SITEMS; ++k) { issue(cs, k, stage_map(false)); commit(tile, k, stage_map(false)); }
    lds_barrier();
    int cur = 0, item = item0;
    f32x4 acc[3][YT];
    // One software-pipelined stream over the steps: the B operands of a k-step (three register sets by name, two live; 9 % 3 == 0
    // keeps the set of a step's first k-step fixed) are requested one k-step ahead, an A tile is refilled with the tile NRING places
    // further on right after its last MFMA.  Staging of the next step's tile: item i is loaded at k-step 2 i and written at 2 i + 1;
    // barriers at k-step 1 (before the first write into the other buffer: every wave has left the previous step, which read it) and
    // at k-step 8 (after the last write, before the first read of that buffer by the A refills of this k-step's last tiles).
    constexpr int KS = 9, NRING = 2;
    const char* wk = reinterpret_cast<const char*>(wset);              // (cs.nh = cs.cg = 0)
    half8 bh[3][3], bl[3][3], ah[NRING], al[NRING];
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) { bh[0][ty] = ldw(wk, ty * kbytes); bl[0][ty] = ldw(wk, ty * kbytes + lobytes); }
#pragma unroll
    for (int u = 0; u < NRING; ++u) { ah[u] = tile[abase + u * HX]; al[u] = tile[abase + u * HX + 2 * HVP]; }
    for (;;) {
        // step order: (item, output group, brick in the column, channel group) - the accumulators belong to one output group, so a
        // column is marched once per group
        StepPosY ns = cs; bool have_next = true;
        if (cs.cg + 1 < NCG) ns.cg = cs.cg + 1;
        else if (MARCH && cs.iy + 1 < L) ns = pos_of(item, cs.iy + 1, cs.nh, 0);
        else if (cs.nh + 1 < NH) ns = pos_of(item, 0, cs.nh + 1, 0);
        else if (item + 1 < item_end) ns = pos_of(item + 1, 0, 0, 0);
        else have_next = false;
        // a carried brick holds the products of its row tiles 0 and 1 already (its predecessor's tiles 8 and 9: the same cells, the
        // same operands, the same MFMA chain) and runs the tiles 2 .. 9; the rows 0 and 1 of its LDS image are not staged and not read
        const bool carried = MARCH && cs.iy > 0, ncarried = MARCH && have_next && ns.iy > 0;
        const int coff = carried ? 2 * HX : 0, noff = ncarried ? 2 * HX : 0;       // first row tile of this / the next step
        const StageMap nmap = stage_map(ncarried);
        if (cs.cg == 0) {
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int j = 0; j < YT; ++j) if (j >= 2 || !carried) acc[ty][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const half8* tb = tile + cur * (NPLANES * HVP);
        half8* nb_ = tile + (cur ^ 1) * (NPLANES * HVP);
        const bool stage = have_next;
        const char* wnext = reinterpret_cast<const char*>(wset + (size_t)ns.nh * 32 + (size_t)(ns.cg * (CG / 16)) * 27 * kstride);
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            const int s = t % 3, s1 = (t + 1) % 3;
            if (stage) {
                if (t == 0) aff_load(ns);
                if (t == 1) aff_store();
            }
            if (have_next && (t == 1 || t == 8)) lds_barrier();
            if (stage) {
#pragma unroll
                for (int i = 0; i < SITEMS; ++i) {
                    if (t == 2 * i + 1) commit(nb_, i, nmap);
                    if (t == 2 * i) issue(ns, i, nmap);
                }
            }
            // B operands of the next k-step - requested BEHIND the staging code (see conv_up2c_x16_kernel)
            {
                const char* wsrc = (t + 1 < KS) ? wk + 3 * kbytes : wnext;
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) { bh[s1][ty] = ldw(wsrc, ty * kbytes); bl[s1][ty] = ldw(wsrc, ty * kbytes + lobytes); }
                wk += 3 * kbytes;
            }
            // ONE accumulator for the three products (see conv_up2c_x16_kernel)
            half8 b2k[3];
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) b2k[ty] = bh[s][ty] * (_Float16)UP2C_SPLIT_SCALE;
            UP2C_SB();
#pragma unroll
            for (int j = 0; j < YT; ++j) {
                if (j < 2 && carried) continue;                            // (wave-uniform)
                const int rs = (YT * t + j) % NRING;
                // the slot's next tile: two on, or the first (+ j - 8) tile of the next tap / of the next step's buffer
                const int jn = (j + NRING) % YT, tn = t + (j + NRING) / YT;
                const half8* xb = (tn == KS) ? nb_ : tb;
                const int nof = ((tn == KS) ? 0 : (tn / 3) * ZP + (tn % 3)) + (tn == t ? 0 : (tn == KS ? noff : coff));
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rs], b2k[ty], acc[ty][j], 0, 0, 0);
                UP2C_SB();
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rs], bl[s][ty], acc[ty][j], 0, 0, 0);
                ah[rs] = xb[abase + jn * HX + nof];
                UP2C_SB();
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rs], bh[s][ty], acc[ty][j], 0, 0, 0);
                al[rs] = xb[abase + jn * HX + nof + 2 * HVP];
                UP2C_SB();
            }
        }
        wk = wnext;
        if (cs.cg == NCG - 1) {
            // ---- epilogue of this 32-channel group: interpolation along y (fine y = 2 i + py of coarse cell i reads the tiles i, i + 1,
            // i + 2 = cells i - 1, i, i + 1), bias, store, GroupNorm partials without the shell
            const size_t sX = (size_t)p.Cout;
            const bool border_brick = cs.cz0 == 0 || cs.cz0 + BZ == p.ID || cs.cy0 == 0 || cs.cy0 + BY == p.IH || cs.cx0 == 0 || cs.cx0 + BX == p.IW;
            const int oz = 2 * (cs.cz0 + (q >> 1)) + pz;
            const bool zshell = oz == 0 || oz == OD - 1;
            const int co = cs.nh * 32 + nbw * 16 + r16;
            const float bv = p.bias ? p.bias[co] : 0.f;
            constexpr float C1 = 0.25f / UP2C_SPLIT_SCALE, C3 = 0.75f / UP2C_SPLIT_SCALE;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                float s = 0.f, ss = 0.f;
#pragma unroll
                for (int i = 0; i < BY; ++i) {
                    const int oy = 2 * (cs.cy0 + i) + py;
                    float* base = p.out + ((((size_t)cs.n * OD + oz) * OH + oy) * OW + 2 * (cs.cx0 + 4 * (q & 1)) + px) * sX + co;
                    // zero padding of the fine conv along y: the fine tap that leaves the volume is left out (the remaining terms are
                    // torch's clamped interpolation: the halo tile is staged with clamped indices)
                    const bool ytop = p.ypad && oy == 0, ybot = p.ypad && oy == OH - 1;
                    const bool zy = zshell || (!p.ypad && (oy == 0 || oy == OH - 1));
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v;
                        if (py == 0 && i == 0 && ytop) {
                            v = C1 * acc[1][i][r];
                            v = __builtin_fmaf(C3, acc[1][i + 1][r], v);
                            v = __builtin_fmaf(C3, acc[2][i + 1][r], v);
                            v = __builtin_fmaf(C1, acc[2][i + 2][r], v);
                        } else if (py == 1 && i == BY - 1 && ybot) {
                            v = C1 * acc[0][i][r];
                            v = __builtin_fmaf(C3, acc[0][i + 1][r], v);
                            v = __builtin_fmaf(C3, acc[1][i + 1][r], v);
                            v = __builtin_fmaf(C1, acc[1][i + 2][r], v);
                        } else if (py == 0) {
                            v = C3 * acc[0][i][r];
                            v = __builtin_fmaf(C1, acc[0][i + 1][r], v);
                            v = __builtin_fmaf(C1, acc[1][i][r], v);
                            v = __builtin_fmaf(C3, acc[1][i + 1][r], v);
                            v = __builtin_fmaf(C3, acc[2][i + 1][r], v);
                            v = __builtin_fmaf(C1, acc[2][i + 2][r], v);
                        } else {
                            v = C1 * acc[0][i][r];
                            v = __builtin_fmaf(C3, acc[0][i + 1][r], v);
                            v = __builtin_fmaf(C3, acc[1][i + 1][r], v);
                            v = __builtin_fmaf(C1, acc[1][i + 2][r], v);
                            v = __builtin_fmaf(C1, acc[2][i + 1][r], v);
                            v = __builtin_fmaf(C3, acc[2][i + 2][r], v);
                        }
                        v += bv;
                        base[(size_t)(2 * r) * sX] = v;
                        float mv = v;
                        if (border_brick) {
                            const int ox = 2 * (cs.cx0 + 4 * (q & 1) + r) + px;
                            if (zy || ox == 0 || ox == OW - 1) mv = 0.f;
                        }
                        s += mv; ss = __builtin_fmaf(mv, mv, ss);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (p.part) {
                    s += __shfl_xor(s, 16); ss += __shfl_xor(ss, 16);
                    s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
                    if (q == 0) { float* dst = p.part + (((size_t)cs.n * p.nblk + cs.br * 8 + cls * 2 + py) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
                }
            }
            if (ncarried) {
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) { acc[ty][0] = acc[ty][YT - 2]; acc[ty][1] = acc[ty][YT - 1]; }
            }
        }
        if (!have_next) break;
        if (ns.cg == 0 && ns.nh == 0 && ns.iy == 0) ++item;
        cs = ns; cur ^= 1;
    }
}

// ---- shell kernels -----------------------------------------------------------------------------------------------------------
// Ownership of the shell cells (per parity class): a cell on two or three faces belongs to an EDGE item, every other shell cell to
// the FACE item of its face (with conv_up2y_kernel padding along y, p.ypad: the y-face items own nothing, write empty partial slots
// and leave; the edge items skip the set S = {y}).  A face cell needs one correction set (S = its face's axis, 9 coarse taps); the cells of an edge need
// three (two faces - their common taps), a corner seven.
//
// conv_up2c_face_kernel: one workgroup = one line of 32 cells on a face (along y on the x faces, along x on the y and z faces);
// its four waves are the four parity combinations of the two in-face axes, which read the SAME coarse voxels (3 lines x 34, all
// channels): staged once into LDS (activated, split), then 9 taps x Cin/16 k-steps per wave from LDS with the wave's own weights
// streamed three k-steps ahead.  The result is added to the main kernel's output; the wave writes the GroupNorm partials of its
// voxels' final values.
constexpr int FPV = face_fpv(1);                      // slots per plane: three staged lines of FP slots (34 used)

template <bool SINGLE, int IO = 0>
__global__ __launch_bounds__(256, 4) void conv_up2c_face_kernel(Up2cParams p, int TY, int TX) {
    constexpr bool IH16 = (IO & 1) != 0, OH16 = (IO & 2) != 0;
    extern __shared__ f32x4 lds_raw[];
    half8* tile = reinterpret_cast<half8*>(lds_raw);               // [chunk*4 + hl*2 + h][FPV], slot = across * FP + along
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const int nX = 2 * p.ID * TY, nY = 2 * p.ID * TX, nZ = 2 * p.IH * TX, per_frame = nX + nY + nZ;
    const int n = (int)blockIdx.x / per_frame; int q = (int)blockIdx.x % per_frame;
    const int bricks = p.nbz * p.nby * p.nbx;
    const int slot_part = 8 * bricks + q * 4 + wave;
    // type 0: x face (line along y at z = f), 1: y face (along x at z = f), 2: z face (along x at y = f)
    int type, side, f, tl;
    if (q < nX) { type = 0; tl = q % TY; f = (q / TY) % p.ID; side = q / (TY * p.ID); }
    else if (q < nX + nY) { q -= nX; type = 1; tl = q % TX; f = (q / TX) % p.ID; side = q / (TX * p.ID); }
    else { q -= nX + nY; type = 2; tl = q % TX; f = (q / TX) % p.IH; side = q / (TX * p.IH); }
    if (p.ypad && type == 1) {
        // the main kernel (conv_up2y_kernel) has padded along y itself and counted these voxels: nothing to add, empty partial slots
        if (p.part && lane < 32)
            for (int co = lane; co < p.Cout; co += 32) { float* dst = p.part + (((size_t)n * p.nblk + slot_part) * p.Cout + co) * 2; dst[0] = 0.f; dst[1] = 0.f; }
        return;
    }
    const int LA = type == 0 ? p.IH : p.IW;                            // cells along the line's axis
    const int AC = type == 2 ? p.IH : p.ID;                            // extent of the across axis
    const int fb = side ? (type == 0 ? p.IW : type == 1 ? p.IH : p.ID) - 1 : 0;      // the face's coarse index on its own axis
    const int C16 = p.Cin >> 4, NH = p.Cout >> 5;
    const bool affine = p.in_scale != nullptr;
    // ---- stage 3 lines x 34 voxels x Cin channels ----
    const int noct = p.Cin >> 3, nitems = 3 * 34 * noct;             // (noct divides 256: a thread's channel octet is fixed)
    f32x4 sca = {0.f, 0.f, 0.f, 0.f}, sha = sca, scb = sca, shb = sca;
    if (affine) {
        const int oct = tid % noct;
        const float* ps = p.in_scale + (size_t)n * p.Cin + oct * 8; const float* ph = p.in_shift + (size_t)n * p.Cin + oct * 8;
        sca = *reinterpret_cast<const f32x4*>(ps); scb = *reinterpret_cast<const f32x4*>(ps + 4);
        sha = *reinterpret_cast<const f32x4*>(ph); shb = *reinterpret_cast<const f32x4*>(ph + 4);
    }
    for (int i = tid; i < nitems; i += 256) {
        const int oct = i % noct, v = i / noct, s = v % 34, a = v / 34;
        const int ca = min(max(f + a - 1, 0), AC - 1), cl = min(max(tl * 32 - 1 + s, 0), LA - 1);
        const int gz = type == 2 ? fb : ca, gy = type == 0 ? cl : (type == 1 ? fb : ca), gx = type == 0 ? fb : cl;
        f32x4 va, vb;
        ld8_raw<IH16>(p.in, ((((size_t)n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + oct * 8, va, vb);
        widen8<IH16>(va, vb);
        half8 hi, lo;
        split8(act4(va, sca, sha, affine, p.in_slope), act4(vb, scb, shb, affine, p.in_slope), hi, lo);
        const int pl = (oct >> 1) * 4 + (oct & 1);
        tile[pl * FPV + a * FP + s] = hi;
        tile[(pl + 2) * FPV + a * FP + s] = lo;
    }
    lds_barrier();
    // ---- this wave's parity class, rows, weights ----
    const int pa = wave >> 1, pl_ = wave & 1;                        // parities of the across / along axes
    int pz, py, px;
    if (type == 0) { px = side; pz = pa; py = pl_; } else if (type == 1) { py = side; pz = pa; px = pl_; } else { pz = side; py = pa; px = pl_; }
    const int par = pz * 4 + py * 2 + px;
    const int S = 1 << type;
    const int ab = pa ? AC - 1 : 0, lb = pl_ ? LA - 1 : 0;           // border indices of this class on the two in-face axes
    const bool wave_off = f == ab;                                    // the whole line lies on an edge for this class
    auto row_owned = [&](int rho) { const int u = tl * 32 + rho; return !wave_off && u < LA && u != lb; };
    const size_t plane = (size_t)p.Co_pad, kstride = 4 * plane;
    const int nk = 9 * C16;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    const int arow = h * FPV + l31;
    for (int nh = 0; nh < NH; ++nh) {
        f32x16 acc, accl;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accl[r] = 0.f; }
        if (!wave_off) {
            const half8* wq = p.wc + (size_t)set_tap_offset(8 + (S - 1) * 8 + par) * C16 * kstride + (size_t)h * plane + nh * 32 + l31;
            half8 bh[3], bl[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) { bh[u] = wq[(size_t)min(u, nk - 1) * kstride]; bl[u] = wq[(size_t)min(u, nk - 1) * kstride + 2 * plane]; }
            for (int c = 0; c < C16; ++c) {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int k = c * 9 + t, s = t % 3;
                    const half8 ah = tile[arow + c * 4 * FPV + (t / 3) * FP + (t % 3)];
                    const half8 al = tile[arow + (c * 4 + 2) * FPV + (t / 3) * FP + (t % 3)];
                    const half8 wh = bh[s], wl = bl[s];
                    const int kn = min(k + 3, nk - 1);
                    bh[s] = wq[(size_t)kn * kstride]; bl[s] = wq[(size_t)kn * kstride + 2 * plane];
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wh, acc, 0, 0, 0);
                    accl = nm_mfma_lo<SINGLE>(ah, wl, accl);
                    accl = nm_mfma_lo<SINGLE>(al, wh, accl);
                }
            }
        }
        float s = 0.f, ss = 0.f;
        const int co = nh * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rho = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row_owned(rho)) {
                const int u = tl * 32 + rho;
                const int rz = type == 2 ? fb : f, ry = type == 0 ? u : (type == 1 ? fb : f), rx = type == 0 ? fb : u;
                const size_t dst = ((((size_t)n * OD + 2 * rz + pz) * OH + 2 * ry + py) * OW + 2 * rx + px) * p.Cout + co;
                const float v = nm_ld1<OH16>(p.out, dst) + (acc[r] + accl[r] * (1.0f / UP2C_SPLIT_SCALE));
                nm_st1<OH16>(p.out, dst, v);
                s += v; ss += v * v;
            }
        }
        if (p.part) {
            s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
            if (h == 0) { float* dst = p.part + (((size_t)n * p.nblk + slot_part) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
        }
    }
}

// conv_up2c_edge_kernel: one wave per item = 32 cells of one parity class on one of the twelve edges (the eight corners belong to
// the edges along z).  For every non-empty subset S of a row's border axes the signed set (S, parity) is applied with the rows
// outside the subset's cells zeroed; operands straight from global memory (a few thousand items in all).
template <bool SINGLE, int IO = 0>
__global__ __launch_bounds__(256, 4) void conv_up2c_edge_kernel(Up2cParams p, int TZ, int TY, int TX, int slot0) {
    constexpr bool IH16 = (IO & 1) != 0, OH16 = (IO & 2) != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const int nXY = 8 * TZ, nXZ = 8 * TY, nYZ = 8 * TX, per_frame = nXY + nXZ + nYZ;
    const long long gitem = (long long)blockIdx.x * 4 + wave;
    if (gitem >= (long long)p.N * per_frame) return;
    const int n = (int)(gitem / per_frame); int q = (int)(gitem % per_frame);
    const int slot = slot0 + q;
    // type 0: x-y edge (line along z), 1: x-z edge (along y), 2: y-z edge (along x); q -> (tile, parity class)
    int type, tile, par;
    if (q < nXY) { type = 0; tile = q / 8; par = q % 8; }
    else if (q < nXY + nXZ) { q -= nXY; type = 1; tile = q / 8; par = q % 8; }
    else { q -= nXY + nXZ; type = 2; tile = q / 8; par = q % 8; }
    const int pz = par >> 2, py = (par >> 1) & 1, px = par & 1;
    const int xb = px ? p.IW - 1 : 0, yb = py ? p.IH - 1 : 0, zb = pz ? p.ID - 1 : 0;
    // cell of row rho
    auto cell = [&](int rho, int& iz, int& iy, int& ix, bool& owned, int& bset) {
        const int u = tile * 32 + rho;
        if (type == 0) { iz = u; iy = yb; ix = xb; owned = u < p.ID; }
        else if (type == 1) { iz = zb; iy = u; ix = xb; owned = u < p.IH && u != yb; }
        else { iz = zb; iy = yb; ix = u; owned = u < p.IW && u != xb; }
        iz = min(iz, p.ID - 1); iy = min(iy, p.IH - 1); ix = min(ix, p.IW - 1);
        bset = (ix == xb ? 1 : 0) | (iy == yb ? 2 : 0) | (iz == zb ? 4 : 0);
    };
    int iz, iy, ix, bset; bool owned;
    cell(l31, iz, iy, ix, owned, bset);
    const int C16 = p.Cin >> 4, NH = p.Cout >> 5;
    const size_t plane = (size_t)p.Co_pad, kstride = 4 * plane;
    const bool affine = p.in_scale != nullptr;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    for (int nh = 0; nh < NH; ++nh) {
        f32x16 acc, accl;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accl[r] = 0.f; }
        for (int S = 1; S < 8; ++S) {
            const bool rowon = owned && (bset & S) == S;
            if (__ballot(rowon) == 0ull) continue;                     // wave-uniform
            if (p.ypad && S == 2) continue;                            // {y} alone: left out by the main kernel's epilogue already
            const int e = 8 + (S - 1) * 8 + par;
            const int ntaps = axes_taps(S);
            const half8* wq = p.wc + (size_t)set_tap_offset(e) * C16 * kstride + (size_t)h * plane + nh * 32 + l31;
            // taps in groups of three: the loads of a group are issued together; a corner set has one tap
            for (int c = 0; c < C16; ++c) {
                const int cbase = c * 16 + 8 * h;
                f32x4 sca = {0.f, 0.f, 0.f, 0.f}, sha = sca, scb = sca, shb = sca;
                if (affine) {
                    const float* ps = p.in_scale + (size_t)n * p.Cin + cbase; const float* ph = p.in_shift + (size_t)n * p.Cin + cbase;
                    sca = *reinterpret_cast<const f32x4*>(ps); scb = *reinterpret_cast<const f32x4*>(ps + 4);
                    sha = *reinterpret_cast<const f32x4*>(ph); shb = *reinterpret_cast<const f32x4*>(ph + 4);
                }
                for (int t0 = 0; t0 < ntaps; t0 += 3) {
                    f32x4 va[3], vb[3]; half8 wh[3], wl[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const int t = min(t0 + u, ntaps - 1);
                        int d[3] = {0, 0, 0}, qd = t;                      // x, y, z offsets
#pragma unroll
                        for (int a = 0; a < 3; ++a) if (!((S >> a) & 1)) { d[a] = qd % 3 - 1; qd /= 3; }
                        const int gz = min(max(iz + d[2], 0), p.ID - 1), gy = min(max(iy + d[1], 0), p.IH - 1), gx = min(max(ix + d[0], 0), p.IW - 1);
                        ld8_raw<IH16>(p.in, ((((size_t)n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + cbase, va[u], vb[u]);
                        const half8* wt = wq + ((size_t)c * ntaps + t) * kstride;
                        wh[u] = wt[0]; wl[u] = wt[2 * plane];
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        if (t0 + u < ntaps) {
                            widen8<IH16>(va[u], vb[u]);
                            f32x4 xa = act4(va[u], sca, sha, affine, p.in_slope), xb2 = act4(vb[u], scb, shb, affine, p.in_slope);
                            if (!rowon) { xa = f32x4{0.f, 0.f, 0.f, 0.f}; xb2 = xa; }
                            half8 hi, lo;
                            split8(xa, xb2, hi, lo);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, wh[u], acc, 0, 0, 0);
                            accl = nm_mfma_lo<SINGLE>(hi, wl[u], accl);
                            accl = nm_mfma_lo<SINGLE>(lo, wh[u], accl);
                        }
                    }
                }
            }
        }
        // add to the main kernel's values, partial sums of the final values
        float s = 0.f, ss = 0.f;
        const int co = nh * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rho = (r & 3) + 8 * (r >> 2) + 4 * h;
            int rz, ry, rx, rb; bool ro;
            cell(rho, rz, ry, rx, ro, rb);
            if (ro) {
                const size_t dst = ((((size_t)n * OD + 2 * rz + pz) * OH + 2 * ry + py) * OW + 2 * rx + px) * p.Cout + co;
                const float v = nm_ld1<OH16>(p.out, dst) + (acc[r] + accl[r] * (1.0f / UP2C_SPLIT_SCALE));
                nm_st1<OH16>(p.out, dst, v);
                s += v; ss += v * v;
            }
        }
        if (p.part) {
            s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
            if (h == 0) { float* dst = p.part + (((size_t)n * p.nblk + slot) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
        }
    }
}

// ---- the shell kernels of the split-fp16, fp32-storage instantiation (NM355_UP2C_SHELL, default) ---------------------------------
// conv_up2c_face_kernel re-reads a class's 9 x Cin/16 weight k-steps (2 KB each) from L2 once per line of 32 cells: three MFMAs per
// fetch, and the launch runs at the L2's gather rate instead of the matrix pipe's.  conv_up2c_face_r_kernel gives a workgroup R lines
// of one (type, side, tile along the line) with adjacent across-indices f0 ... f0 + R - 1: the staged tile is R + 2 lines (the halo
// lines are shared), a wave keeps its parity class, its weight stream and the three-deep prefetch, and one bh / bl pair feeds 3 R
// MFMAs into R pairs of accumulators.  Per output cell nothing changes: the same operands in the same order into the same two
// accumulators (c outer, tap inner; hi w_hi -> acc; hi w_lo, lo w_hi -> accl), the same store expression and the same partial slot
// (one per parent line and wave, rows summed r ascending) - the two forms agree bit for bit.  What was per workgroup is per line:
// `off` (the line lies on an edge for this class), the ownership of a row, a group that ends at the last across-index (lines
// f >= AC are skipped, never padded; their MFMAs run on staged clamped lines and are dropped).  Under p.ypad the y faces have no
// groups at all; their (empty) partial slots are zeroed by the workgroups of the frame, 256 floats per workgroup and round.
template <int R> constexpr int face_r_fpv() { return face_fpv(R); }      // slots per plane (odd)

template <int R, int P>
__global__ __launch_bounds__(256, 2) void conv_up2c_face_r_kernel(Up2cParams p, int TY, int TX) {
    static_assert(P == 6 || P == 9, "prefetch depth: the ring index must be static in the unrolled k-loop");
    constexpr int CU = P == 6 ? 2 : 1;                                // chunks per unrolled body (9 CU % P == 0; Cin / 16 is even)
    constexpr int FPVR = face_r_fpv<R>();
    extern __shared__ f32x4 lds_raw[];
    half8* tile = reinterpret_cast<half8*>(lds_raw);               // [chunk*4 + hl*2 + h][FPVR], slot = staged line * FP + along
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const int GD = (p.ID + R - 1) / R, GH = (p.IH + R - 1) / R;       // line groups across z / across y
    const int nX = 2 * p.ID * TY, nY = 2 * p.ID * TX;                // the parent's lines per frame (slot numbering)
    const int gX = 2 * GD * TY, gY = p.ypad ? 0 : 2 * GD * TX, gZ = 2 * GH * TX, per_frame = gX + gY + gZ;
    const int n = (int)blockIdx.x / per_frame; int g = (int)blockIdx.x % per_frame;
    const int bricks = p.nbz * p.nby * p.nbx;
    if (p.ypad && p.part) {
        float* yz = p.part + (((size_t)n * p.nblk + 8 * bricks + 4 * nX) * p.Cout) * 2;
        const int ny = nY * 4 * p.Cout * 2;
        for (int i = g * 256 + tid; i < ny; i += per_frame * 256) yz[i] = 0.f;
    }
    // type 0: x face (line along y at z = f), 1: y face (along x at z = f), 2: z face (along x at y = f)
    int type, side, f0, tl, qbase;
    if (g < gX) { type = 0; tl = g % TY; f0 = (g / TY) % GD * R; side = g / (TY * GD); qbase = 0; }
    else if (g < gX + gY) { g -= gX; type = 1; tl = g % TX; f0 = (g / TX) % GD * R; side = g / (TX * GD); qbase = nX; }
    else { g -= gX + gY; type = 2; tl = g % TX; f0 = (g / TX) % GH * R; side = g / (TX * GH); qbase = nX + nY; }
    const int LA = type == 0 ? p.IH : p.IW;                            // cells along the line's axis
    const int AC = type == 2 ? p.IH : p.ID;                            // extent of the across axis
    const int TL = type == 0 ? TY : TX;                                // tiles along a line
    const int fb = side ? (type == 0 ? p.IW : type == 1 ? p.IH : p.ID) - 1 : 0;      // the face's coarse index on its own axis
    const int C16 = p.Cin >> 4, NH = p.Cout >> 5;
    const bool affine = p.in_scale != nullptr;
    // ---- stage R + 2 lines x 34 voxels x Cin channels: staged line j is across-index clamp(f0 - 1 + j) ----
    const int noct = p.Cin >> 3, nitems = (R + 2) * 34 * noct;       // (noct divides 256 - nm_launch_conv_up2c sees to it: a thread keeps its channel octet)
    f32x4 sca = {0.f, 0.f, 0.f, 0.f}, sha = sca, scb = sca, shb = sca;
    if (affine) {
        const int oct = tid % noct;
        const float* ps = p.in_scale + (size_t)n * p.Cin + oct * 8; const float* ph = p.in_shift + (size_t)n * p.Cin + oct * 8;
        sca = *reinterpret_cast<const f32x4*>(ps); scb = *reinterpret_cast<const f32x4*>(ps + 4);
        sha = *reinterpret_cast<const f32x4*>(ph); shb = *reinterpret_cast<const f32x4*>(ph + 4);
    }
    // eight items per thread and round: the loads of a round are all issued before the first of them is converted
    constexpr int SB = 8;
    for (int i0 = tid; i0 < nitems; i0 += 256 * SB) {
        f32x4 va[SB], vb[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            const int i = i0 + 256 * j;
            if (i < nitems) {
                const int oct = i % noct, v = i / noct, s = v % 34, a = v / 34;
                const int ca = min(max(f0 + a - 1, 0), AC - 1), cl = min(max(tl * 32 - 1 + s, 0), LA - 1);
                const int gz = type == 2 ? fb : ca, gy = type == 0 ? cl : (type == 1 ? fb : ca), gx = type == 0 ? fb : cl;
                ld8_raw<false>(p.in, ((((size_t)n * p.ID + gz) * p.IH + gy) * p.IW + gx) * p.Cin + oct * 8, va[j], vb[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            const int i = i0 + 256 * j;
            if (i < nitems) {
                const int oct = i % noct, v = i / noct, s = v % 34, a = v / 34;
                half8 hi, lo;
                split8(act4(va[j], sca, sha, affine, p.in_slope), act4(vb[j], scb, shb, affine, p.in_slope), hi, lo);
                const int pl = (oct >> 1) * 4 + (oct & 1);
                tile[pl * FPVR + a * FP + s] = hi;
                tile[(pl + 2) * FPVR + a * FP + s] = lo;
            }
        }
    }
    lds_barrier();
    // ---- this wave's parity class, rows, weights ----
    const int pa = wave >> 1, pl_ = wave & 1;                        // parities of the across / along axes
    int pz, py, px;
    if (type == 0) { px = side; pz = pa; py = pl_; } else if (type == 1) { py = side; pz = pa; px = pl_; } else { pz = side; py = pa; px = pl_; }
    const int par = pz * 4 + py * 2 + px;
    const int S = 1 << type;
    const int ab = pa ? AC - 1 : 0, lb = pl_ ? LA - 1 : 0;           // border indices of this class on the two in-face axes
    const int nlines = min(R, AC - f0);                               // lines of this group that exist
    bool any_on = false;                                              // (wave-uniform) a line that is not on an edge for this class
#pragma unroll
    for (int i = 0; i < R; ++i) any_on = any_on || (i < nlines && f0 + i != ab);
    const size_t plane = (size_t)p.Co_pad, kstride = 4 * plane;
    const int nk = 9 * C16;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    const int arow = h * FPVR + l31;
    for (int nh = 0; nh < NH; ++nh) {
        f32x16 acc[R], accl[R];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; accl[i][r] = 0.f; }
        if (any_on) {
            const half8* wq = p.wc + (size_t)set_tap_offset(8 + (S - 1) * 8 + par) * C16 * kstride + (size_t)h * plane + nh * 32 + l31;
            // the weights of a k-step are requested P k-steps ahead: a wave's own stream is its only traffic in this loop, and at the
            // L2's loaded latency (about 2 us) three k-steps of 12 MFMAs do not cover it
            half8 bh[P], bl[P];
#pragma unroll
            for (int u = 0; u < P; ++u) { bh[u] = wq[(size_t)min(u, nk - 1) * kstride]; bl[u] = wq[(size_t)min(u, nk - 1) * kstride + 2 * plane]; }
            for (int c0 = 0; c0 < C16; c0 += CU) {
#pragma unroll
                for (int tt = 0; tt < 9 * CU; ++tt) {
                    const int c = c0 + tt / 9, t = tt % 9;
                    const int k = c * 9 + t, s = tt % P;
                    // (the row base is opaque per k-step: lines i and i + 1 read the same staged line at taps three apart, and merged
                    //  reads held across k-steps cost more registers than the kernel has)
                    int ar = arow + c * 4 * FPVR;
                    asm volatile("" : "+v"(ar));
                    half8 ah[R], al[R];
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        ah[i] = tile[ar + (i + t / 3) * FP + (t % 3)];
                        al[i] = tile[ar + 2 * FPVR + (i + t / 3) * FP + (t % 3)];
                    }
                    const half8 wh = bh[s], wl = bl[s];
                    const int kn = min(k + P, nk - 1);
                    bh[s] = wq[(size_t)kn * kstride]; bl[s] = wq[(size_t)kn * kstride + 2 * plane];
#pragma unroll
                    for (int i = 0; i < R; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], wh, acc[i], 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < R; ++i) accl[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], wl, accl[i], 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < R; ++i) accl[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], wh, accl[i], 0, 0, 0);
                }
            }
        }
        const int co = nh * 32 + l31;
        // element index of row rho of line f: base + f * across + (tl * 32 + rho) * along (the parent's index, term by term)
        const size_t sX = (size_t)p.Cout, sY = (size_t)OW * sX, sZ = (size_t)OH * sY;
        const size_t along = 2 * (type == 0 ? sY : sX), across = 2 * (type == 2 ? sY : sZ);
        const size_t lane_base = (size_t)n * OD * sZ + pz * sZ + py * sY + px * sX + 2 * fb * (type == 0 ? sX : type == 1 ? sY : sZ) + co +
                                 (size_t)(tl * 32 + 4 * h) * along;
        // the old values of all lines in one batch of loads (one load-add-store round trip per output half, not one per row)
        float old[R][16];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool on = i < nlines && f0 + i != ab;               // (off: the whole line lies on an edge for this class)
            const size_t line_base = lane_base + (size_t)(f0 + i) * across;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = tl * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                old[i][r] = 0.f;
                if (on && u < LA && u != lb) old[i][r] = nm_ld1<false>(p.out, line_base + (size_t)((r & 3) + 8 * (r >> 2)) * along);
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (i >= nlines) break;
            const int f = f0 + i;
            const bool off = f == ab;
            const size_t line_base = lane_base + (size_t)f * across;
            float s = 0.f, ss = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int u = tl * 32 + rho;
                if (!off && u < LA && u != lb) {
                    const size_t dst = line_base + (size_t)((r & 3) + 8 * (r >> 2)) * along;
                    const float v = old[i][r] + (acc[i][r] + accl[i][r] * (1.0f / UP2C_SPLIT_SCALE));
                    nm_st1<false>(p.out, dst, v);
                    s += v; ss += v * v;
                }
            }
            if (p.part) {
                s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
                const int slot_part = 8 * bricks + (qbase + (side * AC + f) * TL + tl) * 4 + wave;
                if (h == 0) { float* dst = p.part + (((size_t)n * p.nblk + slot_part) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
            }
        }
    }
}

// conv_up2c_edge_p_kernel: conv_up2c_edge_kernel's items and arithmetic with the loads kept in flight.  An item's work is a sequence
// of tap groups (subset S ascending, 16-channel chunk ascending, taps in threes ascending); the loads of the groups g + 1 ... g + 3 -
// three A octet pairs and the weights of BOTH 32-channel output halves each - are in flight in a ring of four register sets during
// the MFMAs of group g (one wave per SIMD: the registers are there, the parallelism is not).  For the layers with two output halves
// (Cout = 64); NM355_UP2C_SHELL=2 / 3 only, not the default (it does not clear the bar on the step).  The A operands are
// activated and split once and feed both halves' accumulators.  The pending GroupNorm scale / shift of the frame are copied to LDS
// once per wave (wave-private rows: no workgroup barrier) and read from there with each group's loads.  Per accumulator the MFMA
// sequence is conv_up2c_edge_kernel's.
__global__ __launch_bounds__(256, 1) void conv_up2c_edge_p_kernel(Up2cParams p, int TZ, int TY, int TX, int slot0) {
    constexpr int NHT = 2;                                             // output halves
    __shared__ __attribute__((aligned(16))) float aff[4][2][128];                                  // [wave][scale | shift][channel] (Cin <= 128: nm_conv_plan::up2c_eligible)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const int nXY = 8 * TZ, nXZ = 8 * TY, nYZ = 8 * TX, per_frame = nXY + nXZ + nYZ;
    const long long gitem = (long long)blockIdx.x * 4 + wave;
    if (gitem >= (long long)p.N * per_frame) return;
    const int n = (int)(gitem / per_frame); int q = (int)(gitem % per_frame);
    const int slot = slot0 + q;
    // type 0: x-y edge (line along z), 1: x-z edge (along y), 2: y-z edge (along x); q -> (tile, parity class)
    int type, tile, par;
    if (q < nXY) { type = 0; tile = q / 8; par = q % 8; }
    else if (q < nXY + nXZ) { q -= nXY; type = 1; tile = q / 8; par = q % 8; }
    else { q -= nXY + nXZ; type = 2; tile = q / 8; par = q % 8; }
    const int pz = par >> 2, py = (par >> 1) & 1, px = par & 1;
    const int xb = px ? p.IW - 1 : 0, yb = py ? p.IH - 1 : 0, zb = pz ? p.ID - 1 : 0;
    auto cell = [&](int rho, int& iz, int& iy, int& ix, bool& owned, int& bset) {
        const int u = tile * 32 + rho;
        if (type == 0) { iz = u; iy = yb; ix = xb; owned = u < p.ID; }
        else if (type == 1) { iz = zb; iy = u; ix = xb; owned = u < p.IH && u != yb; }
        else { iz = zb; iy = yb; ix = u; owned = u < p.IW && u != xb; }
        iz = min(iz, p.ID - 1); iy = min(iy, p.IH - 1); ix = min(ix, p.IW - 1);
        bset = (ix == xb ? 1 : 0) | (iy == yb ? 2 : 0) | (iz == zb ? 4 : 0);
    };
    int iz, iy, ix, bset; bool owned;
    cell(l31, iz, iy, ix, owned, bset);
    const int C16 = p.Cin >> 4;
    const size_t plane = (size_t)p.Co_pad, kstride = 4 * plane;
    const bool affine = p.in_scale != nullptr;
    const int OD = 2 * p.ID, OH = 2 * p.IH, OW = 2 * p.IW;
    if (affine) {
        for (int i = lane; i < p.Cin; i += 64) {
            aff[wave][0][i] = p.in_scale[(size_t)n * p.Cin + i];
            aff[wave][1][i] = p.in_shift[(size_t)n * p.Cin + i];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the wave's own rows: written before any lane of it reads them
    }
    // the subsets with a row to correct (wave-uniform), ascending
    unsigned smask = 0;
#pragma unroll
    for (int S = 1; S < 8; ++S) {
        const bool rowon = owned && (bset & S) == S;
        if (__ballot(rowon) != 0ull && !(p.ypad && S == 2)) smask |= 1u << S;      // ({y} alone: left out by the main kernel's epilogue already)
    }
    smask = __builtin_amdgcn_readfirstlane(smask);
    f32x16 acc[NHT], accl[NHT];
#pragma unroll
    for (int nh = 0; nh < NHT; ++nh)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[nh][r] = 0.f; accl[nh][r] = 0.f; }

    struct It { int S, c, t0, ntaps; size_t wbase; };                  // a tap group; wbase: the set's offset in half8 units
    struct Regs { f32x4 va[3], vb[3], sca, scb, sha, shb; half8 wh[3][NHT], wl[3][NHT]; int S, t0, ntaps; };
    auto enter = [&](It& it, int S) {
        // set_tap_offset(8 + (S - 1) * 8 + par) = 216 + 8 * (taps of the subsets below S) + par * taps(S), from two packed tables
        // (taps 9 9 3 9 3 3 1 for S = 1 ... 7; their running sums 0 9 18 21 30 33 36)
        const int nt = (int)((0x1339399ull >> (4 * (S - 1))) & 15), below = (int)((0x2485e552240ull >> (6 * (S - 1))) & 63);
        it.S = S; it.c = 0; it.t0 = 0; it.ntaps = nt;
        it.wbase = (size_t)(216 + 8 * below + par * nt) * C16 * kstride;
    };
    auto advance = [&](It& it) {                                       // false (and `it` unchanged) behind the last group
        if (it.t0 + 3 < it.ntaps) { it.t0 += 3; return true; }
        if (it.c + 1 < C16) { ++it.c; it.t0 = 0; return true; }
        const unsigned rest = smask >> (it.S + 1);
        if (rest == 0) return false;
        enter(it, it.S + 1 + __builtin_ctz(rest));
        return true;
    };
    // element offsets of the lane's three clamped neighbours per axis, once: a tap's address is three selects and three adds
    auto eoff = [&](int i, int k, int ext, size_t stride) { return (size_t)min(max(i + k, 0), ext - 1) * stride; };
    const size_t sx = (size_t)p.Cin, sy = (size_t)p.IW * sx, sz = (size_t)p.IH * sy;
    const size_t z0 = eoff(iz, -1, p.ID, sz), z1 = eoff(iz, 0, p.ID, sz), z2 = eoff(iz, 1, p.ID, sz);
    const size_t y0 = eoff(iy, -1, p.IH, sy), y1 = eoff(iy, 0, p.IH, sy), y2 = eoff(iy, 1, p.IH, sy);
    const size_t x0 = eoff(ix, -1, p.IW, sx), x1 = eoff(ix, 0, p.IW, sx), x2 = eoff(ix, 1, p.IW, sx);
    const size_t in_base = (size_t)n * p.ID * sz;
    auto pick = [](size_t a, size_t b, size_t c, int d) { return d < 0 ? a : d == 0 ? b : c; };
    auto load = [&](Regs& g, const It& it) __attribute__((always_inline)) {
        g.S = it.S; g.t0 = it.t0; g.ntaps = it.ntaps;
        const int cbase = it.c * 16 + 8 * h;
        const half8* wq = p.wc + it.wbase + (size_t)h * plane + l31;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int t = min(it.t0 + u, it.ntaps - 1);
            int d[3] = {0, 0, 0}, qd = t;                              // x, y, z offsets
#pragma unroll
            for (int a = 0; a < 3; ++a) if (!((it.S >> a) & 1)) { d[a] = qd % 3 - 1; qd /= 3; }
            ld8_raw<false>(p.in, in_base + pick(z0, z1, z2, d[2]) + pick(y0, y1, y2, d[1]) + pick(x0, x1, x2, d[0]) + cbase, g.va[u], g.vb[u]);
            const half8* wt = wq + ((size_t)it.c * it.ntaps + t) * kstride;
#pragma unroll
            for (int nh = 0; nh < NHT; ++nh) { g.wh[u][nh] = wt[nh * 32]; g.wl[u][nh] = wt[2 * plane + nh * 32]; }
        }
        if (affine) {
            g.sca = *reinterpret_cast<const f32x4*>(&aff[wave][0][cbase]); g.scb = *reinterpret_cast<const f32x4*>(&aff[wave][0][cbase + 4]);
            g.sha = *reinterpret_cast<const f32x4*>(&aff[wave][1][cbase]); g.shb = *reinterpret_cast<const f32x4*>(&aff[wave][1][cbase + 4]);
        } else {
            g.sca = g.scb = g.sha = g.shb = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto consume = [&](const Regs& g) __attribute__((always_inline)) {
        const bool rowon = owned && (bset & g.S) == g.S;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            if (g.t0 + u < g.ntaps) {
                f32x4 xa = act4(g.va[u], g.sca, g.sha, affine, p.in_slope), xb2 = act4(g.vb[u], g.scb, g.shb, affine, p.in_slope);
                if (!rowon) { xa = f32x4{0.f, 0.f, 0.f, 0.f}; xb2 = xa; }
                half8 hi, lo;
                split8(xa, xb2, hi, lo);
#pragma unroll
                for (int nh = 0; nh < NHT; ++nh) acc[nh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, g.wh[u][nh], acc[nh], 0, 0, 0);
#pragma unroll
                for (int nh = 0; nh < NHT; ++nh) accl[nh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, g.wl[u][nh], accl[nh], 0, 0, 0);
#pragma unroll
                for (int nh = 0; nh < NHT; ++nh) accl[nh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(lo, g.wh[u][nh], accl[nh], 0, 0, 0);
            }
        }
    };
    if (smask) {
        // NSET register sets in a ring: group g is consumed with the loads of g + 1 ... g + NSET - 1 in flight.  The loads are
        // unconditional (behind the last group its own are issued again and dropped), so that the wait in front of a group's
        // MFMAs counts exactly the loads of the groups after it.
        constexpr int NSET = 4;
        int ngroups = 0;
#pragma unroll
        for (int S = 1; S < 8; ++S) if ((smask >> S) & 1) ngroups += C16 * ((axes_taps(S) + 2) / 3);
        It it; enter(it, __builtin_ctz(smask));
        Regs g[NSET];
        load(g[0], it);
#pragma unroll
        for (int j = 1; j < NSET - 1; ++j) { advance(it); load(g[j], it); }
        for (int base = 0; base < ngroups; base += NSET) {
#pragma unroll
            for (int j = 0; j < NSET; ++j) {
                advance(it);
                load(g[(j + NSET - 1) % NSET], it);
                if (base + j < ngroups) consume(g[j]);
            }
        }
    }
    // add to the main kernel's values, partial sums of the final values; the old values of both halves in one batch of loads
    float old[NHT][16];
#pragma unroll
    for (int nh = 0; nh < NHT; ++nh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int rz, ry, rx, rb; bool ro;
            cell((r & 3) + 8 * (r >> 2) + 4 * h, rz, ry, rx, ro, rb);
            old[nh][r] = 0.f;
            if (ro) old[nh][r] = nm_ld1<false>(p.out, ((((size_t)n * OD + 2 * rz + pz) * OH + 2 * ry + py) * OW + 2 * rx + px) * p.Cout + nh * 32 + l31);
        }
#pragma unroll
    for (int nh = 0; nh < NHT; ++nh) {
        float s = 0.f, ss = 0.f;
        const int co = nh * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rho = (r & 3) + 8 * (r >> 2) + 4 * h;
            int rz, ry, rx, rb; bool ro;
            cell(rho, rz, ry, rx, ro, rb);
            if (ro) {
                const size_t dst = ((((size_t)n * OD + 2 * rz + pz) * OH + 2 * ry + py) * OW + 2 * rx + px) * p.Cout + co;
                const float v = old[nh][r] + (acc[nh][r] + accl[nh][r] * (1.0f / UP2C_SPLIT_SCALE));
                nm_st1<false>(p.out, dst, v);
                s += v; ss += v * v;
            }
        }
        if (p.part) {
            s += __shfl_xor(s, 32); ss += __shfl_xor(ss, 32);
            if (h == 0) { float* dst = p.part + (((size_t)n * p.nblk + slot) * p.Cout + co) * 2; dst[0] = s; dst[1] = ss; }
        }
    }
}

}  // namespace

size_t nm_up2c_weight_floats(int Cin, int Co_pad) {
    return (size_t)(TOTAL_TAPS + YSETS * 27) * (Cin >> 4) * 4 * Co_pad * 8 / 2;       // halves -> 4-byte units
}

int nm_launch_up2c_compose(const float* w, int Cout, int Cin, int Co_pad, void* packed, hipStream_t s) {
    if (Cin % 16 || Co_pad % 32 || Cout > Co_pad) { nm_set_error("up2c_compose: bad channels Cin=%d Cout=%d/%d", Cin, Cout, Co_pad); return NM_ERR_ARG; }
    hipLaunchKernelGGL(up2c_compose_kernel, dim3(2048), dim3(256), 0, s, w, Cout, Cin, Co_pad, reinterpret_cast<_Float16*>(packed));
    hipLaunchKernelGGL(up2y_compose_kernel, dim3(512), dim3(256), 0, s, w, Cout, Cin, Co_pad, reinterpret_cast<_Float16*>(packed));
    return nm_check_hip(hipGetLastError(), "up2c_compose launch");
}

// The one-product instantiations of the main / face / edge kernels by storage combination io (bit 0 bfloat16 input, bit 1 bfloat16
// output); launch_io runs `split` in the split-fp16 mode (fp32 storage only) and one[io] in the one-product modes.
static void (*const MAIN_ONE[4])(Up2cParams) = {conv_up2c_kernel<0>, conv_up2c_kernel<1>, conv_up2c_kernel<2>, conv_up2c_kernel<3>};
static void (*const FACE_ONE[4])(Up2cParams, int, int) = {conv_up2c_face_kernel<true, 0>, conv_up2c_face_kernel<true, 1>, conv_up2c_face_kernel<true, 2>, conv_up2c_face_kernel<true, 3>};
static void (*const EDGE_ONE[4])(Up2cParams, int, int, int, int) = {conv_up2c_edge_kernel<true, 0>, conv_up2c_edge_kernel<true, 1>, conv_up2c_edge_kernel<true, 2>, conv_up2c_edge_kernel<true, 3>};
template <typename... P, typename... A>
static void launch_io(void (*split)(P...), void (*const (&one)[4])(P...), bool single, int io, dim3 grid, int threads, size_t lds, hipStream_t s, A... args) {
    hipLaunchKernelGGL(single ? one[io] : split, grid, dim3(threads), lds, s, args...);
}

int nm_launch_conv_up2c(const TensorRef& in, const void* packed, const float* bias, float* out, int Cout, int Co_pad, float* part,
                        hipStream_t s, const nm_conv_plan::Up2cPlan& u) {
    using namespace nm_conv_plan;
    if (!packed) { nm_set_error("conv_up2c: no composite weight sets"); return NM_ERR_ARG; }
    static NmDeviceOnce attr_set;
    if (int rc = nm_raise_lds_limit(attr_set, 160 * 1024, "hipFuncSetAttribute(conv_up2c)", MAIN_ONE[0], MAIN_ONE[1], MAIN_ONE[2], MAIN_ONE[3],
                                    &conv_up2c_x16_kernel, &conv_up2y_kernel<false>, &conv_up2y_kernel<true>,
                                    &conv_up2c_face_r_kernel<2, 9>, &conv_up2c_face_r_kernel<4, 6>)) return rc;
    const bool single = u.main == UP2C_ONE;
    const int io = u.io;
    Up2cParams p;
    p.in = in.p; p.in_scale = in.scale; p.in_shift = in.shift; p.in_slope = in.slope;
    p.N = in.N; p.ID = in.D; p.IH = in.H; p.IW = in.W; p.Cin = in.C;
    p.wc = static_cast<const half8*>(packed); p.wy = p.wc + (size_t)TOTAL_TAPS * (in.C >> 4) * 4 * Co_pad; p.bias = bias; p.out = out; p.part = part;
    p.Cout = Cout; p.Co_pad = Co_pad;
    p.nbz = u.nbz; p.nby = u.nby; p.nbx = u.nbx;
    p.nblk = up2c::part_rows(in.D, in.H, in.W);
    p.march = u.march; p.ypad = u.ypad;
    void (*const main_split)(Up2cParams) = u.main == UP2C_X16 ? conv_up2c_x16_kernel : u.main == UP2Y_MARCH ? conv_up2y_kernel<true> : conv_up2y_kernel<false>;
    launch_io(main_split, MAIN_ONE, single, io, dim3((unsigned)u.main_grid), 512, LDS_BYTES, s, p);
    int rc = nm_check_hip(hipGetLastError(), "conv_up2c launch");
    if (rc) return rc;
    // NM355_ENC_SCHED bit 2 (the lane is set by decode_frames only, nm_net.hip): the edge launch goes to the lane, behind the main
    // launch and BESIDE the face launch, and is joined before this function returns - the caller's profiler bracket and the
    // gn_finalize that follows see the whole layer.  The two launches are independent in every instantiation ("shell kernels" above:
    // each reads the main kernel's output at the cells it owns and nowhere else, stores one float per lane and owned row, and the
    // partial slots are disjoint - face items and the zeroed y-face slots below 8 bricks + 4 fg, edge items from there).
    NmLaunchState& ls = nm_ls();
    const hipStream_t se = (ls.shell_lane && ls.shell_lane != s && ls.shell_fork && ls.shell_join) ? ls.shell_lane : s;
    if (se != s) {
        if ((rc = nm_check_hip(hipEventRecord(ls.shell_fork, s), "conv_up2c: shell fork event"))) return rc;
        if ((rc = nm_check_hip(hipStreamWaitEvent(se, ls.shell_fork, 0), "conv_up2c: shell lane wait"))) return rc;
    }
    const int TZ = u.sh.TZ, TY = u.sh.TY, TX = u.sh.TX;
    if (u.face == FACE_R) {
        if (u.R == 2) hipLaunchKernelGGL((conv_up2c_face_r_kernel<2, 9>), dim3((unsigned)u.face_grid), dim3(256), u.face_lds, s, p, TY, TX);
        else hipLaunchKernelGGL((conv_up2c_face_r_kernel<4, 6>), dim3((unsigned)u.face_grid), dim3(256), u.face_lds, s, p, TY, TX);
    }
    else launch_io(conv_up2c_face_kernel<false>, FACE_ONE, single, io, dim3((unsigned)u.face_grid), 256, u.face_lds, s, p, TY, TX);
    rc = nm_check_hip(hipGetLastError(), "conv_up2c_face launch");
    if (!rc) {
        if (u.edge == EDGE_P) hipLaunchKernelGGL(conv_up2c_edge_p_kernel, dim3((unsigned)u.edge_grid), dim3(256), 0, se, p, TZ, TY, TX, u.slot0);
        else launch_io(conv_up2c_edge_kernel<false>, EDGE_ONE, single, io, dim3((unsigned)u.edge_grid), 256, 0, se, p, TZ, TY, TX, u.slot0);
        rc = nm_check_hip(hipGetLastError(), "conv_up2c_edge launch");
        if (!rc && se != s && ls.prof_on) ++ls.side_launches;
    }
    if (se != s) {      // (joined behind a failed face or edge launch too: once forked, the lane never stays ahead of s)
        int rj = nm_check_hip(hipEventRecord(ls.shell_join, se), "conv_up2c: shell join event");
        if (!rj) rj = nm_check_hip(hipStreamWaitEvent(s, ls.shell_join, 0), "conv_up2c: join the shell lane");
        if (!rc) rc = rj;
    }
    return rc;
}
