// How the producer waves of the persistent conv kernels (conv_f16p, _f16p2, _f16p8, _f16q2, _f16r) stage a brick's halo tile: which
// pieces of the tile a producer thread owns, where a piece comes from and where it goes, and the conversion on the way (pending
// GroupNorm affine + LeakyReLU, zero padding, fp16).  Device code.  What is NOT here is the schedule: the order of loads, converts,
// counted waits and barriers in a step stays in each kernel, and so do the load destination registers (raw / sc / sh), which the
// kernels' counted waits must name; the helpers receive them by reference.
#pragma once

#include "nm_common.h"
#include <type_traits>

#define NM_SPLIT_SCALE 2048.0f   // lo parts of the split-fp16 operands are stored times 2^11

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16-byte global load the compiler's wait-count tracking does not see.  hipcc waits vmcnt(0) at the first use of an
// ordinary load result whenever an LDS-DMA is in flight, which would drain the weight pipeline of conv_f16p at the first
// staging piece; the kernel instead waits explicitly (its group-end vmcnt(0)) before the results are used.
__device__ __forceinline__ f32x4 load16_untracked(const float* q) {
    f32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(q) : "memory");
    return r;
}

// 8-byte form (four bfloat16 channels of a 16-bit-storage tensor), same tracking rules
__device__ __forceinline__ nm_u32x2 load8_untracked(const float* base, unsigned byte_off) {
    nm_u32x2 r;
    const char* q = reinterpret_cast<const char*>(base) + byte_off;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r) : "v"(q) : "memory");
    return r;
}

// the same from a wave-uniform base and a 32-bit per-lane byte offset (one 64-bit VALU add; the scalar-base addressing form
// needs the base in SGPRs, which the compiler does not guarantee for an inline-asm operand computed through VALU divisions)
__device__ __forceinline__ f32x4 load16_untracked(const float* base, unsigned byte_off) {
    return load16_untracked(reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off));
}

// The pieces of producer thread pt (0 ... 255) in a halo tile of HV = (HV / 100) x 10 x 10 voxels x 16 channels: piece k = NCH
// channels (the chunk's channels NCH * sub ... of 16) of halo voxel pt / (16 / NCH) + 256 / (16 / NCH) * k, so neighbouring lanes
// fetch one voxel's contiguous channels.  NP pieces per thread cover the tile (tail masked); EB = bytes per input element (2: the
// tensor is bfloat16).  A halo buffer is planes of HV 16-byte slots, a slot = 8 halves of one voxel: channels 0-7, then 8-15.
template <int NP, int HV, int NCH, unsigned EB, class Params>
struct HaloPieces {
    static_assert((HV == 600 || HV == 1000) && (NCH == 4 || NCH == 8) && (EB == 2u || EB == 4u), "6 | 10 planes of 10 x 10 voxels; quads or octets of fp32 | bfloat16");
    static constexpr int ZP = 100, HX = 10, TPV = 16 / NCH, NQ = NCH / 4;      // (NQ: 16-byte affine loads per table)
    static_assert(NP * 256 >= TPV * HV && (NP - 1) * 256 < TPV * HV, "pieces cover the tile");
    const Params& p;                                                // the launch's: in, in_scale, in_shift, in_slope, ID, IH, IW, Cin (read where they are used)
    int sub;
    int slot[NP], rel[NP], pos[NP];
    unsigned rel111;                                                // halo voxel (1,1,1): always inside (byte offset)
    bool has_affine;

    __device__ __forceinline__ HaloPieces(int pt, const Params& p_)
        : p(p_), sub(pt & (TPV - 1)), rel111((unsigned)(((p_.IH + 1) * p_.IW + 1) * p_.Cin) * EB), has_affine(p_.in_scale != nullptr) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int v = (pt >> (TPV == 4 ? 2 : 1)) + (256 / TPV) * k, vc = min(v, HV - 1);
            const int hz = vc / 100, r = vc % 100, hy = r / 10, hx = r % 10;
            slot[k] = ((sub * NCH) >> 3) * HV + hz * ZP + hy * HX + hx;    // 16-byte slot in a halo buffer (split form: of the hi part; lo: + 2 HV)
            rel[k] = ((hz * p.IH + hy) * p.IW + hx) * p.Cin + NCH * sub;
            pos[k] = (v < HV) ? (hz | (hy << 8) | (hx << 16)) : -1;
        }
    }
    // bit k: piece k of the halo tile of brick w lies inside the volume
    template <class Work>
    __device__ __forceinline__ unsigned inside_mask(const Work& w) const {
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int hz = pos[k] & 0xff, hy = (pos[k] >> 8) & 0xff, hx = pos[k] >> 16;
            const bool in_ = pos[k] >= 0 && (unsigned)(w.oz0 - 1 + hz) < (unsigned)p.ID && (unsigned)(w.oy0 - 1 + hy) < (unsigned)p.IH &&
                             (unsigned)(w.ox0 - 1 + hx) < (unsigned)p.IW;
            m |= (in_ ? 1u : 0u) << k;
        }
        return m;
    }
    // wave-uniform: halo voxel (0,0,0) of brick w, channel 16 cb (may lie outside the tensor)
    template <class Work>
    __device__ __forceinline__ const float* tile_base(const Work& w, int cb) const {
        return nm_eptr(p.in, (size_t)(((((long long)w.n * p.ID + (w.oz0 - 1)) * p.IH + (w.oy0 - 1)) * p.IW + (w.ox0 - 1)) * (long long)p.Cin + cb * 16), EB == 2u);
    }
    // piece k of the tile at `base` into dst (8 bytes where dst has 8): outside pieces fetch an inside voxel (zeroed by convert)
    template <class RawT, int k>
    __device__ __forceinline__ void load_piece(RawT& dst, const float* base, unsigned mask, std::integral_constant<int, k>) const {
        const unsigned off = ((mask >> k) & 1) ? (unsigned)rel[k] * EB : rel111;
        if constexpr (std::is_same_v<RawT, nm_u32x2>) dst = load8_untracked(base, off); else dst = load16_untracked(base, off);
    }
    // the pending affine of this thread's channels of (frame n, chunk cb): always 2 NQ loads - the kernels' waits count instructions
    __device__ __forceinline__ void load_affine(f32x4* sc, f32x4* sh, int n, int cb) const {
        const float* ps = has_affine ? p.in_scale + (size_t)n * p.Cin + cb * 16 : p.in;
        const float* ph = has_affine ? p.in_shift + (size_t)n * p.Cin + cb * 16 : p.in;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            sc[q] = load16_untracked(ps, 4u * (unsigned)(NCH * sub + 4 * q));
            sh[q] = load16_untracked(ph, 4u * (unsigned)(NCH * sub + 4 * q));
        }
    }
    // Split form (conv_f16p, _f16p2, _f16p8): activate, split to hi / lo fp16, write piece k into the halo buffer at `tile`
    // ([hi h0 | hi h1 | lo h0 | lo h1][HV]).  SINGLE (conv modes 3 / 4) has no use for the lo halves.
    template <bool SINGLE, class RawT, int k>
    __device__ __forceinline__ void convert_split(half8* tile, const RawT& raw, const f32x4& sc, const f32x4& sh, unsigned mask, std::integral_constant<int, k>) const {
        static_assert(NCH == 4, "a quad of channels per piece");
        half4v hi4, lo4;
        const float keep = ((mask >> k) & 1) ? 1.f : 0.f;           // padding is zero AFTER the activation
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
            float v0, v1;
            if constexpr (std::is_same_v<RawT, nm_u32x2>) { const unsigned u = raw[e >> 1]; v0 = nm_bf_lo(u); v1 = nm_bf_hi(u); }
            else { v0 = raw[e]; v1 = raw[e + 1]; }
            if (has_affine) { v0 = __builtin_fmaf(v0, sc[e], sh[e]); v1 = __builtin_fmaf(v1, sc[e + 1], sh[e + 1]); }
            // LeakyReLU (slope in (0, 1]) and the padding mask in two instructions per value: max(v, slope v) * keep
            v0 = fmaxf(v0 * keep, (v0 * keep) * p.in_slope); v1 = fmaxf(v1 * keep, (v1 * keep) * p.in_slope);
            half2v hv = __builtin_convertvector(f32x2{v0, v1}, half2v);
            asm volatile("" : "+v"(hv));
            const float t0 = v0 * NM_SPLIT_SCALE, t1 = v1 * NM_SPLIT_SCALE;
            hi4[e] = hv[0]; hi4[e + 1] = hv[1];
            if constexpr (!SINGLE) {
                lo4[e] = (_Float16)__builtin_fmaf((float)hv[0], -NM_SPLIT_SCALE, t0);
                lo4[e + 1] = (_Float16)__builtin_fmaf((float)hv[1], -NM_SPLIT_SCALE, t1);
            }
        }
        if (pos[k] >= 0) {
            half4v* dst = reinterpret_cast<half4v*>(tile + slot[k]) + (sub & 1);
            dst[0] = hi4;
            if constexpr (!SINGLE) dst[4 * HV] = lo4;               // + 2 HV half8 slots
        }
    }
    // One-product form (conv_f16q2, _f16r).  A tensor without a pending affine gets the identity, once per step (behind the wait
    // that covers load_affine's loads): the conversion below is then branch- and select-free (x * 1 + 0 is x)
    __device__ __forceinline__ void fix_affine(f32x4 (&sc)[NQ], f32x4 (&sh)[NQ]) const {
        if (!has_affine) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) { sc[q] = f32x4{1.f, 1.f, 1.f, 1.f}; sh[q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
    }
    // activate, round to fp16, write piece k into the halo buffer at `tile` ([h0 | h1][HV])
    template <int k>
    __device__ __forceinline__ void convert_packed(half8* tile, const f32x4& raw, const f32x4 (&sc)[NQ], const f32x4 (&sh)[NQ], unsigned mask, std::integral_constant<int, k>) const {
        const bool keep = ((mask >> k) & 1) != 0;                   // padding is zero AFTER the activation: selected on the packed halves
        unsigned pk[NCH / 2];
#pragma unroll
        for (int e = 0; e < NCH; e += 2) {
            float v0, v1;
            // (by value: bit_cast of a vector element through a reference reads element 0)
            if constexpr (EB == 2u) { const float rf = raw[e >> 1]; const unsigned u = nm_fbits(rf); v0 = nm_bf_lo(u); v1 = nm_bf_hi(u); }
            else { v0 = raw[e]; v1 = raw[e + 1]; }
            // the pair's affine and slope product as PACKED fp32 instructions (v_pk_fma_f32 / v_pk_mul_f32: two elements per issue
            // slot - the producers are bound by vector issue); the same fma / mul / max per element
            f32x2 vv = f32x2{v0, v1};
            const f32x4 sq = sc[e >> 2], hq = sh[e >> 2];
            const f32x2 s2 = (e & 2) ? f32x2{sq[2], sq[3]} : f32x2{sq[0], sq[1]}, h2 = (e & 2) ? f32x2{hq[2], hq[3]} : f32x2{hq[0], hq[1]};
            vv = __builtin_elementwise_fma(vv, s2, h2);
            const f32x2 vs = vv * f32x2{p.in_slope, p.in_slope};
            vv = f32x2{fmaxf(vv[0], vs[0]), fmaxf(vv[1], vs[1])};
            half2v hv = __builtin_convertvector(vv, half2v);
            asm volatile("" : "+v"(hv));
            pk[e >> 1] = keep ? __builtin_bit_cast(unsigned, hv) : 0u;
        }
        if (pos[k] >= 0) {
            if constexpr (NCH == 8) {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                *reinterpret_cast<u32x4*>(tile + slot[k]) = u32x4{pk[0], pk[1], pk[2], pk[3]};
            } else {
                reinterpret_cast<nm_u32x2*>(tile + slot[k])[sub & 1] = nm_u32x2{pk[0], pk[1]};
            }
        }
    }
};
