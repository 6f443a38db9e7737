// Mesh surface sampling (nm_sample.hip): constants shared by the kernels and their entry point, and the counter-based generator of the
// uniforms - host and device, so the known answers of include/nm355.h can be checked without a launch.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NM_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define NM_SAMPLE_HD inline
#endif

constexpr int NM_SAMPLE_BLOCK = 256;                                 // threads per workgroup (four wavefronts)
constexpr int NM_SAMPLE_MAX_FACES = 1 << 21;                         // 2^21 faces x weights below 2^32: a frame's total stays below 2^53
constexpr int NM_SAMPLE_SEG = 64;                                    // entries of Cum per entry of the coarse table
// The scan.  A thread takes NM_SAMPLE_SCAN_ITEMS consecutive weights, a workgroup NM_SAMPLE_SCAN_STEP per step with a running carry.
// One workgroup scans a whole frame of up to NM_SAMPLE_SCAN_ONE faces (16 steps); longer frames are cut into chunks of
// NM_SAMPLE_SCAN_CHUNK faces: chunk sums, their scan, then the same scan kernel per chunk with the chunk's offset as its carry.
constexpr int NM_SAMPLE_SCAN_ITEMS = 4;
constexpr int NM_SAMPLE_SCAN_STEP = NM_SAMPLE_BLOCK * NM_SAMPLE_SCAN_ITEMS;
constexpr int NM_SAMPLE_SCAN_ONE = 16384;
constexpr int NM_SAMPLE_SCAN_CHUNK = 4096;
static_assert(NM_SAMPLE_SCAN_CHUNK % NM_SAMPLE_SCAN_STEP == 0 && NM_SAMPLE_SCAN_STEP % NM_SAMPLE_SEG == 0, "chunks are whole steps, steps whole segments");
static_assert(NM_SAMPLE_MAX_FACES / NM_SAMPLE_SCAN_CHUNK <= 2 * NM_SAMPLE_BLOCK, "a frame's chunk sums: two per thread of one workgroup");
// The draw.  A workgroup draws up to NM_SAMPLE_DRAW_PER_BLOCK samples of one frame and first copies the frame's coarse table into LDS
// if it has at most NM_SAMPLE_LDS_COARSE entries (16 KiB: the eight workgroups that fill a CU's 32 wavefront slots hold 128 KiB of its
// 160 KiB) - frames of up to 131072 faces.  Past that the coarse table is searched in global memory like the segment.
constexpr int NM_SAMPLE_DRAW_ITEMS = 4;
constexpr int NM_SAMPLE_DRAW_PER_BLOCK = NM_SAMPLE_BLOCK * NM_SAMPLE_DRAW_ITEMS;
constexpr int NM_SAMPLE_LDS_COARSE = 2048;
static_assert(NM_SAMPLE_LDS_COARSE * 8 * (2048 / NM_SAMPLE_BLOCK) <= 160 * 1024, "eight resident workgroups' coarse tables fit a CU's LDS");

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ctr -> ctr in place
NM_SAMPLE_HD void nm_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0], p1 = (uint64_t)0xCD9E8D57u * ctr[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
        ctr[1] = (uint32_t)p1; ctr[3] = (uint32_t)p0; ctr[0] = n0; ctr[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// 53 bits of a pair of words -> [0, 1): every step is exact
NM_SAMPLE_HD double nm_sample_unit(uint32_t hi, uint32_t lo) {
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}
// the three uniforms of sample s of frame t
NM_SAMPLE_HD void nm_sample_uniforms(uint64_t seed, uint64_t s, uint32_t t, double u[3]) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c[4] = {(uint32_t)s, (uint32_t)(s >> 32), t, 0u};
    nm_philox4x32_10(c, k0, k1);
    u[0] = nm_sample_unit(c[0], c[1]); u[1] = nm_sample_unit(c[2], c[3]);
    uint32_t d[4] = {(uint32_t)s, (uint32_t)(s >> 32), t, 1u};
    nm_philox4x32_10(d, k0, k1);
    u[2] = nm_sample_unit(d[0], d[1]);
}
