// Which brick a persistent workgroup processes in each of its steps: the one walk that conv_f16s and the five producer / consumer
// kernels (conv_f16p, _f16p2, _f16p8, _f16q2, _f16r) share, and the host's choice of the order.  Plain integer C++ (no HIP headers
// needed on the host): tests/cpp/brick_walk.cpp walks every workgroup of a launch with these same functions.
#pragma once

#ifdef __HIPCC__
#define NM_PLAN_FN __host__ __device__ constexpr
#define NM_WALK_FN __host__ __device__ __forceinline__
#else
#define NM_PLAN_FN constexpr
#define NM_WALK_FN inline
#endif

namespace nm_walk {

// position of a role in its workgroup's run of `items` work items of C16 channel chunks each
struct Cursor { int item, cb; };
// advances to the next step; false (cursor unchanged) on the run's last step
NM_PLAN_FN bool next_step(Cursor& c, int items, int C16) {
    if (c.cb + 1 < C16) { ++c.cb; return true; }
    if (c.item + 1 >= items) return false;
    c.cb = 0; ++c.item;
    return true;
}

// XCD super-tile in bricks (x == 0: bricks in linear order), see super_tile_item
struct SuperTile {
    int z, y, x;
    unsigned sx, sy, pf;          // super-tiles per row / column / frame, and ceil(2^32 / d) of each (0: d = 1): the three divisions of a brick
    unsigned m_sx, m_sy, m_pf;    // decode as multiplications (round 6); pf == 0: the host could not prove them exact, plain divisions
};

NM_WALK_FN unsigned umulhi(unsigned x, unsigned m) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(x, m);
#else
    return (unsigned)(((unsigned long long)x * m) >> 32);
#endif
}

// Which brick a persistent workgroup processes in its iteration tau.  The eight XCDs have separate L2s and a brick's
// 6x10x10 halo is 2.3x its 4x8x8 outputs, so in linear order (each workgroup a contiguous run of bricks, the 32 CUs of an
// XCD far apart in the volume) the input is fetched from HBM about twice; conv 64^3 x 32 channels moved 8-10 GB per
// launch for 4.3 GB of tensors.  Here the workgroups of one XCD (blockIdx % 8 is the XCD label) take, at the same time,
// the st.z x st.y x st.x bricks of one super-tile (one brick per workgroup, 64 or 32 of them), and consecutive iterations
// walk neighbouring super-tiles of the same frame, so halos shared between neighbouring bricks are served by that L2.
struct BrickPos { int n, bz, by, bx; };
NM_WALK_FN BrickPos super_tile_item(const SuperTile& st, int b, int tau, int per, int nbz, int nby, int nbx) {
    BrickPos r;
    if (st.x == 0) {
        const int nbr = nbz * nby * nbx, item = b * per + tau;
        r.n = item / nbr; const int br = item % nbr;
        r.bx = br % nbx; r.by = (br / nbx) % nby; r.bz = br / (nbx * nby);
        return r;
    }
    const int l = b >> 3, S = (b & 7) * per + tau;
    if (st.pf) {
        // (round 6) a persistent workgroup decodes every brick it walks - nine integer divisions by launch constants, ~250 vector
        // instructions and a dozen hoisted reciprocal registers per wave, in the MFMA waves' path between two steps (in-kernel stamps of
        // conv_f16p: 720 of a 9 800-tick step).  The super-tile is always 4 x 4 bricks in (y, x); the three real divisions are by host
        // constants: q = umulhi(x, ceil(2^32 / d)), exact while x d < 2^32 (checked by choose_super_tile).
        auto fdiv = [](unsigned x, unsigned m) { return m ? umulhi(x, m) : x; };
        const unsigned n = fdiv((unsigned)S, st.m_pf), si = (unsigned)S - n * st.pf;
        const unsigned q = fdiv(si, st.m_sx), sx = si - q * st.sx;
        const unsigned sz = fdiv(q, st.m_sy), sy = q - sz * st.sy;
        r.n = (int)n; r.bx = (int)(sx * 4u) + (l & 3); r.by = (int)(sy * 4u) + ((l >> 2) & 3); r.bz = (int)sz * st.z + (l >> 4);
        return r;
    }
    const int SX = nbx / st.x, SY = nby / st.y, stpf = SX * SY * (nbz / st.z);
    r.n = S / stpf; const int si = S % stpf;
    r.bx = (si % SX) * st.x + l % st.x;
    r.by = ((si / SX) % SY) * st.y + (l / st.x) % st.y;
    r.bz = (si / (SX * SY)) * st.z + l / (st.x * st.y);
    return r;
}

// Host: the super-tile of a launch of nblocks persistent workgroups over N frames of nbz x nby x nbx bricks.  The grid must be
// 8 x (bricks per super-tile) workgroups, the brick grid a multiple of the super-tile, and the super-tiles split evenly over the
// eight XCDs; anything else walks in linear order (all zero).
inline SuperTile choose_super_tile(int N, int nblocks, int nbz, int nby, int nbx) {
    SuperTile t = {0, 0, 0, 0u, 0u, 0u, 0u, 0u, 0u};
    if (nblocks % 8) return t;
    const int gs = nblocks / 8;
    const int sz = gs == 64 ? 4 : gs == 32 ? 2 : 0;
    if (!sz || nbz % sz || nby % 4 || nbx % 4) return t;
    const long long st = (long long)N * (nbz / sz) * (nby / 4) * (nbx / 4);
    if (st % 8 || st / 8 * nblocks != (long long)N * nbz * nby * nbx) return t;
    t.z = sz; t.y = 4; t.x = 4;
    // the decode's divisions as multiplications (super_tile_item): exact while (largest dividend) x (divisor) < 2^32
    const unsigned SX = (unsigned)nbx / 4u, SY = (unsigned)nby / 4u, pf = SX * SY * (unsigned)(nbz / sz);
    const unsigned long long smax = 8ull * (unsigned long long)(((long long)N * nbz * nby * nbx + nblocks - 1) / nblocks) + 8ull;
    auto magic = [](unsigned d) { return d == 1u ? 0u : (unsigned)((0x100000000ull + d - 1ull) / d); };
    if (smax * pf < 0x100000000ull) {
        t.sx = SX; t.sy = SY; t.pf = pf; t.m_sx = magic(SX); t.m_sy = magic(SY); t.m_pf = magic(pf);
    }
    return t;
}

// a work item: a brick of BZ x 8 x 8 output voxels at (oz0, oy0, ox0) of frame n and, where a layer has several, one group of
// output channels of it
template <bool CG> struct Work;
template <> struct Work<false> { int n, oz0, oy0, ox0; };
template <> struct Work<true> { int n, oz0, oy0, ox0, cg; };

// The flat stream of steps (work item, 16-channel chunk) of workgroup b of a grid: a contiguous run of ceil(total / grid) work
// items.  BZ: the brick's z extent (4 | 8); CG: the items of a brick are its ncg output-channel groups, back to back (its input
// stays in L2).  The XCD super-tile order exists for ncg == 1 only.
template <int BZ, bool CG>
struct Walk {
    static_assert(BZ == 4 || BZ == 8, "bricks are 4 x 8 x 8 or 8 x 8 x 8");
    using Work = nm_walk::Work<CG>;
    struct Step { Work w; Cursor c; };
    const SuperTile& st;                                            // the launch's own (it must outlive the walk): read where it is used - a copy costs the kernels SGPRs
    int OD, OH, OW, nbz, nby, nbx, nbr, ncg, C16, b, per, id_first, items;

    NM_WALK_FN Walk(const SuperTile& st_, int N, int OD_, int OH_, int OW_, int ncg_, int C16_, int b_, int grid)
        : st(st_), OD(OD_), OH(OH_), OW(OW_), nbz(OD_ >> (BZ == 8 ? 3 : 2)), nby(OH_ >> 3), nbx(OW_ >> 3), nbr(nbx * nby * nbz), ncg(CG ? ncg_ : 1), C16(C16_), b(b_) {
        const int total = N * nbr * ncg;
        per = (total + grid - 1) / grid;
        id_first = b * per;
        items = (total < id_first + per ? total : id_first + per) - id_first;       // <= 0: the workgroup has nothing to do
    }
    NM_WALK_FN bool tiled() const { return st.x != 0; }
    NM_WALK_FN Work decode(int item) const {
        Work w;
        if (tiled()) {
            const BrickPos bp = super_tile_item(st, b, item, per, nbz, nby, nbx);
            if constexpr (CG) w.cg = 0;
            w.n = bp.n; w.ox0 = bp.bx << 3; w.oy0 = bp.by << 3; w.oz0 = bp.bz * BZ;
            return w;
        }
        int bid = id_first + item;
        if constexpr (CG) { w.cg = bid % ncg; bid /= ncg; }
        w.n = bid / nbr; const int br = bid % nbr;
        w.ox0 = (br % nbx) << 3; w.oy0 = ((br / nbx) % nby) << 3; w.oz0 = (br / (nbx * nby)) * BZ;
        return w;
    }
    NM_WALK_FN Work next_work(Work w, int item) const {            // work item `item` from item - 1 (linear order: no divisions)
        if (tiled()) return decode(item);
        if constexpr (CG) { if (++w.cg != ncg) return w; w.cg = 0; }
        if ((w.ox0 += 8) == OW) { w.ox0 = 0; if ((w.oy0 += 8) == OH) { w.oy0 = 0; if ((w.oz0 += BZ) == OD) { w.oz0 = 0; ++w.n; } } }
        return w;
    }
    NM_WALK_FN Step first() const { Step s; s.w = decode(0); s.c.item = 0; s.c.cb = 0; return s; }
    NM_WALK_FN bool advance(Step& s) const {                       // false (and s unchanged) on the workgroup's last step
        const int item = s.c.item;
        if (!next_step(s.c, items, C16)) return false;
        if (s.c.item != item) s.w = next_work(s.w, s.c.item);
        return true;
    }
};

}  // namespace nm_walk
