// Host check of nm_brick_walk.h, the walk that the persistent conv kernels take their bricks from: every workgroup of a launch is walked
// with the kernels' own functions (Walk::first / advance / decode / next_work, super_tile_item, choose_super_tile).  Over all workgroups
// together every (frame, brick, cout group, chunk) must be visited exactly once; next_work must equal decode at every item; advance must
// return false exactly on a workgroup's last step and leave the step unchanged there; a workgroup with an empty range makes no step.
// Plain C++, no GPU.  Prints one line per case; exit status 0 only if every case holds.
#include "nm_brick_walk.h"

#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace nm_walk;

static int g_cases = 0, g_bad = 0;

template <int BZ, bool CG>
static void walk_case(const char* what, const SuperTile& st, int N, int OD, int OH, int OW, int ncg, int C16, int grid, bool want_tiled) {
    const int nbr = (OD / BZ) * (OH / 8) * (OW / 8), total = N * nbr * ncg;
    std::vector<int> seen((size_t)total * C16, 0);
    int bad = 0;
    for (int b = 0; b < grid; ++b) {
        const Walk<BZ, CG> wk(st, N, OD, OH, OW, ncg, C16, b, grid);
        if (wk.tiled() != want_tiled) ++bad;
        const bool empty = b * wk.per >= total;
        if (empty != (wk.items <= 0)) ++bad;
        if (wk.items <= 0) continue;                                // (the kernels return before their first step)
        typename Walk<BZ, CG>::Step s = wk.first();
        long steps = 0;
        for (;;) {
            ++steps;
            const typename Walk<BZ, CG>::Work d = wk.decode(s.c.item);
            if (std::memcmp(&d, &s.w, sizeof d) != 0) ++bad;        // next_work == decode
            int cg = 0;
            if constexpr (CG) cg = s.w.cg;
            const bool in = s.w.n >= 0 && s.w.n < N && s.w.oz0 >= 0 && s.w.oz0 < OD && s.w.oz0 % BZ == 0 && s.w.oy0 >= 0 && s.w.oy0 < OH && s.w.oy0 % 8 == 0 &&
                            s.w.ox0 >= 0 && s.w.ox0 < OW && s.w.ox0 % 8 == 0 && cg >= 0 && cg < ncg && s.c.cb >= 0 && s.c.cb < C16;
            if (!in) { ++bad; break; }
            const int br = ((s.w.oz0 / BZ) * (OH / 8) + s.w.oy0 / 8) * (OW / 8) + s.w.ox0 / 8;
            ++seen[(((size_t)s.w.n * nbr + br) * ncg + cg) * C16 + s.c.cb];
            typename Walk<BZ, CG>::Step t = s;
            const bool more = wk.advance(t);
            const bool last = s.c.item == wk.items - 1 && s.c.cb == C16 - 1;
            if (more == last) ++bad;                                // false exactly on the last step ...
            if (!more) { if (std::memcmp(&t, &s, sizeof t) != 0) ++bad; break; }     // ... which it leaves unchanged
            s = t;
        }
        if (steps != (long)wk.items * C16) ++bad;
    }
    for (int v : seen) if (v != 1) ++bad;
    ++g_cases; g_bad += bad ? 1 : 0;
    std::printf("%s BZ=%d cg=%d/%d N=%d %dx%dx%d C16=%d grid=%d %s\n", what, BZ, CG ? 1 : 0, ncg, N, OD, OH, OW, C16, grid, bad ? "FAILED" : "ok");
}

template <int BZ>
static void both_forms(const char* what, const SuperTile& st, int N, int OD, int OH, int OW, int C16, int grid, bool tiled) {
    walk_case<BZ, false>(what, st, N, OD, OH, OW, 1, C16, grid, tiled);
    walk_case<BZ, true>(what, st, N, OD, OH, OW, 1, C16, grid, tiled);
}

template <int BZ>
static void tiled_case(int N, int G, bool plain_division) {
    SuperTile st = choose_super_tile(N, 256, G / BZ, G / 8, G / 8);
    const bool want = st.x == 4 && st.y == 4 && st.z == 2 && st.pf != 0;
    if (!want) { ++g_cases; ++g_bad; std::printf("choose_super_tile BZ=%d N=%d %d^3: z=%d y=%d x=%d pf=%u FAILED\n", BZ, N, G, st.z, st.y, st.x, st.pf); return; }
    if (plain_division) st.pf = 0;
    for (int C16 : {1, 2, 8}) both_forms<BZ>(plain_division ? "tiled/div" : "tiled", st, N, G, G, G, C16, 256, true);
}

int main() {
    const SuperTile lin = {0, 0, 0, 0u, 0u, 0u, 0u, 0u, 0u};
    const int shapes[3][3] = {{16, 8, 8}, {16, 16, 24}, {24, 16, 8}};
    for (const auto& s : shapes)
        for (int N : {1, 3})
            for (int C16 : {1, 2, 8})
                for (int ncg : {0, 1, 2, 3}) {                     // 0: the walk without a cout-group digit
                    auto run = [&](auto BZc) {
                        constexpr int BZ = decltype(BZc)::value;
                        const int total = N * (s[0] / BZ) * (s[1] / 8) * (s[2] / 8) * (ncg ? ncg : 1);
                        for (int grid : {1, 3, 7, 64, total + 5}) {
                            if (ncg) walk_case<BZ, true>("linear", lin, N, s[0], s[1], s[2], ncg, C16, grid, false);
                            else walk_case<BZ, false>("linear", lin, N, s[0], s[1], s[2], 1, C16, grid, false);
                        }
                    };
                    run(std::integral_constant<int, 4>{});
                    run(std::integral_constant<int, 8>{});
                }
    // the XCD super-tile order at 256 workgroups
    { const SuperTile t = choose_super_tile(2, 256, 8, 4, 4); if (t.x != 4 || t.z != 2) { ++g_bad; std::printf("32^3, 4-deep bricks: st_x=%d st_z=%d FAILED\n", t.x, t.z); } }
    tiled_case<4>(2, 32, false); tiled_case<4>(4, 32, false);
    tiled_case<8>(4, 32, false); tiled_case<8>(8, 32, false);
    tiled_case<4>(4, 64, false); tiled_case<8>(4, 64, false);
    tiled_case<4>(16, 64, false); tiled_case<4>(16, 64, true);    // the multiply-high decode and the plain divisions agree with one walk's answer
    // ... and with each other, item by item
    {
        SuperTile m = choose_super_tile(16, 256, 16, 8, 8), d = m;
        d.pf = 0;
        int bad = m.pf == 0;
        const int per = 16 * 16 * 8 * 8 / 256;
        for (int b = 0; b < 256; ++b)
            for (int tau = 0; tau < per; ++tau) {
                const BrickPos a = super_tile_item(m, b, tau, per, 16, 8, 8), c = super_tile_item(d, b, tau, per, 16, 8, 8);
                if (a.n != c.n || a.bz != c.bz || a.by != c.by || a.bx != c.bx) ++bad;
            }
        ++g_cases; g_bad += bad ? 1 : 0;
        std::printf("64^3 N=16 umulhi twin against plain division %s\n", bad ? "FAILED" : "ok");
    }
    std::printf("%d cases, %d failed: %s\n", g_cases, g_bad, g_bad ? "FAILED" : "all walks hold");
    return g_bad ? 1 : 0;
}
