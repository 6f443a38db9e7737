// Host check of nm_wgrad_plan.h, the launch plan of the weight gradients.  Plain C++, no GPU.
//  1. A pinned table (wgrad_plan_table.inc): kernel, grid, LDS bytes, S, slots and workspace floats of every conv layer of the default
//     network at 64^3 (4 frames) and of config 4 at 96^3 (16 frames) - channel counts rounded up to the 8-channel granule the tensors are
//     stored with - of every BWD_CASES entry of tests/test_grad_ops_gpu.py in conv modes 0, 1 and 3, of the shapes
//     tests/test_many_frames_gpu.py runs, of NM355_WGRAD_TR=0 and of wgrad_async 0 / 1 / 2 with and without `single`.  The rows were
//     written by the decision functions of the commit before the plan existed (plan_wgrad, w16z_takes, nm_launch_wgrad's inline tests,
//     nm_wgrad_ws_floats), compiled into a stand-alone program with the launch switches stubbed - not by this header.
//  2. Properties of every plan over a sweep of frames, extents, channels, kernel shapes, storages and switches.
//  3. The first layer's workspace layout.
// Prints one line per failure and a summary; exit status 0 only if everything holds.
#include "nm_wgrad_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace nm_wgrad;

static long g_checks = 0, g_bad = 0;
#define EXPECT(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_bad <= 40) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const char* const KERNEL_NAMES[] = {"WGRAD_TAPS", "WGRAD_POINT", "WGRAD_FIRST", "WGRAD_K1", "WGRAD16", "WGRAD16Z", "WGRAD16K2"};

struct Row {
    const char* tag; Call c; Switches sw;
    int status; const char* kernel; int grid_x, grid_y, threads; size_t lds; int S, slots; size_t ws_floats, reserve; const char* groups;
};
static const Row TABLE[] = {
#include "wgrad_plan_table.inc"
};

static void pinned_table() {
    for (const Row& r : TABLE) {
        const Plan q = plan(r.c, r.sw);
        EXPECT(q.status == r.status, "%s: status %d, pinned %d", r.tag, q.status, r.status);
        if (!r.c.first) {
            const size_t res = reserve_floats(r.c.N, r.c.OD, r.c.OH, r.c.OW, r.c.M, r.c.Nc, r.c.ks, r.c.stride, r.sw);
            EXPECT(res == r.reserve, "%s: reserve %zu, pinned %zu", r.tag, res, r.reserve);
        }
        if (q.status || r.status) continue;
        char groups[128] = "";
        if (q.n_groups > 1) {
            char* p = groups;
            for (int i = 0; i < q.n_groups; ++i) { const Group g = q.group(i); p += std::snprintf(p, groups + sizeof groups - p, "%s%d:%d:%d:%d", i ? "," : "", g.frame0, g.frames, g.S, g.slot0); }
        }
        EXPECT(!std::strcmp(KERNEL_NAMES[q.kernel], r.kernel) && q.grid_x == r.grid_x && q.grid_y == r.grid_y && q.threads == r.threads && q.lds == r.lds &&
               q.S == r.S && q.slots == r.slots && q.ws_floats == r.ws_floats && !std::strcmp(groups, r.groups),
               "%s: %s grid %d x %d, %d threads, lds %zu, S %d, slots %d, ws %zu, groups '%s'; pinned %s grid %d x %d, %d threads, lds %zu, S %d, slots %d, ws %zu, groups '%s'",
               r.tag, KERNEL_NAMES[q.kernel], q.grid_x, q.grid_y, q.threads, q.lds, q.S, q.slots, q.ws_floats, groups,
               r.kernel, r.grid_x, r.grid_y, r.threads, r.lds, r.S, r.slots, r.ws_floats, r.groups);
    }
}

// the instantiations the kernels have for bfloat16 operands
static bool bf16_instantiated(const Call& c, const Plan& q, const Switches& sw) {
    switch (q.kernel) {
    case WGRAD_TAPS: return c.ks == 2 && c.in_h;                    // wgrad_kernel<0, 2, true, dy_h>
    case WGRAD_FIRST: return !c.in_h;                               // wgrad_kernel<2, 7, false, true>
    case WGRAD_K1: return c.in_h && c.dy_h;                         // wgrad_k1_kernel<NTW, true>
    case WGRAD16Z: return c.in_h && c.dy_h && sw.single;            // wgrad16z_kernel<true, true>
    case WGRAD16K2: return sw.single && c.in_h;                     // wgrad16k2_kernel<MT, true, true, dy_h>
    default: return false;                                          // wgrad_kernel<1>, wgrad16_kernel: fp32 operands only
    }
}

static void check_plan(const Call& c, const Switches& sw, size_t reserve) {
    const Plan q = plan(c, sw);
    if (q.status) { EXPECT(q.status == ERR_ARG || q.status == ERR_UNSUPPORTED, "status %d", q.status); return; }
    const int tiles = q.m_tiles * q.n_tiles;
    const auto where = [&]() {
        static char b[256];
        std::snprintf(b, sizeof b, "N=%d %dx%dx%d in %dx%dx%d M=%d Nc=%d k%d s%d p%d f16=%d h=%d%d sw=%d,%d,%d,%d %s", c.N, c.OD, c.OH, c.OW, c.ID, c.IH, c.IW, c.M, c.Nc,
                      c.ks, c.stride, c.pad, c.allow_f16, c.in_h, c.dy_h, sw.wgrad_tr, sw.wgrad_async, sw.single, sw.store16, KERNEL_NAMES[q.kernel]);
        return b;
    };
    EXPECT(q.S >= 1 && q.slots >= 1 && q.grid_x >= 1 && q.grid_y >= 1, "%s: S %d slots %d grid %d x %d", where(), q.S, q.slots, q.grid_x, q.grid_y);
    EXPECT((size_t)q.slots * tiles * q.groups * 1024 <= q.ws_floats, "%s: slots %d tiles %d groups %d, ws %zu", where(), q.slots, tiles, q.groups, q.ws_floats);
    EXPECT(q.ws_floats <= reserve, "%s: ws %zu above the reservation %zu", where(), q.ws_floats, reserve);
    EXPECT(q.lds <= 163840, "%s: lds %zu", where(), q.lds);
    if (c.in_h || c.dy_h) EXPECT(bf16_instantiated(c, q, sw), "%s: no bfloat16 instantiation", where());
    EXPECT(q.n_groups == 1 || q.kernel == WGRAD16Z, "%s: %d groups", where(), q.n_groups);
    // frame groups: a partition of [0, N) in order, at most 96 frames each, sizes within one of each other; slot ranges back to back
    int frame = 0, slot = 0, lo = c.N, hi = 0;
    for (int i = 0; i < q.n_groups; ++i) {
        const Group g = q.group(i);
        EXPECT(g.frame0 == frame && g.slot0 == slot && g.frames >= 1 && g.S >= 1, "%s: group %d = (%d, %d, %d, %d) after frame %d slot %d", where(), i, g.frame0, g.frames, g.S, g.slot0, frame, slot);
        frame += g.frames; slot += g.S;
        lo = g.frames < lo ? g.frames : lo; hi = g.frames > hi ? g.frames : hi;
        if (q.kernel == WGRAD16Z) {
            EXPECT(g.frames <= 96 && g.S <= g.frames * q.nby * q.nbx && w16z_lds(g.frames) <= 163840, "%s: group %d of %d frames, S %d", where(), i, g.frames, g.S);
        }
    }
    EXPECT(frame == c.N && hi - lo <= 1, "%s: groups cover %d frames, sizes %d..%d", where(), frame, lo, hi);
    if (q.kernel == WGRAD16Z) {
        EXPECT(slot == q.slots && q.nbz >= 2, "%s: group slots %d, plan %d, nbz %d", where(), slot, q.slots, q.nbz);
    }
}

static void sweep() {
    static const int CH[] = {4, 8, 32, 40, 48, 72, 128, 176, 256};
    static const int KSP[][3] = {{1, 1, 0}, {3, 1, 1}, {2, 2, 0}, {3, 2, 1}, {5, 1, 2}};
    // cubes 1 .. 40 and non-cubic extents (one brick deep, ragged bricks, whole bricks)
    static int EXT[52][3];
    int n_ext = 0;
    for (int g = 1; g <= 40; ++g) { EXT[n_ext][0] = EXT[n_ext][1] = EXT[n_ext][2] = g; ++n_ext; }
    static const int ODD[][3] = {{2, 8, 8}, {4, 8, 8}, {4, 8, 16}, {6, 16, 8}, {1, 8, 8}, {3, 5, 7}, {40, 8, 24}, {16, 24, 40}, {2, 40, 40}, {5, 16, 16}, {12, 12, 40}, {8, 1, 33}};
    for (const auto& o : ODD) { EXT[n_ext][0] = o[0]; EXT[n_ext][1] = o[1]; EXT[n_ext][2] = o[2]; ++n_ext; }
    static int FRAMES[202];
    for (int i = 0; i < 200; ++i) FRAMES[i] = i + 1;
    FRAMES[200] = 240; FRAMES[201] = 385;
    Switches sws[24];
    int n_sw = 0;
    for (int tr = 0; tr < 2; ++tr) for (int as = 0; as < 3; ++as) for (int mode = 0; mode < 3; ++mode) sws[n_sw++] = {tr, as, mode >= 1, mode == 2};     // (store16 comes with single)
    long plans = 0;
    for (int fi = 0; fi < 202; ++fi)
        for (int e = 0; e < n_ext; ++e) {
            // (the full cross product is 10^9 plans: every frame count meets every extent, the channel pairs and switch sets rotate)
            const int N = FRAMES[fi], *o = EXT[e];
            for (const auto& k : KSP) {
                const int M = CH[(fi + e) % 9], Nc = CH[(fi * 5 + e * 2 + k[0]) % 9];
                for (int s = 0; s < 2; ++s) {
                    const Switches& sw = sws[(fi * 7 + e * 3 + s * 11 + k[0]) % n_sw];
                    const size_t reserve = reserve_floats(N, o[0], o[1], o[2], M, Nc, k[0], k[1], sw);
                    for (int geom = 0; geom < 3; ++geom)            // input extents: as the conv gives them, equal, twice
                        for (int v = 0; v < 8; ++v) {
                            Call c = {N, o[0], o[1], o[2], 0, 0, 0, M, Nc, k[0], k[1], k[2], (v & 1) != 0, (v & 2) != 0, (v & 4) != 0, false};
                            const int us = geom == 2 ? 2 : 1;
                            c.ID = geom ? us * o[0] : (o[0] - 1) * k[1] + k[0] - 2 * k[2]; c.IH = geom ? us * o[1] : (o[1] - 1) * k[1] + k[0] - 2 * k[2];
                            c.IW = geom ? us * o[2] : (o[2] - 1) * k[1] + k[0] - 2 * k[2];
                            check_plan(c, sw, reserve);
                            ++plans;
                        }
                }
            }
        }
    // every channel pair and every switch set at the frame counts and extents where the decisions change
    static const int NS[] = {1, 2, 49, 96, 97, 192, 193, 196, 200, 240, 385};
    static const int ES[][3] = {{2, 8, 8}, {4, 8, 8}, {8, 8, 8}, {16, 16, 16}, {32, 32, 32}, {5, 5, 5}, {40, 40, 40}, {1, 1, 1}, {4, 4, 4}};
    for (int N : NS) for (const auto& o : ES) for (int M : CH) for (int Nc : CH) for (const auto& k : KSP) for (int s = 0; s < n_sw; ++s) {
        const size_t reserve = reserve_floats(N, o[0], o[1], o[2], M, Nc, k[0], k[1], sws[s]);
        for (int geom = 1; geom < 3; ++geom) for (int v = 0; v < 8; ++v) {
            const Call c = {N, o[0], o[1], o[2], geom * o[0], geom * o[1], geom * o[2], M, Nc, k[0], k[1], k[2], (v & 1) != 0, (v & 2) != 0, (v & 4) != 0, false};
            check_plan(c, sws[s], reserve);
            ++plans;
        }
    }
    std::printf("sweep: %ld plans\n", plans);
}

static void first_layer() {
    const Switches sw = {1, 1, false, false};
    for (int G : {12, 16, 24, 32, 40, 64, 96}) for (int N = 1; N <= 100; ++N) for (int M : {32, 64}) {
        const FirstLayout l = first_layout(N, G, M, sw);
        const size_t G3 = (size_t)G * G * G, dense = plan(first_call(1, G, M, false), sw).ws_floats, reserve = first_reserve_floats(N, G, M, sw);
        EXPECT(l.dysum + G3 * M <= l.zocc && l.zocc + G3 <= l.dense_ws && l.dense_ws + dense <= l.part && l.part + (size_t)N * l.chunks * 125 * M <= l.total && l.total <= reserve,
               "first layer G=%d N=%d M=%d: %zu | %zu | %zu | %zu | %zu, reserve %zu", G, N, M, l.dysum, l.zocc, l.dense_ws, l.part, l.total, reserve);
        EXPECT((size_t)l.chunks * K5S_CHUNK_VOXELS >= G3, "first layer G=%d: %d chunks", G, l.chunks);
        const Plan q = plan(first_call(N, G, M, false), sw);
        EXPECT(!q.status && q.kernel == WGRAD_FIRST && q.ws_floats <= reserve, "first layer G=%d N=%d M=%d: dense status %d ws %zu reserve %zu", G, N, M, q.status, q.ws_floats, reserve);
    }
}

int main() {
    pinned_table();
    std::printf("pinned table: %zu rows\n", sizeof TABLE / sizeof TABLE[0]);
    sweep();
    first_layer();
    std::printf("%ld checks, %ld failed: %s\n", g_checks, g_bad, g_bad ? "FAILED" : "all plans hold");
    return g_bad ? 1 : 0;
}
