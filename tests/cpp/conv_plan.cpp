// Host check of nm_conv_plan.h, the launch plan of the forward convs.  Plain C++, no GPU.
//  1. A pinned table (conv_plan_table.inc): kernel, instantiation, status, grid, LDS bytes, every ConvParams integer, the super tile,
//     the profiler variant and FLOPs factor, the GroupNorm partial rows and conv_up2c's sub-plan.  The rows were written by the decision
//     code of the commit before the plan existed, not by this header (see the table's header comment).
//  2. Properties of every plan over a sweep of frames, extents, channels, kernel shapes, storages and switches.
//  3. The three routing queries of nm_net.hip against the full plan.
// Prints one line per failure and a summary; exit status 0 only if everything holds.
#include "nm_conv_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace nm_conv_plan;

static long g_checks = 0, g_bad = 0;
#define EXPECT(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_bad <= 40) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const char* const KERNEL_NAMES[] = {"CONV_MFMA", "CONV_F16S", "CONV_POOL_F16S", "CONV_POOL_F16Q", "CONV_F16P", "CONV_F16P2", "CONV_F16P8", "CONV_F16Q2", "CONV_F16R", "CONV_UP2C"};

// A pinned row: the call in short (Co_pad is Cout rounded up to 32; flags: 1 up2, 2 have_w16, 4 have_up2c, 8 in_h, 16 out_h, 32 has_in2,
// 64 has_map, 128 has_alt), the switches, and what the previous launchers did with it
struct ShortCall { int N, ID, IH, IW, Cin, cin_real, Cout, ks, stride, pad, flags, wgs_cap, cus; };
struct Row {
    const char* tag; ShortCall sc; Switches sw;
    int status, kernel;         // Kernel; a refused row: the family its message names, -1 if none (argument errors, the LDS tile)
    int inst[8];                // MT, NT, KS, UP2, SINGLE, IO, C16T, IN2: compared where the launched kernel's template takes them (INST_MASK)
    int grid_x, grid_y, threads, lds;
    int params[15];             // bz_l2, by_l2, bx_l2, nbz, nby, nbx, KC, HZ, HY, HX, HV, HVp, CVp, ZP, ksplit; conv_up2c: main, march, ypad, main grid, face, R, face grid, face LDS, edge, edge grid, slot0
    unsigned st[6];             // z, y, x, sx, sy, pf (the three multipliers are ceil(2^32 / d) of the last three)
    int w_f16, w16, variant, taps2 /* 2 x taps x FLOPs factor */, part_rows;
};
#define M0 {0, false, false, 1, 1, 1, 1, 1, 1}
#define M1 {1, false, false, 1, 1, 1, 1, 1, 1}
#define M2 {1, true, false, 1, 1, 1, 1, 1, 1}
#define M3 {1, false, true, 1, 1, 1, 1, 1, 1}
static const Row TABLE[] = {
#include "conv_plan_table.inc"
};
// template parameters per kernel, as bits of inst[]:       mfma      f16s                 pool_f16s  pool_f16q       f16p      p2 p8 q2      f16r      up2c (conv_up2c_kernel<IO>)
static const int INST_MASK[] = {1 | 2, 2 | 4 | 8 | 16 | 32, 2 | 16, 2 | 16 | 32 | 128, 16 | 32, 0, 0, 32, 32 | 64, 0};

static void pinned_table() {
    for (const Row& r : TABLE) {
        const ShortCall& s = r.sc;
        const Call c = {s.N, s.ID, s.IH, s.IW, s.Cin, s.cin_real, s.Cout, (s.Cout + 31) & ~31, s.ks, s.stride, s.pad, (s.flags & 1) != 0, (s.flags & 2) != 0, (s.flags & 4) != 0,
                        (s.flags & 8) != 0, (s.flags & 16) != 0, (s.flags & 32) != 0, (s.flags & 64) != 0, (s.flags & 128) != 0, s.wgs_cap, s.cus};
        const Plan q = plan(c, r.sw);
        EXPECT(q.status == r.status, "%s: status %d, pinned %d", r.tag, q.status, r.status);
        EXPECT(q.part_rows == r.part_rows || r.status == ERR_ARG, "%s: part_rows %d, pinned %d", r.tag, q.part_rows, r.part_rows);
        EXPECT(r.kernel < 0 || q.kernel == r.kernel, "%s: %s, pinned %s", r.tag, KERNEL_NAMES[q.kernel], r.kernel < 0 ? "" : KERNEL_NAMES[r.kernel]);
        if (q.status || r.status) continue;
        const int inst[8] = {q.MT, q.NT, q.KS, q.UP2, q.SINGLE, q.IO, q.C16T, q.IN2};
        for (int i = 0; i < 8; ++i) EXPECT(!(INST_MASK[q.kernel] >> i & 1) || inst[i] == r.inst[i], "%s: instantiation field %d is %d, pinned %d", r.tag, i, inst[i], r.inst[i]);
        EXPECT(q.grid_x == r.grid_x && q.grid_y == r.grid_y && q.threads == r.threads && q.lds == (size_t)r.lds, "%s: grid %d x %d, %d threads, lds %zu; pinned %d x %d, %d, %d",
               r.tag, q.grid_x, q.grid_y, q.threads, q.lds, r.grid_x, r.grid_y, r.threads, r.lds);
        EXPECT(q.variant == r.variant && (int)(2 * q.taps * q.flops_factor) == r.taps2, "%s: variant %d taps %d x %g; pinned %d, %d / 2", r.tag, q.variant, q.taps, q.flops_factor, r.variant, r.taps2);
        const Up2cPlan& u = q.up;
        const nm_walk::SuperTile& t = q.st;
        auto magic = [](unsigned d) { return d <= 1u ? 0u : (unsigned)((0x100000000ull + d - 1ull) / d); };
        const int up[15] = {u.main, u.march, u.ypad, u.main_grid, u.face, u.R, u.face_grid, (int)u.face_lds, u.edge, u.edge_grid, u.slot0, 0, 0, 0, 0};
        const int conv[15] = {q.bz_l2, q.by_l2, q.bx_l2, q.nbz, q.nby, q.nbx, q.KC, q.HZ, q.HY, q.HX, q.HV, q.HVp, q.CVp, q.ZP, q.ksplit};
        const int* params = q.kernel == CONV_UP2C ? up : conv;
        for (int i = 0; i < 15; ++i) EXPECT(params[i] == r.params[i], "%s: %s integer %d is %d, pinned %d", r.tag, q.kernel == CONV_UP2C ? "sub-plan" : "ConvParams", i, params[i], r.params[i]);
        if (q.kernel == CONV_UP2C) { EXPECT(q.IO == r.inst[5] || u.main != UP2C_ONE, "%s: conv_up2c_kernel<%d>, pinned %d", r.tag, q.IO, r.inst[5]); continue; }
        const unsigned st[6] = {(unsigned)t.z, (unsigned)t.y, (unsigned)t.x, t.sx, t.sy, t.pf};
        for (int i = 0; i < 6; ++i) EXPECT(st[i] == r.st[i], "%s: super tile field %d is %u, pinned %u", r.tag, i, st[i], r.st[i]);
        EXPECT(t.pf ? t.m_sx == magic(t.sx) && t.m_sy == magic(t.sy) && t.m_pf == magic(t.pf) : !(t.m_sx | t.m_sy | t.m_pf | t.sx | t.sy), "%s: super tile multipliers", r.tag);
        EXPECT(q.w_f16 == (r.w_f16 != 0) && q.w16 == (r.w16 != 0), "%s: w_f16 %d w16 %d, pinned %d %d", r.tag, q.w_f16, q.w16, r.w_f16, r.w16);
    }
}

// the instantiations the kernels have for bfloat16 tensors (io: bit 0 input, bit 1 output), from the kernels' template lists
static bool bf16_instantiated(const Call& c, const Plan& q, const Switches& sw, int io) {
    switch (q.kernel) {
    case CONV_F16S: return sw.single && ((q.KS == 1 && !q.UP2 && io == 3) || (q.KS == 3 && q.UP2 && q.NT == 2 && io == 2));    // conv_f16s_kernel<2, NT, 1, false, true, 3>, <2, 2, 3, true, true, 2>
    case CONV_POOL_F16Q: return sw.single && (io == 1 || io == 3) && !q.IN2 && c.Cin <= 128;     // conv_pool_f16q_kernel<NT, true, false, 1 | 3>
    case CONV_F16P: return sw.single && io == 3;                    // conv_f16p_kernel<true, 3>
    case CONV_F16Q2: return io == 3;                                // conv_f16q2_kernel<3>
    case CONV_F16R: return io == 3;                                 // conv_f16r_kernel<3, 2 | 4>
    case CONV_UP2C: return q.up.main == UP2C_ONE && q.up.face == FACE && q.up.edge == EDGE;      // conv_up2c_kernel<io>, conv_up2c_face_kernel<true, io>, conv_up2c_edge_kernel<true, io>
    default: return false;                                          // conv_mfma, conv_pool_f16s, conv_f16p2, conv_f16p8: fp32 tensors only
    }
}

static long g_plans = 0, g_taken = 0;
static void check_plan(const Call& c, const Switches& sw) {
    const Plan q = plan(c, sw);
    ++g_plans;
    char where[320];
    std::snprintf(where, sizeof where, "N=%d in %dx%dx%d Cin=%d Cout=%d/%d k%d s%d p%d up2=%d w16=%d up2c=%d h=%d%d in2=%d map=%d%d cap=%d cus=%d sw=%d,%d,%d,%d,%d,%d,%d,%d,%d %s", c.N, c.ID, c.IH, c.IW, c.Cin,
                  c.Cout, c.Co_pad, c.ks, c.stride, c.pad, c.up2, c.have_w16, c.have_up2c, c.in_h, c.out_h, c.has_in2, c.has_map, c.has_alt, c.wgs_cap, c.cus,
                  sw.conv_mode, sw.f16p_all, sw.single, sw.pool_q, sw.f16r, sw.up2y, sw.up2y_march, sw.up2y_ypad, sw.up2c_shell, KERNEL_NAMES[q.kernel]);
    // the fp32 retry of nm_op_conv3d: conv mode 0, no composite sets, into the rows reserved for this plan
    if (q.status != ERR_ARG && !c.has_in2 && !c.has_map) {
        Call c0 = c; c0.have_up2c = false; c0.in_h = c0.out_h = false;
        const Plan q0 = plan(c0, Switches{0, false, false, sw.pool_q, sw.f16r, sw.up2y, sw.up2y_march, sw.up2y_ypad, sw.up2c_shell});
        EXPECT(q0.part_rows <= q.part_rows && q0.kernel == CONV_MFMA, "%s: the conv mode 0 plan writes %d rows, this one %d", where, q0.part_rows, q.part_rows);
    }
    if (q.status) { EXPECT(q.status == ERR_ARG || q.status == ERR_UNSUPPORTED, "%s: status %d", where, q.status); return; }
    ++g_taken;
    const int io = (c.in_h ? 1 : 0) | (c.out_h ? 2 : 0);
    EXPECT(q.lds <= 163840 && q.up.face_lds <= 163840, "%s: lds %zu / %zu", where, q.lds, q.up.face_lds);
    EXPECT(q.grid_x >= 1 && q.grid_y >= 1 && q.threads >= 1, "%s: grid %d x %d", where, q.grid_x, q.grid_y);
    if (io) EXPECT(bf16_instantiated(c, q, sw, io), "%s: no bfloat16 instantiation", where);
    const int bricks = (q.OD / 4) * (q.OH / 8) * (q.OW / 8);
    switch (q.kernel) {
    case CONV_MFMA: case CONV_F16S: case CONV_POOL_F16S: case CONV_POOL_F16Q:
        // the kernels' row index is the tiling's brick number; every output voxel lies in one of its bricks
        EXPECT(q.part_rows == q.nbz * q.nby * q.nbx && (q.nbz << q.bz_l2) >= q.OD && (q.nby << q.by_l2) >= q.OH && (q.nbx << q.bx_l2) >= q.OW, "%s: part_rows %d, tiling %d x %d x %d", where, q.part_rows, q.nbz, q.nby, q.nbx);
        if (q.kernel != CONV_MFMA) EXPECT(q.bz_l2 == 2 && q.by_l2 == 3 && q.bx_l2 == 3 && q.MT == 2, "%s: not on 4 x 8 x 8 bricks", where);
        EXPECT(q.kernel == CONV_F16S ? q.grid_x == (c.N * q.part_rows < 512 ? c.N * q.part_rows : 512) : q.grid_x == c.N * q.part_rows, "%s: grid %d", where, q.grid_x);
        break;
    case CONV_F16P: case CONV_F16P2: case CONV_F16Q2: case CONV_F16R: case CONV_F16P8: {
        EXPECT(q.part_rows == bricks && q.OD % (q.kernel == CONV_F16P8 ? 8 : 4) == 0 && q.OH % 8 == 0 && q.OW % 8 == 0, "%s: part_rows %d, bricks %d", where, q.part_rows, bricks);
        const int groups = q.kernel == CONV_F16P ? c.Cout / 32 : q.kernel == CONV_F16P2 || q.kernel == CONV_F16Q2 ? c.Cout / 64 : 1;
        EXPECT(q.work == c.N * bricks * groups / (q.kernel == CONV_F16P8 ? 2 : 1), "%s: %d work items", where, q.work);
        const bool capped = c.wgs_cap > 0 && c.wgs_cap < c.cus;
        const int wgs = persistent_wgs(c.wgs_cap, c.cus);
        EXPECT(q.grid_x == (q.work < wgs ? q.work : wgs) && wgs <= c.cus && (!capped || (wgs % 8 == 0 && wgs <= (c.wgs_cap > 8 ? c.wgs_cap : 8))), "%s: grid %d, work %d, wgs %d", where, q.grid_x, q.work, wgs);
        break;
    }
    case CONV_UP2C: {
        const int b = (c.ID / 2) * (c.IH / 8) * (c.IW / 8), TZ = (c.ID + 31) / 32, TY = (c.IH + 31) / 32, TX = (c.IW + 31) / 32, fg = 2 * c.ID * TY + 2 * c.ID * TX + 2 * c.IH * TX;
        EXPECT(q.part_rows == 8 * b + 4 * fg + 8 * (TZ + TY + TX) && q.up.slot0 == 8 * b + 4 * fg && q.up.face_grid >= 1 && q.up.edge_grid >= 1 && q.up.main_grid <= c.cus, "%s: part_rows %d slot0 %d", where, q.part_rows, q.up.slot0);
        break;
    }
    }
    if (q.st.x) EXPECT(q.grid_x == 256 || q.grid_x == 512, "%s: super tile on a grid of %d", where, q.grid_x);
}

static void sweep() {
    static const int EXT[][3] = {{1, 1, 1}, {2, 2, 2}, {3, 3, 3}, {4, 4, 4}, {5, 5, 5}, {6, 6, 6}, {8, 8, 8}, {12, 12, 12}, {16, 16, 16}, {20, 20, 20}, {24, 24, 24}, {32, 32, 32}, {40, 40, 40}, {48, 48, 48}, {64, 64, 64},
                                 {2, 8, 16}, {6, 24, 8}, {4, 40, 8}, {20, 32, 32}, {16, 8, 8}, {12, 8, 8}, {3, 5, 7}, {8, 12, 8}, {5, 8, 8}, {16, 9, 16}, {18, 16, 16}, {1, 8, 33}, {4, 8, 24}, {28, 16, 8}};
    static const int CH[][2] = {{8, 4}, {16, 16}, {32, 32}, {48, 48}, {64, 64}, {72, 72}, {96, 96}, {128, 128}, {136, 136}, {184, 179}, {256, 256}};        // padded, real
    static const int CO[] = {8, 24, 32, 48, 64, 72, 96, 128, 256, 1088};
    static const int KSP[][3] = {{1, 1, 0}, {2, 2, 0}, {3, 1, 1}, {3, 2, 1}, {5, 1, 2}, {3, 1, 0}};
    static const int CAPS[][2] = {{0, 256}, {3, 256}, {8, 256}, {100, 256}, {224, 256}, {255, 256}, {256, 256}, {300, 256}, {100, 304}, {0, 64}, {0, 80}};
    Switches sws[64]; int n_sw = 0;
    for (int mode = 0; mode < 4; ++mode) {
        const Switches d = {mode ? 1 : 0, mode == 2, mode == 3, 1, 1, 1, 1, 1, 1};
        sws[n_sw++] = d;
        if (!mode) continue;
        { Switches s = d; s.pool_q = 0; sws[n_sw++] = s; } { Switches s = d; s.f16r = 0; sws[n_sw++] = s; } { Switches s = d; s.up2y = 0; sws[n_sw++] = s; }
        for (int m : {0, 2}) { Switches s = d; s.up2y_march = m; sws[n_sw++] = s; }
        { Switches s = d; s.up2y_ypad = 0; sws[n_sw++] = s; }
        for (int sh : {0, 2, 3, 21, 42, 23}) { Switches s = d; s.up2c_shell = sh; sws[n_sw++] = s; }
    }
    for (int N : {1, 3, 16, 40})
        for (const auto& e : EXT) for (const auto& ch : CH) for (int Cout : CO) for (const auto& k : KSP) for (int up2 = 0; up2 < 2; ++up2) {
            if (up2 && k[1] != 1) continue;
            const int us = up2 ? 2 : 1;
            if (us * e[0] + 2 * k[2] < k[0] || us * e[1] + 2 * k[2] < k[0] || us * e[2] + 2 * k[2] < k[0]) continue;      // (no output voxel)
            for (int si = 0; si < 10; ++si) {
                // (the full cross product is 10^8 plans: every shape meets ten of the switch sets; they, the storages, the weight packs, the
                //  lazy / sparse inputs and the caps rotate)
                const int s = (N + e[0] * 7 + e[1] + ch[0] / 8 + Cout / 8 + k[0] + up2 + si * 4) % n_sw;
                const int rot = N + e[0] + e[1] * 3 + ch[0] + Cout + k[0] + s;
                const auto& cap = CAPS[rot % 11];
                for (int io = 0; io < 4; ++io) {
                    if (io && !sws[s].single && (rot + io) % 3) continue;    // (outside the one-product modes every bfloat16 call is refused: a third of them)
                    Call c = {N, e[0], e[1], e[2], ch[0], ch[1], Cout, (Cout + 31) & ~31, k[0], k[1], k[2], up2 != 0, ch[0] >= 16 && rot % 5 != 0, up2 && rot % 4 != 0,
                              (io & 1) != 0, (io & 2) != 0, false, false, false, cap[0], cap[1]};
                    check_plan(c, sws[s]);
                    if (k[0] == 2 && !io && rot % 2) {
                        c.has_in2 = true; check_plan(c, sws[s]); c.has_in2 = false;
                        c.has_map = true; check_plan(c, sws[s]); c.has_alt = true; check_plan(c, sws[s]); c.has_in2 = true; check_plan(c, sws[s]);
                    }
                }
            }
        }
    std::printf("sweep: %ld plans, %ld not refused\n", g_plans, g_taken);
}

// nm_net.hip's questions, against the full plan of the conv they are about
static void queries() {
    const Switches sws[] = {{0, false, false, 1, 1, 1, 1, 1, 1}, {1, false, false, 1, 1, 1, 1, 1, 1}, {1, true, false, 1, 1, 1, 1, 1, 1}, {1, false, true, 1, 1, 1, 1, 1, 1}, {1, false, true, 1, 0, 1, 1, 1, 1},
                            {1, false, false, 0, 1, 0, 1, 1, 1}, {1, false, true, 1, 1, 0, 1, 1, 1}};
    long n = 0, yes[3] = {0, 0, 0};
    for (const Switches& sw : sws) for (int D = 1; D <= 40; ++D) for (int H : {D, 8, 16, 12}) for (int W : {D, 8, 24}) for (int C : {8, 16, 24, 32, 48, 64, 96, 128, 192, 256}) for (int w16 = 0; w16 < 2; ++w16) {
        // first_layer / feature_net: the pool conv C -> C that consumes a brick-sparse or lazy tensor goes to the pool kernels
        const Call pc = {2, 2 * D, 2 * H, 2 * W, C, C, C, (C + 31) & ~31, 2, 2, 0, false, w16 != 0, false, false, false, false, false, false, 0, 256};
        const Plan pp = plan(pc, sw);
        const bool pq = pool_on_pool_kernels(sw, C, D, H, W, w16 != 0);
        EXPECT(pq == (pp.kernel == CONV_POOL_F16S || pp.kernel == CONV_POOL_F16Q), "pool query C=%d %dx%dx%d w16=%d mode %d,%d: %d, plan %s", C, D, H, W, w16, sw.conv_mode, sw.single, pq, KERNEL_NAMES[pp.kernel]);
        yes[0] += pq;
        for (int Cout : {32, 64}) for (int h = 0; h < 2; ++h) {
            // conv_gn: the plain k3 conv on the materialised upsampled tensor (both tensors of storage h) runs on conv_f16r
            const Call kc = {2, D, H, W, C, C, Cout, (Cout + 31) & ~31, 3, 1, 1, false, w16 != 0, false, h != 0, h != 0, false, false, false, 0, 256};
            const Plan kp = plan(kc, sw);
            const bool rq = k3_on_f16r(sw, C, Cout, 3, 1, 1, D, H, W, w16 != 0);
            EXPECT(rq == (kp.kernel == CONV_F16R) && (!rq || !kp.status), "f16r query C=%d Cout=%d %dx%dx%d w16=%d h=%d: %d, plan %s status %d", C, Cout, D, H, W, w16, h, rq, KERNEL_NAMES[kp.kernel], kp.status);
            yes[1] += rq;
            // set_weights: composite sets are composed exactly for the layers the plan sends to conv_up2c once they exist
            const Call uc = {2, D, H, W, C, C, Cout, (Cout + 31) & ~31, 3, 1, 1, true, w16 != 0, true, false, false, false, false, false, 0, 256};
            const bool uq = up2c_eligible(sw, D, H, W, C, Cout, 3, 1, 1);
            EXPECT((uq && sw.conv_mode == 1) == (plan(uc, sw).kernel == CONV_UP2C), "up2c query C=%d Cout=%d %dx%dx%d: %d, plan %s", C, Cout, D, H, W, uq, KERNEL_NAMES[plan(uc, sw).kernel]);
            yes[2] += uq;
            ++n;
        }
    }
    std::printf("queries: %ld shapes, true %ld / %ld / %ld times\n", n, yes[0], yes[1], yes[2]);
    EXPECT(yes[0] && yes[1] && yes[2], "a query that is never true checks nothing");
}

int main() {
    pinned_table();
    std::printf("pinned table: %zu rows\n", sizeof TABLE / sizeof TABLE[0]);
    sweep();
    queries();
    std::printf("%ld checks, %ld failed: %s\n", g_checks, g_bad, g_bad ? "FAILED" : "all plans hold");
    return g_bad ? 1 : 0;
}
