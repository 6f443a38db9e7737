// Host check of conv_f16p8_kernel's barrier discipline: walks the MFMA waves' and the producer waves' control flow, as the kernel
// writes them, with the functions of nm_f16p8_plan.h that the kernel itself takes its barriers from, and requires the two sequences
// of workgroup barriers to be equal (kind by kind, not only in number) for C16 = 1 ... 4 chunks and 1 ... 3 bricks per workgroup.
// Plain C++, no GPU.  Prints one line per case; exit status 0 only if every case matches.
// What it does NOT prove: the two walks below are a transcription of the kernel's control flow, not the kernel's code.  They show that the
// plan is consistent with itself (both roles, following it, meet at the same barriers); a barrier written into the kernel that does
// not come from the plan, or a role that stops following it, is invisible here - that is kept true by reading the kernel, where
// every barrier sits beside the plan function that places it.
#include "nm_f16p8_plan.h"

#include <cstdio>
#include <vector>

namespace pl = nm_f16p8;

enum Kind { PROLOGUE = 100, BRICK_END = 200 };      // group ends are recorded as the group's number 0 ... 3

// producer waves: prologue, then per step one stage (and one barrier) per tap group, the brick-end barrier, two steps of look-ahead
static std::vector<int> walk_producers(int C16, int items) {
    std::vector<int> b;
    pl::Cursor cur{0, 0};
    pl::Cursor s1 = cur; bool has1 = pl::next_step(s1, items, C16);
    pl::Cursor s2 = s1;  bool has2 = has1 && pl::next_step(s2, items, C16);
    b.push_back(PROLOGUE);
    for (;;) {
        for (int g = 0; g < pl::kGroups; ++g) b.push_back(g);
        if (pl::brick_end(cur.cb, C16)) b.push_back(BRICK_END);
        if (!has1) break;
        cur = s1; s1 = s2; has1 = has2; has2 = has2 && pl::next_step(s2, items, C16);
    }
    return b;
}

// MFMA waves: prologue, then per step the 27 taps with a barrier wherever a tap ends its group, the brick-end barrier in the epilogue
static std::vector<int> walk_mfma(int C16, int items) {
    std::vector<int> b;
    pl::Cursor cur{0, 0};
    b.push_back(PROLOGUE);
    for (;;) {
        pl::Cursor nxt = cur;
        const bool has_next = pl::next_step(nxt, items, C16);
        for (int tt = 0; tt < pl::kTaps; ++tt)
            if (pl::group_end(tt)) b.push_back(pl::group_of(tt));
        if (pl::brick_end(cur.cb, C16)) b.push_back(BRICK_END);
        if (!has_next) break;
        cur = nxt;
    }
    return b;
}

int main() {
    int bad = 0;
    for (int C16 = 1; C16 <= 4; ++C16)
        for (int items = 1; items <= 3; ++items) {
            const std::vector<int> a = walk_producers(C16, items), m = walk_mfma(C16, items);
            const size_t want = 1 + (size_t)items * C16 * pl::kGroups + items;
            const bool ok = a == m && a.size() == want;
            std::printf("C16=%d bricks=%d producers=%zu mfma=%zu expected=%zu %s\n", C16, items, a.size(), m.size(), want, ok ? "ok" : "MISMATCH");
            bad += ok ? 0 : 1;
        }
    // every tap belongs to exactly one group, in order, and no group is longer than a weight buffer
    int taps = 0;
    for (int g = 0; g < pl::kGroups; ++g) {
        if (pl::group_taps(g) < 1 || pl::group_taps(g) > pl::kGroupTaps || pl::group_first(g) != taps) ++bad;
        for (int t = 0; t < pl::group_taps(g); ++t)
            if (pl::group_of(taps + t) != g || pl::tap_in_group(taps + t) != t) ++bad;
        taps += pl::group_taps(g);
    }
    if (taps != pl::kTaps) ++bad;
    std::printf("%s\n", bad ? "FAILED" : "all barrier sequences match");
    return bad ? 1 : 0;
}
