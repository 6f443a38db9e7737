// conv_f16p8_kernel: the one description of a step that BOTH roles of the workgroup (MFMA waves, producer waves) take their
// workgroup barriers from.  A mismatch between the two barrier sequences hangs a CU, so neither role writes a barrier of its
// own: the MFMA waves place one wherever group_end(tap) holds, the producers run one stage per tap group, both add the
// brick-end barrier where brick_end(cb, C16) holds, and both walk steps with next_step().  Plain C++ (no HIP): the host check
// tests/cpp/f16p8_barrier_walk.cpp walks both roles with these same functions and compares the sequences.
#pragma once

#include "nm_brick_walk.h"

namespace nm_f16p8 {

constexpr int kTaps = 27;          // 3 x 3 x 3, walked 0 ... 26 in every step
constexpr int kGroupTaps = 7;      // taps per weight buffer: two 7-tap buffers fit beside the 10 x 10 x 10 halo tiles
constexpr int kGroups = 4;         // tap groups of a step: 7 / 7 / 7 / 6; group g lives in weight buffer g & 1
constexpr int kPieces = 16;        // 16-byte input pieces per producer thread and step (4 000 / 256, tail masked)

// LDS layout, in this order (the kernel's pointers and the launcher's byte count both come from here)
constexpr int kHaloVoxels = 1000;                                // 10 x 10 x 10 halo tile of an 8 x 8 x 8 brick
constexpr int kHaloSlots = 2 * 4 * kHaloVoxels;                  // 16-byte slots: [2 buffers][hi h0 | hi h1 | lo h0 | lo h1][voxel]
constexpr int kWeightBufSlots = kGroupTaps * 4 * 32;             // 16-byte slots of one weight buffer: [tap][4 planes][32 channels]
constexpr int kWeightSlots = 2 * kWeightBufSlots;
constexpr int kRedFloats = 2 * 4 * 32 * 2;                       // GroupNorm scratch [2 z halves][4 waves][32 channels][sum, sum of squares]
constexpr int kBiasFloats = 32;
constexpr unsigned long kLdsBytes = (unsigned long)(kHaloSlots + kWeightSlots) * 16 + (unsigned long)(kRedFloats + kBiasFloats) * 4;
static_assert(kLdsBytes == 158848 && kLdsBytes <= 160 * 1024, "LDS budget of gfx950: 163 840 B per workgroup");

NM_PLAN_FN int group_first(int g) { return g * kGroupTaps < kTaps ? g * kGroupTaps : kTaps; }
NM_PLAN_FN int group_taps(int g) { return group_first(g + 1) - group_first(g); }
NM_PLAN_FN int group_of(int tap) { return tap / kGroupTaps; }
NM_PLAN_FN int tap_in_group(int tap) { return tap % kGroupTaps; }
// a workgroup barrier follows this tap (the producers publish the next group's weights; after the last group, the next tile)
NM_PLAN_FN bool group_end(int tap) { return tap + 1 == group_first(group_of(tap) + 1); }
// the producers' pieces of the NEXT step's tile converted during tap group g: [piece_first(g), piece_first(g + 1))
NM_PLAN_FN int piece_first(int g) { return g == 0 ? 0 : g == 1 ? 4 : g == 2 ? 9 : g == 3 ? 14 : kPieces; }
// the step of chunk cb finishes a brick: the MFMA waves' exposed epilogue holds one more workgroup barrier
NM_PLAN_FN bool brick_end(int cb, int C16) { return cb == C16 - 1; }

static_assert(group_first(kGroups) == kTaps && group_taps(3) == 6 && group_taps(0) == 7, "7 / 7 / 7 / 6");
static_assert(kGroups % 2 == 0, "group g in buffer g & 1 needs an even number of groups per step");
static_assert(group_end(6) && group_end(13) && group_end(20) && group_end(26) && !group_end(0) && !group_end(25), "group ends");
static_assert(piece_first(kGroups) == kPieces, "every piece is dealt to a group");

// position of a role in its workgroup's run of bricks, and the step to the next one: the walk's (nm_brick_walk.h), which the kernel
// reaches through nm_walk::Walk::advance
using nm_walk::Cursor;
using nm_walk::next_step;

}  // namespace nm_f16p8
