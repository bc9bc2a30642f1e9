// Layout policy of the build: the decisions that fix a graph's shape for its whole life -- fused
// or split layout, class count, row geometry, entry code, hot-set size -- as pure functions of a
// few numbers, shared by the build's stages (pr_build.hip) and the CPU test shim
// (host/layout_shim.cpp, tests/test_layout_policy_cpu.py).  Plain C++ with PR_HD qualifiers, so a
// host compiler builds it without the HIP runtime.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "pagerank_hip.h"
#include "pr_pieces.h"

namespace pr {

// ---- layouts (pr_graph.h) -----------------------------------------------------------------------
constexpr int kLayoutFused = 0;  // one class, k_spmv_units (gather space <= 4 MiB)
constexpr int kLayoutSplit = 1;  // column classes, LDS hot sets, partial slots (k_spmv_hot + k_epilogue_grp)
constexpr int kXcds = 8;             // XCDs of the MI355X (one L2 each)
constexpr int kMaxClasses = 128;     // 8, 16, 32, 64 or 128 (PR_BOPT_CLASSES)
constexpr int kAutoMaxClasses = 64;  // the most the size policy picks by itself
static_assert(kMaxClasses == 16 * kXcds, "class counts");
// split once the gather space passes 4 MiB: R-MAT s20 (5.2 MB, L2-resident either way) runs the
// split layout at 8 classes in 0.09 ms/iter against 0.18 ms fused (profiles/r01/configs_ab/s20_*)
constexpr int64_t kSplitMinSliceBytes = 4ll << 20;

// Column classes of the split layout: the fewest (8, 16, 32, 64) whose class region of the part's
// gather space (its slice plus the expected received runs at P > 1) fits one XCD's 4 MiB L2 (the
// phased schedule runs one class per XCD at a time), capped at kAutoMaxClasses; PR_BOPT_CLASSES
// (opt_classes != 0) overrides.  More classes keep more gathers in L2 and the LDS hot sets but cost
// epilogue work per (row, class): R-MAT s26 (262 MB) -> 64 at P = 1, 2, 4 and 32 for an 8-way part
// (121 MB: 8 % less per iteration than 64); the Twitter shape stays at 64 at P = 8 (6 % better than
// 32); ER s24 (134 MB) -> 64, LiveJournal (39 MB) -> 16 (profiles/r02/class_policy/).
constexpr int64_t kClassRegionBytes = 4000000;  // just under the 4 MiB L2: ER s24 (4.19 MB at 32) stays at 64
inline int class_setting(int opt_classes, int64_t gather_bytes) {
  if (opt_classes) return opt_classes;
  for (int c = kXcds; c < kAutoMaxClasses; c *= 2)
    if (gather_bytes <= (int64_t)c * kClassRegionBytes) return c;
  return kAutoMaxClasses;
}

// Layout and row geometry of a part: the fused layout while the gather space of all P parts
// (n_local_max rows each) fits the L2s, the split layout beyond (profiles/r03/rows_layout/: a
// row-block layout with LDS row sums and no partial slots ran 2x slower at ER s24 and far slower on
// skewed graphs, and was removed); PR_LAYOUT_* flags override.  Split-layout entry codes are byte
// offsets below 2^31 (pr_internal.h), so a larger gather space stays fused whatever the flags say.
// Local rank j -> class j % C, row (j % C) * Q_pad + j / C; rows come in whole 64-row blocks
// (k_epilogue_grp), and a slice is its rows plus the two slots, padded to 64.
struct LayoutGeom {
  int layout, C;
  int64_t Q_pad, n_rows, S_pad;
  bool fits;  // false: the gather space exceeds 2^31 entries (the build fails)
};
inline LayoutGeom choose_layout(uint32_t flags, int opt_classes, int P, int64_t n_local_max, int64_t gather_est) {
  LayoutGeom l{};
  l.layout = (int64_t)P * n_local_max * 8 > kSplitMinSliceBytes ? kLayoutSplit : kLayoutFused;
  if (flags & PR_LAYOUT_FUSED) l.layout = kLayoutFused;
  if (flags & PR_LAYOUT_SPLIT) l.layout = kLayoutSplit;
  if ((int64_t)P * (n_local_max + 64 + kMaxClasses) * 8 >= (1ll << 31) - (1ll << 20)) l.layout = kLayoutFused;
  l.C = l.layout == kLayoutSplit ? class_setting(opt_classes, gather_est) : 1;
  l.Q_pad = ((n_local_max + l.C - 1) / l.C + 63) / 64 * 64;
  l.n_rows = (int64_t)l.C * l.Q_pad;
  l.S_pad = (l.n_rows + 2 + 63) / 64 * 64;
  l.fits = (int64_t)P * l.S_pad < (int64_t(1) << 31);
  return l;
}

// ---- LDS of k_spmv_hot ----------------------------------------------------------------------
// The hot set (slot 0 = 0.0, then the hot contributions of every part), one more 0.0 slot (where
// compact cold entries point their LDS read), the workgroup's unit counter, then one staging
// window of kStageSlots segment sums per wave (16 KiB in all; 128 beat 256 by ~0.5 % and 64 by
// ~0.8 % at R-MAT s26, profiles/r01/stage_ab/).
constexpr int kHotThreads = 1024;  // 16 waves per CU: one workgroup per CU
#ifndef PR_STAGE_SLOTS  // A/B builds only (tools/ab_build.sh): the library reads no environment
#define PR_STAGE_SLOTS 128
#endif
constexpr int kStageSlots = PR_STAGE_SLOTS;
constexpr int kHotLdsBytes = 160 * 1024;
constexpr int kHotSlotsMax = (kHotLdsBytes - (kHotThreads / 64) * kStageSlots * 8) / 8 - 3;
constexpr int kHotSlotsDefault = kHotSlotsMax;  // 18429 hot contributions (144 KiB)
inline int hot_slots_setting(int opt_hot_slots) {  // PR_BOPT_HOT_SLOTS, < 0: the default
  return std::max(0, std::min(opt_hot_slots < 0 ? kHotSlotsDefault : opt_hot_slots, kHotSlotsMax));
}

// A class's hot set: for every part p, rows [x*Q_pad, + q_load) of p's slice go to LDS slots
// 1 + [p*Kp, p*Kp + q_load); slot 0 holds 0.0.  Their gather positions come from a table (the
// part's gather space is compacted when only some remote positions are received).
struct HotGeom {
  int C, P, Kp, q_load;
  int64_t S_pad, Q_pad;
  int tbl;  // 1: piece codes, the class's piece table follows the staging windows (kPieceTblSlots)
  PR_HD int slots() const { return P * Kp + 1; }
  // slot `slots()` holds 0.0 (compact codes' cold entries read it), slot `slots() + 1` is a
  // control word (the workgroup's unit counter, pr_spmv.h hot_class_units); the staging windows
  // start 16-byte aligned after it
  PR_HD int ctr_slot() const { return slots() + 1; }
  PR_HD int stage_off() const { return (slots() + 3) & ~1; }
  PR_HD int tbl_off() const { return stage_off() + (kHotThreads / 64) * kStageSlots; }
  PR_HD size_t lds_bytes() const {
    return sizeof(double) * ((size_t)tbl_off() + (tbl ? (size_t)kPieceTblSlots : 0));
  }
};

// ---- entry codes (formats: pr_internal.h) ------------------------------------------------------
constexpr int kCodeU32 = 0;
constexpr int kCodeC20 = 1;
constexpr int kCodeC24 = 2;
constexpr int kCodeC20P = 3;
constexpr int kCodeC24P = 4;
constexpr PR_HD bool code_is_piece(int code) { return code >= kCodeC20P; }
constexpr int kMaxPackParts = 8;  // the most parts of a fused pack (pr_internal.h PackDst)

// One part: compact codes when every region index fits (a class's sources are its region of the
// one slice, whole_slice: gsize == S_pad) -- 2.5 bytes per entry below 2^19 region rows, 3 below
// 2^20 -- else 32-bit codes; opt_codes == 0 (PR_BOPT_CODES) asks for those.
inline int code_one_part(int opt_codes, int P, bool whole_slice, int64_t Q_pad) {
  const bool compact = opt_codes != 0 && P == 1 && whole_slice;
  return compact && Q_pad < (int64_t(1) << kC20IdxBits)   ? kCodeC20
         : compact && Q_pad < (int64_t(1) << kC24IdxBits) ? kCodeC24
                                                           : kCodeU32;
}
// A part of a row partition may take the piece codes (the build then plans its pieces: vmax).
inline bool piece_codes_allowed(int opt_codes, int P) { return opt_codes != 0 && P > 1 && P <= kMaxPackParts; }
// ... and takes them when its classes' virtual spaces fit: the hot set shrinks from `slots` to the
// largest that leaves LDS room for the piece table, and the largest index + 1 is its P * Kp slots
// plus vmax.  Else 32-bit codes and the caller's slots.
struct CodeChoice { int code, slots; };
inline CodeChoice code_of_parts(int slots, int P, int64_t vmax) {
  HotGeom t{0, P, 0, 0, 0, 0, 1};  // P parts, with a piece table
  int ps = slots;
  for (;; --ps) {
    t.Kp = ps / P;
    if (t.lds_bytes() <= (size_t)kHotLdsBytes) break;
  }
  const int64_t top = (int64_t)P * (ps / P) + vmax;
  if (top < (int64_t(1) << kC20IdxBits)) return {kCodeC20P, ps};
  if (top < (int64_t(1) << kC24IdxBits)) return {kCodeC24P, ps};
  return {kCodeU32, slots};
}

}  // namespace pr
