// pr_batch_step_until (pr_batch.hip): the per-column convergence decision and the few words of
// device state it works on, shared by the library and the CPU test shim (host/batch_until_shim.cpp,
// tests/test_batch_until_cpu.py).  Plain C++ with PR_HD qualifiers, like pr_batch.h.
//
// Bit j of the active mask says "column j still iterates in this call".  After every iteration one
// thread applies batch_until_decide to the mask the iteration ran under and to the L1 deltas it
// produced; the next iteration's kernels read the result.  A column whose bit is clear keeps its
// ranks, contributions, next-iteration dangling sum and L1 exactly as its last applied iteration
// left them.
#pragma once

#include <stdint.h>

#include "pr_batch.h"

namespace pr {

// Iterations enqueued between two read-backs of BatchUntilState.  Measured with 1, 4, 8, 16 and 32
// (profiles/batch_until/): the fewer read-backs the faster, by less than 1 % from 8 on; the
// iterations of a block past the last active column cost a few empty launches each.
constexpr int kUntilBlock = 32;

// What the host reads back after every block of iterations, in one copy.
struct BatchUntilState {
  uint32_t mask;                  // columns still active
  int32_t executed;               // iterations that ran with a non-empty mask
  int32_t iters[kBatchMaxWidth];  // per column: iterations applied in this call
};
static_assert(sizeof(BatchUntilState) == 8 + 4 * kBatchMaxWidth, "BatchUntilState is read back as plain words");

// The mask after an iteration that ran under `mask` and left the L1 deltas l1[0..width): column j
// leaves the mask when l1[j] <= tol.  The test is absolute.  A NaN never satisfies it, so a column
// whose L1 is NaN never converges; tol == 0 needs an L1 of exactly 0; a bit that is clear in `mask`
// stays clear whatever l1[j] holds, and bits >= width are never set.
PR_HD inline uint32_t batch_until_decide(uint32_t mask, const double *l1, double tol, int width) {
  uint32_t out = 0;
  for (int j = 0; j < width && j < kBatchMaxWidth; ++j)
    if (((mask >> j) & 1u) && !(l1[j] <= tol)) out |= 1u << j;
  return out;
}

// The mask a call starts with: every one of the `width` columns.
PR_HD inline uint32_t batch_until_all(int width) {
  return width >= 32 ? 0xffffffffu : (1u << width) - 1u;
}

}  // namespace pr
