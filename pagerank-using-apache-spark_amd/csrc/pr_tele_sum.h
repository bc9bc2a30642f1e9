// ts, the sum of a handle's teleport vector (pr_set_teleport_dangling, pr_get_teleport_sum): the
// divisor of q = dc / ts in the engine's teleport dangling mode.  Shared by the library and the CPU
// test shim (host/tele_sum_shim.cpp, tests/test_teleport_dangling_cpu.py).  Plain C++ with PR_HD
// qualifiers, like pr_batch_dangling.h; the host builds are compiled with -ffp-contract=off.
//
// The sum runs over all V original IDs, not over a part's rows: pr_set_teleport* receives the whole
// vector on every part, so every part forms ts on the host from the call's own arguments, and ts is
// a function of those arguments and V only -- the same bits on every part, for every layout and for
// both forms of the setter.  The order:
//   blocks of kTeleSumBlock consecutive original IDs (the last one shorter);
//   within a block, a sequential sum in ID order starting from +0.0;
//   the block sums added sequentially in block order, starting from +0.0.
#pragma once

#include <stdint.h>

#include "pr_batch.h"  // PR_HD

namespace pr {

constexpr int64_t kTeleSumBlock = 1024;

// t[0..n) added in order to +0.0
PR_HD inline double tele_block_sum(const double *t, int64_t n) {
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i) acc = acc + t[i];
  return acc;
}

// `n` times `rest` added in order to +0.0 (a block without a seed)
PR_HD inline double tele_rest_sum(double rest, int64_t n) {
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i) acc = acc + rest;
  return acc;
}

// The dense form: t holds V doubles in original-ID order.
PR_HD inline double tele_sum_dense(const double *t, int64_t V) {
  double ts = 0.0;
  for (int64_t b0 = 0; b0 < V; b0 += kTeleSumBlock) {
    const int64_t n = V - b0 < kTeleSumBlock ? V - b0 : kTeleSumBlock;
    ts = ts + tele_block_sum(t + b0, n);
  }
  return ts;
}

// The sparse form: t[ids[i]] = values[i] for the n seeds, `rest` elsewhere; ids ascending, distinct
// and in [0, V).  The bits of tele_sum_dense over the equal dense vector in O(V / 1024 + 1024 *
// seeded blocks): a full block without a seed has the same sum every time (formed once), and only
// the blocks that hold seeds are walked.
PR_HD inline double tele_sum_sparse(int64_t V, int64_t n, const int32_t *ids, const double *values, double rest) {
  const double full = tele_rest_sum(rest, kTeleSumBlock);
  double ts = 0.0;
  int64_t k = 0;  // the next seed
  for (int64_t b0 = 0; b0 < V; b0 += kTeleSumBlock) {
    const int64_t len = V - b0 < kTeleSumBlock ? V - b0 : kTeleSumBlock;
    double bs;
    if (k < n && ids[k] < b0 + len) {  // a block that holds seeds: walked in ID order
      bs = 0.0;
      for (int64_t v = b0; v < b0 + len; ++v) {
        if (k < n && ids[k] == v) bs = bs + values[k++];
        else bs = bs + rest;
      }
    } else {
      bs = len == kTeleSumBlock ? full : tele_rest_sum(rest, len);
    }
    ts = ts + bs;
  }
  return ts;
}

}  // namespace pr
