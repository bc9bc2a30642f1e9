// Batch top-K (pr_batch_topk.hip): the per-column state of the lockstep select and its host driver,
// shared by the library and the CPU test shim (host/batch_topk_shim.cpp,
// tests/test_batch_topk_cpu.py).  Plain C++ with PR_HD qualifiers, so a host compiler builds it
// without the HIP runtime.
//
// Every column of a batch runs the MSD radix select of pr_topk.h -- same 96-bit composite keys
// (rank key, ~original ID), same 8-bit digits -- over its own column of the interleaved V x stride
// rank matrix, and all columns advance together: pass p builds one histogram of digit p per active
// column in a single sweep, and btopk_advance moves every active column by that digit.  A column
// is done as soon as a bin's count equals what it still misses (or after the last digit); its
// prefix with zero low digits is then its threshold, exactly topk_select_threshold's.  A vertex
// whose bit j is set in the exclusion mask does not take part in column j.
#pragma once

#include <stdint.h>

#include "pr_topk.h"

namespace pr {

constexpr int kBTopkMaxCols = 16;  // = kBatchMaxWidth

// One column of the lockstep select.  `need` keys are still to be found among the `cand`
// candidates, the keys that agree with (phi, plo) on the digits chosen so far.
struct BTopkCol {
  uint64_t phi = 0;
  uint32_t plo = 0;
  uint64_t need = 0;
  uint64_t cand = 0;
  bool done = true;  // done from the start: nothing to select, or everything available is
};

// Column c is to select k of n_avail keys.  0 < k < n_avail starts the select; otherwise the
// column is done with threshold 0 (k == n_avail: every available key is >= it).
PR_HD inline void btopk_begin(BTopkCol *c, uint64_t k, uint64_t n_avail) {
  c->phi = 0;
  c->plo = 0;
  c->need = k;
  c->cand = n_avail;
  c->done = !(k > 0 && k < n_avail);
}

// Advances an active column by digit p, whose histogram over the column's candidates is hist.
// The same steps as one round of topk_select_threshold.
PR_HD inline void btopk_advance(BTopkCol *c, int p, const uint32_t *hist) {
  uint64_t above = 0;
  const int b = topk_choose_bin(hist, c->need, &above);
  c->need -= above;
  topk_extend(&c->phi, &c->plo, p, (uint32_t)b);
  c->cand = hist[b];
  if (c->cand == c->need || p + 1 >= kTopkDigits) c->done = true;
}

// Host driver of the lockstep select.  cols[0..width) come from btopk_begin.
// `hist_pass(p, cols, hist)` fills hist[j * kTopkBins + d] for every active (not done) column j with
// the digit-p counts of its candidates and returns 0, or an error code that ends the select.
// `narrow(p, cols, total)` is called at most once, after the first pass that leaves the active
// columns with at most narrow_limit candidates together (narrow_limit < 0: never): p digits are
// known, total is that sum; later hist_pass calls may read what it compacted.  On return every
// column's (phi, plo) is its threshold.  *passes = histogram passes run, *narrowed_at = the digits
// known when narrow ran, or -1.
template <class HistPass, class Narrow>
inline int btopk_select_thresholds(int width, BTopkCol *cols, int64_t narrow_limit, HistPass hist_pass, Narrow narrow,
                                   int *passes, int *narrowed_at) {
  *passes = 0;
  *narrowed_at = -1;
  std::vector<uint32_t> hist((size_t)kBTopkMaxCols * kTopkBins);
  for (int p = 0; p < kTopkDigits; ++p) {
    bool any = false;
    for (int j = 0; j < width; ++j) any = any || !cols[j].done;
    if (!any) break;
    const int rc = hist_pass(p, (const BTopkCol *)cols, hist.data());
    if (rc != 0) return rc;
    ++*passes;
    uint64_t total = 0;
    any = false;
    for (int j = 0; j < width; ++j) {
      if (cols[j].done) continue;
      btopk_advance(&cols[j], p, hist.data() + (size_t)j * kTopkBins);
      if (!cols[j].done) {
        any = true;
        total += cols[j].cand;
      }
    }
    if (any && *narrowed_at < 0 && narrow_limit >= 0 && p + 1 < kTopkDigits && total <= (uint64_t)narrow_limit) {
      const int rc2 = narrow(p + 1, (const BTopkCol *)cols, total);
      if (rc2 != 0) return rc2;
      *narrowed_at = p + 1;
    }
  }
  return 0;
}

// Candidates at which the lockstep select narrows: V * width / narrow_div (narrow_div 0: never).
inline int64_t btopk_narrow_limit(int64_t V, int width, int64_t narrow_div) {
  return narrow_div > 0 ? V * (int64_t)width / narrow_div : -1;
}

}  // namespace pr
