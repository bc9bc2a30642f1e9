// pr_batch_step_until_any and pr_batch_run_queue (pr_batch.hip): the stop rule of a call that ends
// at the first convergence, the two words of device state it adds to BatchUntilState, and the host
// scheduler that keeps a fixed number of columns filled from a queue of queries.  Shared by the
// library and the CPU test shim (host/batch_queue_shim.cpp, tests/test_batch_queue_cpu.py).  Plain
// C++ with PR_HD qualifiers, like pr_batch_until.h; no HIP in it.
//
// The stop.  Iterations are enqueued in blocks on an in-order stream, so the device ends the rest
// of a block itself: after the first iteration in which an active column converged, the one-thread
// decide kernel parks the mask the iteration ran under in BatchQueueState::saved, records the
// columns that converged, and stores 0 in BatchUntilState::mask.  The *_until kernels of the
// remaining launches then return at entry, as they do once pr_batch_step_until has frozen every
// column.  The host reads both structs back once per block.
//
// The scheduler.  QueueSched holds, per column, the query it serves and that query's age (the
// iterations it has had); every pr_batch_step_until_any call runs all occupied columns with the
// smallest remaining allowance as its cap, so that no query ever gets more than max_iterations.  A
// query leaves its column when it converged or when its age reached max_iterations; the column takes
// the next query of the queue before the next call.  Slot assignment, caps and the order of the
// completions are therefore a function of the queries' iteration counts, the width and
// max_iterations alone.
#pragma once

#include <stdint.h>

#include "pr_batch_until.h"

namespace pr {

// Iterations enqueued between two read-backs by pr_batch_step_until_any.  A call ends at the first
// convergence, so part of its last block is launched empty.  Measured with 1, 4, 8, 16 and 32
// (profiles/batch_queue/): all within 1.3 % of each other, 1 the slowest, no order among the rest
// that holds from run to run: an empty launch costs about what the read-back it saves does.  8 is a
// middle value, not a measured optimum.
constexpr int kAnyBlock = 8;

// Read back with BatchUntilState after every block.
struct BatchQueueState {
  uint32_t saved;      // the mask the stopping iteration ran under (0: the call has not stopped)
  uint32_t converged;  // the columns of `saved` whose L1 was within tol in that iteration
};
static_assert(sizeof(BatchQueueState) == 8, "BatchQueueState is read back as plain words");

// After an iteration that ran under `mask` and left l1[0..width): the columns of `mask` that
// converged (l1[j] <= tol: batch_until_decide's test, so a NaN never passes, tol == 0 needs an exact
// 0, bits outside `mask` and bits >= width never appear).
PR_HD inline uint32_t batch_any_converged(uint32_t mask, const double *l1, double tol, int width) {
  const uint32_t in = mask & batch_until_all(width < kBatchMaxWidth ? width : kBatchMaxWidth);
  return in & ~batch_until_decide(mask, l1, tol, width);
}

// The mask the next launch reads: unchanged while nothing converged, 0 (stop) otherwise.  *qs is
// written only on a stop.
PR_HD inline uint32_t batch_any_decide(uint32_t mask, const double *l1, double tol, int width, BatchQueueState *qs) {
  const uint32_t conv = batch_any_converged(mask, l1, tol, width);
  if (conv == 0) return mask;
  qs->saved = mask;
  qs->converged = conv;
  return 0;
}

// ---- the scheduler -----------------------------------------------------------------------------
struct QueueDone {
  int32_t query, column, iterations, converged;
};

struct QueueSched {
  int32_t n_queries = 0, width = 0, max_iterations = 0;
  int32_t next = 0;      // the next query of the queue
  int32_t reported = 0;  // queries that have left their column
  int32_t query[kBatchMaxWidth];  // per column: the query it serves, -1: free
  int32_t age[kBatchMaxWidth];    // per column: iterations its query has had

  void init(int32_t n, int32_t w, int32_t max_it) {
    n_queries = n;
    width = w;
    max_iterations = max_it;
    next = reported = 0;
    for (int j = 0; j < kBatchMaxWidth; ++j) {
      query[j] = -1;
      age[j] = 0;
    }
  }
  bool finished() const { return reported >= n_queries; }
  // Free columns take the next queries, in ascending column order.  cols / queries (width entries
  // at most) list what has to be started; returns how many.
  int refill(int32_t *cols, int32_t *queries) {
    int n = 0;
    for (int j = 0; j < width && next < n_queries; ++j)
      if (query[j] < 0) {
        query[j] = next++;
        age[j] = 0;
        cols[n] = j;
        queries[n] = query[j];
        ++n;
      }
    return n;
  }
  // The occupied columns, and the cap of the next call: the smallest remaining allowance.
  uint32_t active() const {
    uint32_t m = 0;
    for (int j = 0; j < width; ++j)
      if (query[j] >= 0) m |= 1u << j;
    return m;
  }
  int32_t cap() const {
    int32_t c = max_iterations;
    for (int j = 0; j < width; ++j)
      if (query[j] >= 0 && max_iterations - age[j] < c) c = max_iterations - age[j];
    return c;
  }
  // A call applied `executed` iterations to every occupied column and reported `converged`.  The
  // queries that leave (converged, or at their allowance), in ascending column order; their columns
  // are free afterwards.  Returns how many.
  int advance(int32_t executed, uint32_t converged, QueueDone *done) {
    int n = 0;
    for (int j = 0; j < width; ++j) {
      if (query[j] < 0) continue;
      age[j] += executed;
      const bool conv = (converged >> j) & 1u;
      if (conv || age[j] >= max_iterations) {
        done[n++] = QueueDone{query[j], j, age[j], conv ? 1 : 0};
        query[j] = -1;
        ++reported;
      }
    }
    return n;
  }
};

}  // namespace pr
