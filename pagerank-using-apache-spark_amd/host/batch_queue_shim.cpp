// Test shim (not product code): exposes csrc/pr_batch_queue.h -- the stop rule k_batch_decide_any
// applies on the device and the scheduler behind pr_batch_run_queue -- to
// tests/test_batch_queue_cpu.py on the CPU.
#include "pr_batch_queue.h"

extern "C" {

// The mask the next launch reads; saved / converged as the device would leave them (0, 0: no stop).
uint32_t prq_decide(uint32_t mask, const double *l1, double tol, int width, uint32_t *saved, uint32_t *converged) {
  pr::BatchQueueState qs{0, 0};
  const uint32_t next = pr::batch_any_decide(mask, l1, tol, width, &qs);
  *saved = qs.saved;
  *converged = qs.converged;
  return next;
}
int prq_block(void) { return pr::kAnyBlock; }
int prq_state_bytes(void) { return (int)sizeof(pr::BatchQueueState); }

// Drives QueueSched the way pr_batch_run_queue does, with a model in place of the device: query q
// converges in its need[q]-th iteration (need[q] > max_iterations: never).  Outputs: per query its
// column, iteration count and converged flag; the queries in completion order; per
// pr_batch_step_until_any call (mask, cap, executed) in calls[3 * i ..]; the sum of `executed`.
// Returns the number of calls, or -1 if they exceed max_calls.
int prq_simulate(int32_t n, const int32_t *need, int32_t width, int32_t max_iterations, int32_t *column,
                 int32_t *iterations, int32_t *converged, int32_t *order, int32_t *calls, int32_t max_calls,
                 int64_t *total) {
  pr::QueueSched s;
  s.init(n, width, max_iterations);
  int32_t cols[pr::kBatchMaxWidth], qs[pr::kBatchMaxWidth];
  pr::QueueDone done[pr::kBatchMaxWidth];
  int32_t n_calls = 0, n_done = 0;
  *total = 0;
  while (!s.finished()) {
    const int nf = s.refill(cols, qs);
    for (int i = 0; i < nf; ++i) column[qs[i]] = cols[i];
    const uint32_t mask = s.active();
    const int32_t cap = s.cap();
    int32_t executed = cap;
    for (int j = 0; j < width; ++j)
      if (s.query[j] >= 0 && need[s.query[j]] - s.age[j] < executed) executed = need[s.query[j]] - s.age[j];
    uint32_t conv = 0;
    for (int j = 0; j < width; ++j)
      if (s.query[j] >= 0 && s.age[j] + executed == need[s.query[j]]) conv |= 1u << j;
    if (n_calls >= max_calls) return -1;
    calls[3 * n_calls] = (int32_t)mask;
    calls[3 * n_calls + 1] = cap;
    calls[3 * n_calls + 2] = executed;
    ++n_calls;
    *total += executed;
    const int nd = s.advance(executed, conv, done);
    for (int i = 0; i < nd; ++i) {
      iterations[done[i].query] = done[i].iterations;
      converged[done[i].query] = done[i].converged;
      order[n_done++] = done[i].query;
    }
  }
  return n_calls;
}
}
