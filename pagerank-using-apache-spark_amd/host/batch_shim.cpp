// Test shim (not product code): exposes the batch planner of csrc/pr_batch.h -- the layout stride,
// the unit capacity and the plan of work units over a row_ptr array -- to tests/test_batch_cpu.py
// on the CPU.  The plan is the library's own (batch_plan), flattened into plain arrays.
#include "pr_batch.h"

#include <cstddef>

extern "C" {

int prb_stride(int width) { return pr::batch_stride(width); }
int prb_unit_cap(int stride) { return pr::batch_unit_cap(stride); }
int prb_unit_rows(void) { return pr::kBatchUnitRows; }

// Plans rows [0, V) of row_ptr for `stride`.  Returns the number of units; when it is at most
// max_units, unit u is written as (e0[u], row0[u], rows[u], n[u], slot[u]) with the fields of
// pr::BatchUnit.  *n_long = rows cut into chunks, *n_slots = chunk partial slots in all.
int64_t prb_plan(const int64_t *row_ptr, int64_t V, int stride, int64_t max_units, int64_t *e0, int32_t *row0,
                 int32_t *rows, int32_t *n, int32_t *slot, int64_t *n_long, int64_t *n_slots) {
  pr::BatchPlan plan;
  pr::batch_plan(row_ptr, V, stride, &plan);
  const int64_t nu = (int64_t)plan.units.size();
  if (n_long) *n_long = (int64_t)plan.long_row.size();
  if (n_slots) *n_slots = plan.long_p0.back();
  if (nu <= max_units)
    for (int64_t u = 0; u < nu; ++u) {
      const pr::BatchUnit &b = plan.units[(std::size_t)u];
      e0[u] = b.e0;
      row0[u] = b.row0;
      rows[u] = b.rows;
      n[u] = b.n;
      slot[u] = b.slot;
    }
  return nu;
}
}
