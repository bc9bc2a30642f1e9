// Test shim (not product code): exposes the per-column rule and the term of the batch's teleport
// dangling mode (csrc/pr_batch_dangling.h) -- the functions k_batch_units_td / k_batch_long_td apply on
// the device -- to tests/test_batch_dangling_cpu.py on the CPU.  Built with -ffp-contract=off, so the
// host rounds every operation on its own, as the device does.
#include "pr_batch_dangling.h"

extern "C" {

int prd_uses_teleport(double ts) { return pr::batch_dangling_uses_teleport(ts) ? 1 : 0; }
double prd_term(double q, double t) { return pr::batch_dangling_term(q, t); }
double prd_factor(int use, double dc, double ts, double n_vertices) {
  return pr::batch_dangling_factor(use != 0, dc, ts, n_vertices);
}
void prd_terms(int n, const double *q, const double *t, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pr::batch_dangling_term(q[i], t[i]);
}
}
