// Test shim (not product code): exposes the block-order sum of a handle's teleport vector
// (csrc/pr_tele_sum.h) -- ts of pr_set_teleport_dangling's mode, which pr_set_teleport and
// pr_set_teleport_sparse form on the host -- to tests/test_teleport_dangling_cpu.py.  Built with
// -ffp-contract=off, like the library.
#include "pr_tele_sum.h"

extern "C" {

long long prts_block(void) { return (long long)pr::kTeleSumBlock; }
double prts_dense(const double *t, long long V) { return pr::tele_sum_dense(t, (int64_t)V); }
// ids ascending and distinct, as the library passes them
double prts_sparse(long long V, long long n, const int32_t *ids, const double *values, double rest) {
  return pr::tele_sum_sparse((int64_t)V, (int64_t)n, ids, values, rest);
}
}
