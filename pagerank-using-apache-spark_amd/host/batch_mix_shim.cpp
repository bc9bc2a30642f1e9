// Test shim (not product code): exposes the blend of the batch mixes (csrc/pr_batch_mix.h) -- the
// expression k_batch_mix applies on the device -- to tests/test_batch_mix_cpu.py on the CPU.  Built
// with -ffp-contract=off, so the host rounds every operation on its own, as the device does.
#include "pr_batch_mix.h"

extern "C" {

int prm_stride(int n_mixes) { return pr::batch_mix_stride(n_mixes); }
double prm_elem(const double *w, const double *x, int width) { return pr::batch_mix_elem(w, x, width); }
// out[v] = the blend of row v of x (n_vertices x width, row-major) under w
void prm_blend(int n_vertices, int width, const double *w, const double *x, double *out) {
  for (int v = 0; v < n_vertices; ++v) out[v] = pr::batch_mix_elem(w, x + (long)v * width, width);
}
}
