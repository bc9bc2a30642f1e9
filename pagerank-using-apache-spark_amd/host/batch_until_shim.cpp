// Test shim (not product code): exposes the convergence decision of csrc/pr_batch_until.h -- the
// function k_batch_decide applies on the device after every iteration of pr_batch_step_until -- to
// tests/test_batch_until_cpu.py on the CPU.
#include "pr_batch_until.h"

extern "C" {

uint32_t pru_decide(uint32_t mask, const double *l1, double tol, int width) {
  return pr::batch_until_decide(mask, l1, tol, width);
}
uint32_t pru_all(int width) { return pr::batch_until_all(width); }
int pru_block(void) { return pr::kUntilBlock; }
int pru_state_bytes(void) { return (int)sizeof(pr::BatchUntilState); }
}
