// The batch's dangling modes (pr_batch_set_dangling, pr_batch.hip): which columns return their
// dangling mass along the teleport vector, and the term they add, shared by the kernels and the CPU
// test shim (host/batch_dangling_shim.cpp, tests/test_batch_dangling_cpu.py).  Plain C++ with PR_HD
// qualifiers, like pr_batch.h.
//
// In teleport mode column j's iteration is r'[v] = t[v] + damping * (S[v] + q_j * t[v]) with
// q_j = dc_j / ts_j and ts_j = the sum of the column's teleport vector, every operation rounded on
// its own.  A column whose ts_j is exactly 0 (no vector, padding, or a vector that sums to 0) or not
// finite keeps the uniform dc_j / N: the choice is made once per lane at kernel entry, as a select.
#pragma once

#include "pr_batch.h"

namespace pr {

// Whether a column whose teleport vector sums to `ts` uses the teleport term: ts finite and != 0
// (+-0, +-inf and NaN select the uniform term; a negative or subnormal sum is allowed).
PR_HD inline bool batch_dangling_uses_teleport(double ts) {
  return ts != 0.0 && __builtin_fabs(ts) <= 1.7976931348623157e308;
}

// The dangling term of one element in teleport mode: q * t in one rounded multiply (the caller adds
// it to S; the host build of this header is compiled with -ffp-contract=off, like the library).
PR_HD inline double batch_dangling_term(double q, double t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(q, t);
#else
  return q * t;
#endif
}

// A lane's factor, chosen at kernel entry: q_j = dc / ts where the column uses the teleport term,
// else the uniform term dc / N itself.  Both quotients are formed, then one is selected.
PR_HD inline double batch_dangling_factor(bool use, double dc, double ts, double n_vertices) {
  const double uni = dc / n_vertices;
#if defined(__HIP_DEVICE_COMPILE__)
  const double q = __ddiv_rn(dc, use ? ts : 1.0);
#else
  const double q = dc / (use ? ts : 1.0);
#endif
  return use ? q : uni;
}

}  // namespace pr
