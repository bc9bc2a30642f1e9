// Batch mixes (pr_batch_mix_topk / pr_batch_mix_get, pr_batch_mix.hip): the blend of one vertex's
// column values under one mix's weights, shared by k_batch_mix and the CPU test shim
// (host/batch_mix_shim.cpp, tests/test_batch_mix_cpu.py).  Plain C++ with PR_HD qualifiers, like
// pr_batch.h.
//
// Mix i scores vertex v by m_i[v], formed over the columns j = 0 .. width-1 in ascending order: a
// column whose weight is exactly 0.0 (either sign) takes no part; the first participating column
// gives acc = w_j * r_j[v], every later one acc = acc + w_j * r_j[v], every product and every sum
// rounded on its own (the host build of this header is compiled with -ffp-contract=off, like the
// library).  A mix with no non-zero weight scores +0.0.  So a one-hot mix with weight 1.0 is its
// column bit for bit (a -0.0 stays -0.0), and an inf or NaN in a column of weight 0 never enters.
//
// The functions below compute exactly that without a branch or a "first column" flag: -0.0 is the
// identity of IEEE addition for every operand (-0.0 + p has the bits of p, also for p = +-0.0, inf
// and NaN), so the sum starts at -0.0, a column of weight 0 adds -0.0 in place of its product (which
// may be 0 * inf = NaN: it is formed and dropped by a select), and batch_mix_result turns the -0.0
// of a mix without any participating column into +0.0.
//
// batch_mix_add has two bodies: the device form names the rounding (__dmul_rn, __dadd_rn, which the
// compiler never contracts), the host form is plain `*` and `+` under -ffp-contract=off.  The CPU
// shim therefore checks the host form and everything around it (the start value, the select, the
// result); that the device form gives the same bits is what tests/test_gpu_batch_mix.py's model
// tests hold the kernel to.
#pragma once

#include "pr_batch.h"

namespace pr {

constexpr int kBatchMaxMixes = 16;  // = PR_BATCH_MAX_MIXES

// Layout stride of the blend matrix for n_mixes mixes: 1, 2, 4, 8 or 16.
PR_HD inline int batch_mix_stride(int n_mixes) { return batch_stride(n_mixes); }

// What the sum of a blend starts from.
PR_HD inline double batch_mix_start() { return -0.0; }

// One column's step of the blend: the sum so far, the column's weight and value.  Every lane of a
// wave runs the same instructions whatever its weight.
PR_HD inline double batch_mix_add(double acc, double w, double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double p = __dmul_rn(w, x);
  return __dadd_rn(acc, w != 0.0 ? p : -0.0);
#else
  const double p = w * x;
  return acc + (w != 0.0 ? p : -0.0);
#endif
}

// The blend from the sum: `any` = some column took part.
PR_HD inline double batch_mix_result(double acc, bool any) { return any ? acc : 0.0; }

// m[v] of one mix from the vertex's `width` column values.
PR_HD inline double batch_mix_elem(const double *w, const double *x, int width) {
  double acc = batch_mix_start();
  bool any = false;
  for (int j = 0; j < width; ++j) {
    acc = batch_mix_add(acc, w[j], x[j]);
    any = any || w[j] != 0.0;
  }
  return batch_mix_result(acc, any);
}

}  // namespace pr
