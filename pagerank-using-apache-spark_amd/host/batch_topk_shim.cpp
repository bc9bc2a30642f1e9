// Test shim (not product code): exposes the per-column state of the batch top-K (csrc/pr_batch_topk.h
// btopk_begin / btopk_advance) and a host model of the lockstep select to
// tests/test_batch_topk_cpu.py on the CPU.  The model runs the library's own driver
// (btopk_select_thresholds) with the pass structure of csrc/pr_batch_topk.hip: per digit one sweep
// over the interleaved V x stride matrix that builds every active column's histogram, or, once
// narrowed, over every active column's segment of the compacted candidates; then the emit sweep
// and the host ordering of every column's pairs.
#include "pr_batch_topk.h"

#include <cstring>

namespace {

uint64_t key_of(const double *R, int64_t q) {
  uint64_t bits;
  std::memcpy(&bits, &R[q], sizeof(bits));
  return pr::topk_rank_key(bits);
}

}  // namespace

extern "C" {

// state = {phi, plo, need, cand, done} as five u64; one btopk_begin / btopk_advance on it.
void prbt_begin(uint64_t *state, uint64_t k, uint64_t n_avail) {
  pr::BTopkCol c;
  pr::btopk_begin(&c, k, n_avail);
  state[0] = c.phi, state[1] = c.plo, state[2] = c.need, state[3] = c.cand, state[4] = c.done;
}
void prbt_advance(uint64_t *state, int p, const uint32_t *hist) {
  pr::BTopkCol c;
  c.phi = state[0], c.plo = (uint32_t)state[1], c.need = state[2], c.cand = state[3], c.done = state[4] != 0;
  pr::btopk_advance(&c, p, hist);
  state[0] = c.phi, state[1] = c.plo, state[2] = c.need, state[3] = c.cand, state[4] = c.done;
}

// The threshold of topk_select_threshold for the k largest of n composite keys (hi[i], lo[i]),
// 1 <= k <= n, histograms on the host; returns the passes it ran.
int prbt_threshold_ref(const uint64_t *hi, const uint32_t *lo, int64_t n, uint64_t k, uint64_t *thi, uint32_t *tlo) {
  int passes = 0;
  auto hist_pass = [&](int p, uint64_t phi, uint32_t plo, uint32_t *h) -> int {
    std::memset(h, 0, sizeof(uint32_t) * pr::kTopkBins);
    for (int64_t i = 0; i < n; ++i)
      if (pr::topk_match(hi[i], lo[i], phi, plo, p)) ++h[pr::topk_digit(hi[i], lo[i], p)];
    return 0;
  };
  auto after_pass = [](int, uint64_t, uint32_t, uint64_t) -> int { return 0; };
  if (pr::topk_select_threshold(k, hist_pass, after_pass, thi, tlo, &passes) != 0) return -1;
  return passes;
}

// R: V x stride doubles, element (v, j) at v * stride + j; mask (V entries, may be NULL): bit j of
// mask[v] leaves v out of column j.  Column j's min(k, V - excluded_j) pairs go to ids_out /
// ranks_out[j * k ..) in the query's order, their number to n_out[j]; thr_hi / thr_lo / col_passes
// [width] get every column's threshold and the passes it took part in.  info[4] as pr_graph.h
// btopk_select.  Returns 0, or -1 when a sweep did not yield what the histograms counted.
int prbt_select(const double *R, int64_t V, int stride, int width, const uint16_t *mask, int64_t k, int64_t narrow_div,
                int32_t *ids_out, double *ranks_out, int32_t *n_out, uint64_t *thr_hi, uint32_t *thr_lo,
                int32_t *col_passes, int32_t *info) {
  pr::BTopkCol cols[pr::kBTopkMaxCols];
  int64_t n_sel[pr::kBTopkMaxCols] = {0};
  auto excluded = [&](int64_t v, int j) { return mask && ((mask[v] >> j) & 1u); };
  for (int j = 0; j < width; ++j) {
    int64_t avail = 0;
    for (int64_t v = 0; v < V; ++v) avail += !excluded(v, j);
    n_sel[j] = k < avail ? k : avail;
    pr::btopk_begin(&cols[j], (uint64_t)n_sel[j], (uint64_t)avail);
    col_passes[j] = 0;
  }
  int passes = 0, passes_cand = 0, narrowed_at = -1;
  std::vector<uint64_t> ckey[pr::kBTopkMaxCols];
  std::vector<uint32_t> cid[pr::kBTopkMaxCols];
  auto hist_pass = [&](int p, const pr::BTopkCol *cs, uint32_t *h) -> int {
    std::memset(h, 0, sizeof(uint32_t) * (size_t)stride * pr::kTopkBins);
    if (narrowed_at >= 0) {
      ++passes_cand;
      for (int j = 0; j < width; ++j) {
        if (cs[j].done) continue;
        for (size_t i = 0; i < ckey[j].size(); ++i)
          if (pr::topk_match(ckey[j][i], cid[j][i], cs[j].phi, cs[j].plo, p))
            ++h[j * pr::kTopkBins + pr::topk_digit(ckey[j][i], cid[j][i], p)];
      }
    } else {
      for (int64_t q = 0; q < V * stride; ++q) {  // the sweep: element q is of column q % stride
        const int j = (int)(q % stride);
        const int64_t v = q / stride;
        if (j >= width || cs[j].done || excluded(v, j)) continue;
        const uint64_t hi = key_of(R, q);
        const uint32_t lo = pr::topk_id_key((int32_t)v);
        if (pr::topk_match(hi, lo, cs[j].phi, cs[j].plo, p)) ++h[j * pr::kTopkBins + pr::topk_digit(hi, lo, p)];
      }
    }
    for (int j = 0; j < width; ++j) col_passes[j] += !cs[j].done;
    return 0;
  };
  auto narrow = [&](int p, const pr::BTopkCol *cs, uint64_t total) -> int {
    uint64_t got = 0;
    for (int64_t q = 0; q < V * stride; ++q) {
      const int j = (int)(q % stride);
      const int64_t v = q / stride;
      if (j >= width || cs[j].done || excluded(v, j)) continue;
      const uint64_t hi = key_of(R, q);
      const uint32_t lo = pr::topk_id_key((int32_t)v);
      if (pr::topk_match(hi, lo, cs[j].phi, cs[j].plo, p)) {
        ckey[j].push_back(hi);
        cid[j].push_back(lo);
        ++got;
      }
    }
    for (int j = 0; j < width; ++j)
      if (!cs[j].done && ckey[j].size() != cs[j].cand) return -1;
    if (got != total) return -1;
    narrowed_at = p;
    return 0;
  };
  int drv_narrowed = -1;
  if (pr::btopk_select_thresholds(width, cols, pr::btopk_narrow_limit(V, width, narrow_div), hist_pass, narrow, &passes,
                                  &drv_narrowed) != 0)
    return -1;
  if (info) {
    info[0] = passes;
    info[1] = passes - passes_cand;
    info[2] = passes_cand;
    info[3] = narrowed_at;
  }
  for (int j = 0; j < width; ++j) {
    thr_hi[j] = cols[j].phi;
    thr_lo[j] = cols[j].plo;
    std::vector<pr::TopkPair> v;
    if (n_sel[j] > 0)
      for (int64_t x = 0; x < V; ++x) {
        const uint64_t hi = key_of(R, x * stride + j);
        if (!excluded(x, j) && pr::topk_ge(hi, pr::topk_id_key((int32_t)x), cols[j].phi, cols[j].plo))
          v.push_back({hi, (int32_t)x});
      }
    if ((int64_t)v.size() != n_sel[j]) return -1;
    pr::topk_sort_pairs(&v);
    for (int64_t i = 0; i < n_sel[j]; ++i) {
      ids_out[j * k + i] = v[(size_t)i].id;
      const uint64_t bits = pr::topk_rank_bits(v[(size_t)i].key);
      std::memcpy(&ranks_out[j * k + i], &bits, sizeof(bits));
    }
    n_out[j] = (int32_t)n_sel[j];
  }
  return 0;
}
}
