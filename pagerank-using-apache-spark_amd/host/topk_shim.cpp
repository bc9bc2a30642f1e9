// Test shim (not product code): exposes the top-K arithmetic of csrc/pr_topk.h -- the rank key
// map, the digits of the composite key, the bin choice -- and a host model of the select to
// tests/test_topk_cpu.py on the CPU.  The model runs the library's own driver
// (topk_select_threshold) with the pass structure of csrc/pr_topk.hip: a histogram pass per digit
// over the rows or, once narrowed, over the compacted candidates; then the emit pass over the rows
// and the host ordering of the selected pairs.
#include "pr_topk.h"

#include <cstring>

extern "C" {

uint64_t prt_rank_key(uint64_t bits) { return pr::topk_rank_key(bits); }
uint64_t prt_rank_bits(uint64_t key) { return pr::topk_rank_bits(key); }
void prt_rank_keys(const uint64_t *bits, int64_t n, uint64_t *keys) {
  for (int64_t i = 0; i < n; ++i) keys[i] = pr::topk_rank_key(bits[i]);
}
uint32_t prt_digit(uint64_t hi, uint32_t lo, int p) { return pr::topk_digit(hi, lo, p); }
int prt_match(uint64_t hi, uint32_t lo, uint64_t phi, uint32_t plo, int p) { return pr::topk_match(hi, lo, phi, plo, p); }
int prt_choose_bin(const uint32_t *hist, uint64_t need, uint64_t *above) { return pr::topk_choose_bin(hist, need, above); }

// ranks / ids: n rows, ids[i] == -1 marks a hole.  Writes min(k, owned rows) pairs in the query's
// order and returns their number (-1: the emit pass did not select exactly that many).
// info[4] as pr_graph.h topk_part.
int64_t prt_select(const double *ranks, const int32_t *ids, int64_t n, int64_t k, int64_t narrow_div,
                   int32_t *ids_out, double *ranks_out, int32_t *info) {
  int64_t owned = 0;
  for (int64_t i = 0; i < n; ++i) owned += ids[i] >= 0;
  const int64_t m = k < owned ? k : owned;
  int passes = 0, passes_cand = 0, narrowed_at = -1;
  auto key_of = [&](int64_t i) {
    uint64_t bits;
    std::memcpy(&bits, &ranks[i], sizeof(bits));
    return pr::topk_rank_key(bits);
  };
  uint64_t thi = 0;
  uint32_t tlo = 0;
  if (m > 0 && m < owned) {
    std::vector<uint64_t> ckey;
    std::vector<uint32_t> cid;
    auto hist_pass = [&](int p, uint64_t phi, uint32_t plo, uint32_t *h) -> int {
      std::memset(h, 0, sizeof(uint32_t) * pr::kTopkBins);
      if (narrowed_at >= 0) {
        ++passes_cand;
        for (size_t i = 0; i < ckey.size(); ++i)
          if (pr::topk_match(ckey[i], cid[i], phi, plo, p)) ++h[pr::topk_digit(ckey[i], cid[i], p)];
      } else {
        for (int64_t i = 0; i < n; ++i) {
          const uint64_t hi = key_of(i);
          const uint32_t lo = pr::topk_id_key(ids[i]);
          if (ids[i] >= 0 && pr::topk_match(hi, lo, phi, plo, p)) ++h[pr::topk_digit(hi, lo, p)];
        }
      }
      return 0;
    };
    auto after_pass = [&](int p, uint64_t phi, uint32_t plo, uint64_t count) -> int {
      if (narrowed_at >= 0 || narrow_div <= 0 || p >= pr::kTopkDigits) return 0;
      if ((int64_t)count > n / narrow_div) return 0;
      for (int64_t i = 0; i < n; ++i) {
        const uint64_t hi = key_of(i);
        const uint32_t lo = pr::topk_id_key(ids[i]);
        if (ids[i] >= 0 && pr::topk_match(hi, lo, phi, plo, p)) {
          ckey.push_back(hi);
          cid.push_back(lo);
        }
      }
      if (ckey.size() != count) return -1;
      narrowed_at = p;
      return 0;
    };
    if (pr::topk_select_threshold((uint64_t)m, hist_pass, after_pass, &thi, &tlo, &passes) != 0) return -1;
  }
  std::vector<pr::TopkPair> v;
  if (m > 0)
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t hi = key_of(i);
      if (ids[i] >= 0 && pr::topk_ge(hi, pr::topk_id_key(ids[i]), thi, tlo)) v.push_back({hi, ids[i]});
    }
  if (info) {
    info[0] = passes;
    info[1] = passes - passes_cand;
    info[2] = passes_cand;
    info[3] = narrowed_at;
  }
  if ((int64_t)v.size() != m) return -1;
  pr::topk_sort_pairs(&v);
  for (int64_t i = 0; i < m; ++i) {
    ids_out[i] = v[(size_t)i].id;
    const uint64_t bits = pr::topk_rank_bits(v[(size_t)i].key);
    std::memcpy(&ranks_out[i], &bits, sizeof(bits));
  }
  return m;
}
}
