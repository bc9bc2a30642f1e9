// Top-K rank query (pr_topk.hip): the arithmetic shared by the device kernels, the host driver of
// the select and the CPU test shim (host/topk_shim.cpp, tests/test_topk_cpu.py).  Plain C++ with
// PR_HD qualifiers, so a host compiler builds it without the HIP runtime.
//
// Order of the query: rank descending, ties by original vertex ID ascending.  Every vertex gets a
// 96-bit composite key (hi = the order-preserving u64 image of its rank's IEEE-754 bits, lo =
// ~original ID); composite keys are unique per vertex and "the K best" = "the K largest keys".
// The select is an MSD radix select over the kTopkDigits 8-bit digits of that key: pass p builds
// the histogram of digit p over the candidates (the keys that agree with the chosen prefix on
// digits 0..p-1), topk_choose_bin picks the bin holding the K-th largest key, and everything in a
// higher bin is already known to be selected.  After the last pass (or as soon as a bin's count
// equals what is still missing) the K-th key itself is known as a threshold T, and the result is
// every vertex with key >= T.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PR_HD __host__ __device__
#else
#define PR_HD
#endif

namespace pr {

constexpr int kTopkDigitBits = 8;
constexpr int kTopkBins = 1 << kTopkDigitBits;  // 256
constexpr int kTopkHiDigits = 8;                // digits 0..7: the rank key, most significant first
constexpr int kTopkDigits = 12;                 // digits 8..11: ~original ID

// IEEE-754 bits -> u64 whose unsigned order is the numeric order: a non-negative value gets its
// sign bit set, a negative one all bits inverted (-0.0 lands just below +0.0).
PR_HD inline uint64_t topk_rank_key(uint64_t bits) {
  return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}
PR_HD inline uint64_t topk_rank_bits(uint64_t key) {  // the inverse
  return (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
}
PR_HD inline uint32_t topk_id_key(int32_t orig_id) { return ~(uint32_t)orig_id; }

// Digit p (0 = most significant) of the composite key (hi, lo).
PR_HD inline uint32_t topk_digit(uint64_t hi, uint32_t lo, int p) {
  return p < kTopkHiDigits ? (uint32_t)(hi >> (56 - 8 * p)) & 0xFFu
                           : (lo >> (24 - 8 * (p - kTopkHiDigits))) & 0xFFu;
}

// Whether (hi, lo) agrees with the prefix (phi, plo) on digits 0..p-1 (p = 0: always).
PR_HD inline bool topk_match(uint64_t hi, uint32_t lo, uint64_t phi, uint32_t plo, int p) {
  if (p <= 0) return true;
  if (p < kTopkHiDigits) return ((hi ^ phi) >> (64 - 8 * p)) == 0;
  if (hi != phi) return false;
  if (p == kTopkHiDigits) return true;
  if (p >= kTopkDigits) return lo == plo;
  return ((lo ^ plo) >> (32 - 8 * (p - kTopkHiDigits))) == 0;
}

// The prefix extended by digit p = bin (the lower digits of the prefix are zero).
PR_HD inline void topk_extend(uint64_t *phi, uint32_t *plo, int p, uint32_t bin) {
  if (p < kTopkHiDigits) *phi |= (uint64_t)bin << (56 - 8 * p);
  else *plo |= bin << (24 - 8 * (p - kTopkHiDigits));
}

// (hi, lo) >= (thi, tlo) as 96-bit numbers.
PR_HD inline bool topk_ge(uint64_t hi, uint32_t lo, uint64_t thi, uint32_t tlo) {
  return hi > thi || (hi == thi && lo >= tlo);
}

// The bin of `hist` (kTopkBins counts of one digit over the candidates) that holds the need-th
// largest candidate, 1 <= need <= sum(hist); *above = the candidates in higher bins (all selected).
PR_HD inline int topk_choose_bin(const uint32_t *hist, uint64_t need, uint64_t *above) {
  uint64_t acc = 0;
  for (int b = kTopkBins - 1; b > 0; --b) {
    if (acc + hist[b] >= need) {
      *above = acc;
      return b;
    }
    acc += hist[b];
  }
  *above = acc;
  return 0;
}

// Host driver of the select, shared by the library (device histograms) and the CPU model of the
// shim (host histograms): `hist_pass(p, phi, plo, hist)` fills hist[kTopkBins] with the digit-p
// counts of the candidates of prefix (phi, plo) and returns 0, or an error code that ends the
// select.  `after_pass(p, phi, plo, count)` is told the prefix (now p digits) and its candidate
// count after every pass that did not end the select (the library compacts the candidates there).
// k must be in [1, number of keys].  On return (*thi, *tlo) is the threshold: exactly k keys are
// >= it.  *passes = histogram passes run.
template <class HistPass, class AfterPass>
inline int topk_select_threshold(uint64_t k, HistPass hist_pass, AfterPass after_pass, uint64_t *thi,
                                 uint32_t *tlo, int *passes) {
  uint64_t phi = 0;
  uint32_t plo = 0;
  uint64_t need = k;
  int p = 0;
  for (; p < kTopkDigits; ++p) {
    uint32_t hist[kTopkBins];
    const int rc = hist_pass(p, phi, plo, hist);
    if (rc != 0) return rc;
    uint64_t above = 0;
    const int b = topk_choose_bin(hist, need, &above);
    need -= above;
    topk_extend(&phi, &plo, p, (uint32_t)b);
    if (hist[b] == need) {  // the whole bin is selected: the prefix with zero low digits is T
      ++p;
      break;
    }
    const int rc2 = after_pass(p + 1, phi, plo, (uint64_t)hist[b]);
    if (rc2 != 0) return rc2;
  }
  *thi = phi;
  *tlo = plo;
  *passes = p;
  return 0;
}

// One selected vertex on the host: its rank key and original ID.  The query's order.
struct TopkPair {
  uint64_t key;
  int32_t id;
};
inline bool topk_before(const TopkPair &a, const TopkPair &b) { return a.key != b.key ? a.key > b.key : a.id < b.id; }
inline void topk_sort_pairs(std::vector<TopkPair> *v) { std::sort(v->begin(), v->end(), topk_before); }

}  // namespace pr
