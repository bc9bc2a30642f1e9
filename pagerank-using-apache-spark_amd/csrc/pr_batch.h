// Batched personalised PageRank (pr_batch.hip): the planner's arithmetic, shared by the library
// and the CPU test shim (host/batch_shim.cpp, tests/test_batch_cpu.py).  Plain C++ with PR_HD
// qualifiers, so a host compiler builds it without the HIP runtime.
//
// A batch advances `width` rank vectors together, stored interleaved as R[v][0..stride) with
// stride = the next power of two >= width.  A wave's 64 lanes form 64 / stride groups of `stride`
// lanes: lane = g * stride + j reads column j of the in-link its group g holds.
//
// Work units are planned once from the canonical row_ptr; a unit is one wave's work:
//   PACK   whole consecutive rows [row0, row0 + rows): at most kBatchUnitRows rows (one row_ptr
//          value per lane) whose in-links total at most batch_unit_cap(stride); empty rows count.
//   CHUNK  in-links [e0, e0 + n) of one row longer than the capacity, cut into consecutive chunks
//          of exactly the capacity (the last one shorter); chunk k's partial sum goes to slot
//          p0 + k and a second kernel adds a row's slots in chunk order.
// Within a row (or chunk) that starts at in-link b, group g adds in-links b + g, b + g + G, ... in
// that order (G = 64 / stride); the G group sums are then combined by a butterfly over the lane
// offsets stride, 2 stride, ..., 32.  A row of a PACK unit with at most kBatchShortRow in-links is
// instead summed by a single lane group in in-link order, G such rows at a time.  The order of a
// row's sum is therefore a function of the row's length and the stride alone.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define PR_HD __host__ __device__
#else
#define PR_HD
#endif

namespace pr {

constexpr int kBatchMaxWidth = 16;
constexpr int kBatchSteps = 64;     // in-links one lane group takes per unit at most
constexpr int kBatchUnitRows = 64;  // rows of a PACK unit at most
constexpr int kBatchShortRow = 8;   // rows of a PACK unit up to this length are summed by one lane group

// Layout stride of a batch of `width` columns: 1, 2, 4, 8 or 16.
PR_HD inline int batch_stride(int width) {
  int s = 1;
  while (s < width) s <<= 1;
  return s;
}
PR_HD inline int batch_groups(int stride) { return 64 / stride; }
// In-links per unit: every group takes kBatchSteps of them (4096 at stride 1, 256 at stride 16).
PR_HD inline int batch_unit_cap(int stride) { return batch_groups(stride) * kBatchSteps; }
// Whether a row of `deg` in-links joins a PACK unit that holds `rows` rows and `n` in-links.
PR_HD inline bool batch_row_fits(int rows, int64_t n, int64_t deg, int cap) {
  return rows < kBatchUnitRows && n + deg <= (int64_t)cap;
}
// Chunks of a row of `deg` > cap in-links, and chunk k's range within the row.
PR_HD inline int64_t batch_chunks(int64_t deg, int cap) { return (deg + cap - 1) / cap; }
PR_HD inline int64_t batch_chunk_begin(int64_t k, int cap) { return k * (int64_t)cap; }
PR_HD inline int64_t batch_chunk_len(int64_t deg, int64_t k, int cap) {
  const int64_t left = deg - batch_chunk_begin(k, cap);
  return left < cap ? left : cap;
}

struct BatchUnit {
  int64_t e0;    // first in-link in canon_col
  int32_t row0;  // first row (PACK) or the long row (CHUNK)
  int32_t rows;  // PACK: rows (>= 1); CHUNK: -(chunk index within the row + 1)
  int32_t n;     // in-links
  int32_t slot;  // CHUNK: partial slot (p0 of the row + chunk index); PACK: 0
};
static_assert(sizeof(BatchUnit) == 24, "BatchUnit must stay 24 bytes");

struct BatchPlan {
  std::vector<BatchUnit> units;
  std::vector<int32_t> long_row;  // rows cut into chunks, ascending
  std::vector<int32_t> long_p0;   // first partial slot of every long row, then the slot count
};

// Plans rows [0, V) of row_ptr (V + 1 entries) for `stride`.
inline void batch_plan(const int64_t *row_ptr, int64_t V, int stride, BatchPlan *plan) {
  const int cap = batch_unit_cap(stride);
  plan->units.clear();
  plan->long_row.clear();
  plan->long_p0.clear();
  BatchUnit cur{0, 0, 0, 0, 0};
  int32_t slots = 0;
  auto flush = [&]() {
    if (cur.rows > 0) plan->units.push_back(cur);
    cur.rows = 0;
    cur.n = 0;
  };
  for (int64_t v = 0; v < V; ++v) {
    const int64_t b = row_ptr[v], deg = row_ptr[v + 1] - b;
    if (deg > cap) {
      flush();
      const int64_t nc = batch_chunks(deg, cap);
      plan->long_row.push_back((int32_t)v);
      plan->long_p0.push_back(slots);
      for (int64_t k = 0; k < nc; ++k)
        plan->units.push_back({b + batch_chunk_begin(k, cap), (int32_t)v, (int32_t)-(k + 1),
                               (int32_t)batch_chunk_len(deg, k, cap), slots++});
      continue;
    }
    if (!batch_row_fits(cur.rows, cur.n, deg, cap)) flush();
    if (cur.rows == 0) {
      cur.e0 = b;
      cur.row0 = (int32_t)v;
    }
    ++cur.rows;
    cur.n += (int32_t)deg;
  }
  flush();
  plan->long_p0.push_back(slots);
}

}  // namespace pr
