// Device-side top-K rank query for gfx950 (pr_get_topk / pr_group_topk; arithmetic in pr_topk.h).
//
// MSD radix select over the 96-bit composite key (rank key, ~original ID) of every owned row,
// then one compaction pass.  Per 8-bit digit one launch of k_topk_hist and a 1 KiB read of its
// histogram by the host, which picks the bin of the K-th key (pr_topk.h topk_select_threshold);
// at most 12 passes, fewer when a bin's count equals what is still missing.  Once the candidates
// (the rows that share the chosen prefix) are at most n_rows / narrow_div, a collect pass compacts
// them into a (key, ~id) buffer (k_topk_collect<false>) and the remaining passes read that buffer
// instead of the rows.  k_topk_collect<true> then writes every row whose key is >= the threshold;
// the K pairs are ordered on the host.
//
// Bytes per pass: 12 per row (8 rank + 4 original ID; hole rows, original ID -1, never take
// part) while the passes read the rows, 12 per candidate after narrowing; the emit pass reads 12
// per row and writes 12 per selected pair.
//
// Skew: ranks share sign, exponent and leading mantissa bits, and whole tie classes are
// bit-identical, so in most passes nearly every candidate of a wave has the same digit.  A wave
// therefore adds equal digits once: the digit of its first candidate lane is broadcast, the lanes
// that hold it are counted with one ballot and the leader adds the count to the wave's private
// LDS histogram; a second round takes the next digit, and only lanes left after that add one by
// one.  No per-element global atomic: a workgroup adds its 256 totals once at the end.
//
// Nothing here reads the environment or touches r, the gather buffers, the statistics or the
// timing events.  The device copy of orig_of_local and all scratch are allocated on the first
// call and freed with the handle.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pr_device.h"
#include "pr_graph.h"
#include "pr_topk.h"

namespace pr {

struct TopkState {
  DevBuf oid;    // int32[n_rows]: original ID of every local row, -1 for a hole
  DevBuf hist;   // u32[kTopkDigits * 256] histograms, then the two append counters
  DevBuf ckey, cid;  // narrowed candidates: u64 rank keys, u32 ~IDs
  DevBuf out_id, out_rank;  // the selected pairs, unordered: u32 ~IDs, u64 rank keys
  int64_t cand_cap = 0, out_cap = 0;
  int grid_max = 0;  // workgroups of a full-device launch
};

namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkBlocksPerCU = 8;
constexpr size_t kTopkHistWords = (size_t)kTopkDigits * kTopkBins;

// Adds digit d of every valid lane to the wave's private histogram hw (wave-uniform call).
__device__ __forceinline__ void wave_hist_add(uint32_t *hw, bool valid, uint32_t d) {
  unsigned long long rem = __ballot(valid);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (rem == 0) break;
    const int leader = __ffsll((long long)rem) - 1;
    const uint32_t dl = (uint32_t)__shfl((int)d, leader, kWave);
    const unsigned long long eq = __ballot(valid && d == dl) & rem;
    if (lane_id() == leader) atomicAdd(&hw[dl], (uint32_t)__popcll(eq));
    rem &= ~eq;
  }
  if ((rem >> lane_id()) & 1ull) atomicAdd(&hw[d], 1u);
}

// Elements 2i and 2i + 1 of the rows (rank, original ID) as composite keys; ok = not a hole and
// inside [0, n).  16 bytes per lane of r, 8 of oid.  oid == nullptr: the identity map (row = ID).
__device__ __forceinline__ void load_rows2(const double *__restrict__ r, const int32_t *__restrict__ oid,
                                           int64_t n, int64_t i, uint64_t hi[2], uint32_t lo[2], bool ok[2]) {
  double2 rv = make_double2(0.0, 0.0);
  int2 ov = make_int2(-1, -1);
  if (2 * i + 1 < n) {
    rv = reinterpret_cast<const double2 *>(r)[i];
    ov = oid ? reinterpret_cast<const int2 *>(oid)[i] : make_int2((int)(2 * i), (int)(2 * i + 1));
  } else if (2 * i < n) {
    rv.x = r[2 * i];
    ov.x = oid ? oid[2 * i] : (int)(2 * i);
  }
  hi[0] = topk_rank_key((uint64_t)__double_as_longlong(rv.x));
  hi[1] = topk_rank_key((uint64_t)__double_as_longlong(rv.y));
  lo[0] = topk_id_key(ov.x);
  lo[1] = topk_id_key(ov.y);
  ok[0] = ov.x >= 0;
  ok[1] = ov.y >= 0;
}

__device__ __forceinline__ void load_cand2(const uint64_t *__restrict__ ckey, const uint32_t *__restrict__ cid,
                                           int64_t n, int64_t i, uint64_t hi[2], uint32_t lo[2], bool ok[2]) {
  ulonglong2 kv = make_ulonglong2(0ull, 0ull);
  uint2 iv = make_uint2(0u, 0u);
  ok[0] = 2 * i < n;
  ok[1] = 2 * i + 1 < n;
  if (ok[1]) {
    kv = reinterpret_cast<const ulonglong2 *>(ckey)[i];
    iv = reinterpret_cast<const uint2 *>(cid)[i];
  } else if (ok[0]) {
    kv.x = ckey[2 * i];
    iv.x = cid[2 * i];
  }
  hi[0] = kv.x;
  hi[1] = kv.y;
  lo[0] = iv.x;
  lo[1] = iv.y;
}

// Histogram of digit p over the candidates of prefix (phi, plo).  kCand: the source is the
// narrowed buffer (ckey, cid) instead of the rows (r, oid).  Grid-stride over pairs of elements;
// the loop count is the same for every lane of the grid, so the ballots see whole waves.
template <bool kCand>
__global__ __launch_bounds__(kTopkThreads) void k_topk_hist(const double *__restrict__ r,
                                                            const int32_t *__restrict__ oid,
                                                            const uint64_t *__restrict__ ckey,
                                                            const uint32_t *__restrict__ cid, int64_t n, int p,
                                                            uint64_t phi, uint32_t plo,
                                                            uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[4 * kTopkBins];
  for (int i = threadIdx.x; i < 4 * kTopkBins; i += kTopkThreads) h[i] = 0;
  __syncthreads();
  uint32_t *hw = h + wave_id() * kTopkBins;
  const int64_t npair = (n + 1) >> 1;
  const int64_t stride = (int64_t)gridDim.x * kTopkThreads;
  for (int64_t base = (int64_t)blockIdx.x * kTopkThreads; base < npair; base += stride) {
    const int64_t i = base + threadIdx.x;
    uint64_t hi[2];
    uint32_t lo[2];
    bool ok[2];
    if (kCand) load_cand2(ckey, cid, n, i, hi, lo, ok);
    else load_rows2(r, oid, n, i, hi, lo, ok);
#pragma unroll
    for (int e = 0; e < 2; ++e)
      wave_hist_add(hw, ok[e] && topk_match(hi[e], lo[e], phi, plo, p), topk_digit(hi[e], lo[e], p));
  }
  __syncthreads();
  const int t = threadIdx.x;
  const uint32_t s = h[t] + h[kTopkBins + t] + h[2 * kTopkBins + t] + h[3 * kTopkBins + t];
  if (s) atomicAdd(&hist[t], s);
}

// Per-wave staging of an append-only output (the compacted candidates, the selected pairs): a
// wave collects the keys it takes in its own kStageCap LDS slots and reserves output space with
// one global atomic per flush -- per >= kStageCap - 63 entries -- instead of one per load, since
// hundreds of thousands of atomics on the one counter word serialise (they cost more than the
// pass's memory traffic).  A flush also writes whole runs of consecutive slots.  Everything is
// wave-synchronous: LDS operations of one wave complete in order, the arrays are volatile so the
// compiler keeps that order, and no barrier is needed.  Calls must be wave-uniform.
constexpr int kStageCap = 256;

struct WaveStage {
  volatile uint64_t *hi;  // this wave's kStageCap rank keys
  volatile uint32_t *lo;  // and ~IDs
  uint32_t cnt;           // staged entries (wave-uniform)
};

__device__ __forceinline__ void stage_flush(WaveStage &st, uint64_t *__restrict__ okey, uint32_t *__restrict__ oid,
                                            uint32_t *__restrict__ counter, uint32_t cap) {
  if (st.cnt == 0) return;
  uint32_t base = 0;
  if (lane_id() == 0) base = atomicAdd(counter, st.cnt);
  base = (uint32_t)__shfl((int)base, 0, kWave);
  for (uint32_t j = lane_id(); j < st.cnt; j += kWave) {
    const uint32_t pos = base + j;
    if (pos < cap) {  // cap = the entries the histograms counted: a slot past it is never written
      okey[pos] = st.hi[j];
      oid[pos] = st.lo[j];
    }
  }
  st.cnt = 0;
}

__device__ __forceinline__ void stage_append(WaveStage &st, bool take, uint64_t hi, uint32_t lo,
                                             uint64_t *__restrict__ okey, uint32_t *__restrict__ oid,
                                             uint32_t *__restrict__ counter, uint32_t cap) {
  const unsigned long long m = __ballot(take);
  const uint32_t c = (uint32_t)__popcll(m);
  if (c == 0) return;
  if (st.cnt + c > (uint32_t)kStageCap) stage_flush(st, okey, oid, counter, cap);
  if (take) {
    const uint32_t slot = st.cnt + (uint32_t)__popcll(m & lanemask_lt());
    st.hi[slot] = hi;
    st.lo[slot] = lo;
  }
  st.cnt += c;
}

// Appends (rank key, ~original ID) of the rows it selects to (okey, oid), in any order.  kGe: the
// rows whose composite key is >= (phi, plo) -- the emit pass, (phi, plo) = the threshold; otherwise
// the rows that agree with the prefix (phi, plo) on digits 0..p-1 -- the narrowing pass.
template <bool kGe>
__global__ __launch_bounds__(kTopkThreads) void k_topk_collect(const double *__restrict__ r,
                                                               const int32_t *__restrict__ oid, int64_t n, int p,
                                                               uint64_t phi, uint32_t plo,
                                                               uint64_t *__restrict__ okey,
                                                               uint32_t *__restrict__ olo,
                                                               uint32_t *__restrict__ counter, uint32_t cap) {
  __shared__ uint64_t shi[(kTopkThreads / kWave) * kStageCap];
  __shared__ uint32_t slo[(kTopkThreads / kWave) * kStageCap];
  WaveStage st{shi + wave_id() * kStageCap, slo + wave_id() * kStageCap, 0u};
  const int64_t npair = (n + 1) >> 1;
  const int64_t stride = (int64_t)gridDim.x * kTopkThreads;
  for (int64_t base = (int64_t)blockIdx.x * kTopkThreads; base < npair; base += stride) {
    uint64_t hi[2];
    uint32_t lo[2];
    bool ok[2];
    load_rows2(r, oid, n, base + threadIdx.x, hi, lo, ok);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool take = ok[e] && (kGe ? topk_ge(hi[e], lo[e], phi, plo) : topk_match(hi[e], lo[e], phi, plo, p));
      stage_append(st, take, hi[e], lo[e], okey, olo, counter, cap);
    }
  }
  stage_flush(st, okey, olo, counter, cap);
}

// The select's scratch (histograms, launch geometry), allocated on first use.
int topk_scratch(TopkState **st, int device) {
  if (!*st) {
    TopkState *t = new (std::nothrow) TopkState();
    if (!t) return fail(PR_ERR_OOM, "host allocation failed");
    *st = t;
  }
  TopkState *t = *st;
  if (!t->hist.p) {
    int cus = 0;
    PR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    t->grid_max = std::max(1, cus) * kTopkBlocksPerCU;
    PR_TRY(t->hist.alloc(sizeof(uint32_t) * (kTopkHistWords + 2)));
  }
  return PR_OK;
}

int topk_state(pr_graph *g, TopkState **out) {
  PR_TRY(topk_scratch(&g->topk, g->device));
  TopkState *t = g->topk;
  if (!t->oid.p) {
    DevBuf oid;
    PR_TRY(oid.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(g->n_rows, 1)));
    if (g->n_rows > 0)
      PR_HIP(hipMemcpyAsync(oid.p, g->orig_of_local.data(), sizeof(int32_t) * g->n_rows, hipMemcpyHostToDevice,
                            g->stream));
    PR_HIP(hipStreamSynchronize(g->stream));
    t->oid = std::move(oid);
  }
  *out = t;
  return PR_OK;
}

unsigned topk_grid(const TopkState *t, int64_t n) {
  const int64_t npair = (n + 1) >> 1;
  int64_t b = (npair + kTopkThreads - 1) / kTopkThreads;
  if (b < 1) b = 1;
  if (b > t->grid_max) b = t->grid_max;
  return (unsigned)b;
}

}  // namespace

size_t topk_state_bytes(const TopkState *t) {
  if (!t) return 0;
  return t->oid.bytes + t->hist.bytes + t->ckey.bytes + t->cid.bytes + t->out_id.bytes + t->out_rank.bytes;
}

void topk_state_free(TopkState *t) { delete t; }  // DevBufs free their memory

size_t topk_bytes(const pr_graph *g) { return topk_state_bytes(g->topk); }

void topk_destroy(pr_graph *g) {
  topk_state_free(g->topk);
  g->topk = nullptr;
}

int topk_part(pr_graph *g, int64_t k, int64_t narrow_div, int32_t *ids_out, double *ranks_out, int32_t *n_out,
              int32_t *info) {
  PR_TRY(join_exchange(g));
  PR_HIP(hipStreamSynchronize(g->stream));
  if (std::min<int64_t>(k, g->n_local) > 0) {
    if (g->n_rows >= (int64_t(1) << 32)) return fail(PR_ERR_INVALID, "pr_get_topk: n_rows >= 2^32");
    TopkState *t = nullptr;
    PR_TRY(topk_state(g, &t));  // uploads the row -> original ID map on the first call
  }
  return topk_select(&g->topk, g->device, g->stream, g->r.as<double>(), g->topk ? g->topk->oid.as<int32_t>() : nullptr,
                     g->n_rows, g->n_local, k, narrow_div, ids_out, ranks_out, n_out, info);
}

// The select over n_rows (rank, original ID) rows of which n_owned are not holes; oid == nullptr:
// row i is vertex i (no holes).  *state is created on first use.

int topk_select(TopkState **state, int device, hipStream_t s, const double *r, const int32_t *oid, int64_t n_rows,
                int64_t n_owned, int64_t k, int64_t narrow_div, int32_t *ids_out, double *ranks_out, int32_t *n_out,
                int32_t *info) {
  PR_HIP(hipStreamSynchronize(s));
  const int64_t n = std::min<int64_t>(k, n_owned);
  int passes = 0, passes_cand = 0, narrowed_at = -1;
  if (n > 0) {
    if (!oid && n_rows >= (int64_t(1) << 31)) return fail(PR_ERR_INVALID, "top-K: n_rows >= 2^31");
    PR_TRY(topk_scratch(state, device));
    TopkState *t = *state;
    if (t->out_cap < n) {
      t->out_cap = 0;
      PR_TRY(t->out_id.alloc(sizeof(int32_t) * (size_t)n));
      PR_TRY(t->out_rank.alloc(sizeof(uint64_t) * (size_t)n));
      t->out_cap = n;
    }
    uint32_t *hist = t->hist.as<uint32_t>();
    uint32_t *ctr = hist + kTopkHistWords;
    PR_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (kTopkHistWords + 2), s));
    uint64_t thi = 0;
    uint32_t tlo = 0;
    if (n < n_owned) {  // otherwise every owned row is selected: threshold 0
      int64_t cand_n = 0;
      auto hist_pass = [&](int p, uint64_t phi, uint32_t plo, uint32_t *h) -> int {
        uint32_t *dh = hist + (size_t)p * kTopkBins;
        if (narrowed_at >= 0) {
          hipLaunchKernelGGL(k_topk_hist<true>, dim3(topk_grid(t, cand_n)), dim3(kTopkThreads), 0, s, nullptr,
                             nullptr, t->ckey.as<uint64_t>(), t->cid.as<uint32_t>(), cand_n, p, phi, plo, dh);
          ++passes_cand;
        } else {
          hipLaunchKernelGGL(k_topk_hist<false>, dim3(topk_grid(t, n_rows)), dim3(kTopkThreads), 0, s, r, oid,
                             nullptr, nullptr, n_rows, p, phi, plo, dh);
        }
        PR_HIP(hipGetLastError());
        PR_HIP(hipMemcpyAsync(h, dh, sizeof(uint32_t) * kTopkBins, hipMemcpyDeviceToHost, s));
        PR_HIP(hipStreamSynchronize(s));
        return PR_OK;
      };
      auto after_pass = [&](int p, uint64_t phi, uint32_t plo, uint64_t count) -> int {
        if (narrowed_at >= 0 || narrow_div <= 0 || p >= kTopkDigits) return PR_OK;
        if ((int64_t)count > n_rows / narrow_div) return PR_OK;
        if (t->cand_cap < (int64_t)count) {
          t->cand_cap = 0;
          PR_TRY(t->ckey.alloc(sizeof(uint64_t) * (size_t)count));
          PR_TRY(t->cid.alloc(sizeof(uint32_t) * (size_t)count));
          t->cand_cap = (int64_t)count;
        }
        hipLaunchKernelGGL(k_topk_collect<false>, dim3(topk_grid(t, n_rows)), dim3(kTopkThreads), 0, s, r, oid,
                           n_rows, p, phi, plo, t->ckey.as<uint64_t>(), t->cid.as<uint32_t>(), ctr, (uint32_t)count);
        PR_HIP(hipGetLastError());
        cand_n = (int64_t)count;
        narrowed_at = p;
        return PR_OK;
      };
      PR_TRY(topk_select_threshold((uint64_t)n, hist_pass, after_pass, &thi, &tlo, &passes));
    }
    hipLaunchKernelGGL(k_topk_collect<true>, dim3(topk_grid(t, n_rows)), dim3(kTopkThreads), 0, s, r, oid,
                       n_rows, 0, thi, tlo, t->out_rank.as<uint64_t>(), t->out_id.as<uint32_t>(), ctr + 1, (uint32_t)n);
    PR_HIP(hipGetLastError());
    uint32_t counts[2] = {0, 0};
    std::vector<uint32_t> hid((size_t)n);
    std::vector<uint64_t> hkey((size_t)n);
    PR_HIP(hipMemcpyAsync(counts, ctr, sizeof(counts), hipMemcpyDeviceToHost, s));
    PR_HIP(hipMemcpyAsync(hid.data(), t->out_id.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    PR_HIP(hipMemcpyAsync(hkey.data(), t->out_rank.p, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    PR_HIP(hipStreamSynchronize(s));
    if ((int64_t)counts[1] != n)
      return fail(PR_ERR_HIP, "pr_get_topk: selected " + std::to_string(counts[1]) + " of " + std::to_string(n) +
                                  " pairs (duplicate original IDs?)");
    std::vector<TopkPair> v((size_t)n);
    for (int64_t i = 0; i < n; ++i) v[(size_t)i] = {hkey[(size_t)i], (int32_t)~hid[(size_t)i]};
    topk_sort_pairs(&v);
    for (int64_t i = 0; i < n; ++i) {
      ids_out[i] = v[(size_t)i].id;
      const uint64_t bits = topk_rank_bits(v[(size_t)i].key);
      std::memcpy(&ranks_out[i], &bits, sizeof(bits));
    }
  }
  *n_out = (int32_t)n;
  if (info) {
    info[0] = passes;
    info[1] = passes - passes_cand;
    info[2] = passes_cand;
    info[3] = narrowed_at;
  }
  return PR_OK;
}

}  // namespace pr
