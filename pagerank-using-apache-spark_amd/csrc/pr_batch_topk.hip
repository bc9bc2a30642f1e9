// Batch top-K for gfx950 (pr_batch_get_topk_all; arithmetic and host driver in pr_batch_topk.h):
// the top-K lists of every column of a batch from one lockstep select over the interleaved
// V x stride rank matrix R, element (v, j) at v * stride + j.
//
// The select is pr_topk.hip's MSD radix select, run for all columns at once.  Per 8-bit digit one
// launch of k_btopk_hist<S> sweeps R once, coalesced, and leaves stride x 256 counts; the host
// reads them in one copy (at most 16 KiB) and advances every active column (btopk_advance): one
// synchronisation per pass for all columns.  Once the active columns' candidates together are at
// most V * width / narrow_div, one launch of k_btopk_collect<S, false> compacts every active
// column's candidates (key, ~id) into that column's segment of a candidate buffer -- the segment
// lengths are the histogram counts, their bases a prefix sum -- and the remaining passes read the
// segments (k_btopk_hist_cand) instead of R.  k_btopk_collect<S, true> then writes every element
// whose key is >= its column's threshold into the column's output segment; the host checks the
// per-column counters against the expected lengths and orders each column (topk_sort_pairs).
//
// A lane of the sweeps stays in one column: the workgroup size is a multiple of S, so a thread's
// elements all have column threadIdx.x % S, and it loads its column's prefix and activity once from
// a small per-column device array.  Padding columns, finished columns and excluded elements (bit j
// of mask[v]; mask == nullptr: no column excludes anything) never count and their lanes load nothing.
//
// Skew: in most passes every candidate of a column has the same digit, and a lane's elements are
// all of one column, so a lane counts the run of equal digits in a register and adds a run to the
// workgroup's LDS histogram (S x 256 counters, 16 KiB at S = 16: eight workgroups of 256 threads per
// CU keep all 32 wave slots) only when the digit changes -- once per lane in such a pass.  No
// per-element global atomic: a workgroup adds its non-zero totals once.
//
// Appends are staged per wave as pr_topk.hip's WaveStage does, with the entry's column next to it: a
// flush ranks the staged entries per column with ballots, reserves output space with one atomic
// instruction (lane j adds column j's count to column j's counter) and writes each entry to its
// column's segment, never past the segment's length.
#include <algorithm>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "pr_batch_topk.h"
#include "pr_device.h"
#include "pr_graph.h"

namespace pr {

// What a lane knows of its column during one launch.
struct BTopkColDev {
  uint64_t phi;       // prefix (hist, narrowing) or threshold (emit), high part
  uint64_t seg_base;  // first slot of the column's segment: candidates (narrowing, candidate passes) or output (emit)
  uint32_t plo;
  uint32_t seg_len;
  int32_t active;     // takes part in this launch
  int32_t pad;
};
static_assert(sizeof(BTopkColDev) == 32, "BTopkColDev must stay 32 bytes");

struct BTopkState {
  DevBuf hist;  // u32[kTopkDigits * S * 256] histograms, then S candidate and S output counters
  DevBuf cols;  // BTopkColDev[kBTopkMaxCols]
  DevBuf ckey, cid;         // narrowed candidates, all columns: u64 rank keys, u32 ~IDs
  DevBuf out_key, out_id;   // the selected pairs, column segments, unordered
  int64_t cand_cap = 0, out_cap = 0;
  int grid_max = 0;  // workgroups of a full-device launch
  // timed calls only (info != nullptr): an event before and after every kernel launch
  std::vector<hipEvent_t> ev;
  int64_t kernel_ns = -1;  // sum over the launches of the last timed call
};

namespace {

constexpr int kBtThreads = 256;
constexpr int kBtUnroll = 4;  // elements a lane loads per step
constexpr int kBtTile = kBtThreads * kBtUnroll;
constexpr int kBtBlocksPerCU = 8;
constexpr int kBtStageCap = 256;
constexpr int kBtChunks = kBtStageCap / kWave;

// Elements base + u * kBtThreads + threadIdx.x, u < kBtUnroll, of R as composite keys of column j
// (all of them: kBtThreads is a multiple of S); ok = inside [0, n) and not excluded from column j.
// A lane with live == false loads nothing.
template <int S>
__device__ __forceinline__ void bt_load(const double *__restrict__ R, const uint16_t *__restrict__ mask, int64_t n,
                                        int64_t base, int j, bool live, uint64_t hi[kBtUnroll], uint32_t lo[kBtUnroll],
                                        bool ok[kBtUnroll]) {
  double x[kBtUnroll];
  uint32_t mb[kBtUnroll];
#pragma unroll
  for (int u = 0; u < kBtUnroll; ++u) {
    const int64_t q = base + (int64_t)u * kBtThreads + threadIdx.x;
    ok[u] = live && q < n;
    x[u] = ok[u] ? R[q] : 0.0;
    mb[u] = (ok[u] && mask) ? (uint32_t)mask[q / S] : 0u;
  }
#pragma unroll
  for (int u = 0; u < kBtUnroll; ++u) {
    const int64_t q = base + (int64_t)u * kBtThreads + threadIdx.x;
    hi[u] = topk_rank_key((uint64_t)__double_as_longlong(x[u]));
    lo[u] = topk_id_key((int32_t)(q / S));
    ok[u] = ok[u] && !((mb[u] >> j) & 1u);
  }
}

// Histograms of digit p of every active column over R[0 .. n), n = V * S.
template <int S>
__global__ __launch_bounds__(kBtThreads) void k_btopk_hist(const double *__restrict__ R,
                                                           const uint16_t *__restrict__ mask, int64_t n, int p,
                                                           const BTopkColDev *__restrict__ cols,
                                                           uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[S * kTopkBins];
  for (int i = threadIdx.x; i < S * kTopkBins; i += kBtThreads) h[i] = 0;
  const int j = threadIdx.x % S;
  const BTopkColDev c = cols[j];
  __syncthreads();
  if (c.active) {  // no barrier or cross-lane operation inside: lanes of a wave may differ here
    uint32_t *hj = h + j * kTopkBins;
    uint32_t cur = 0, run = 0;  // the lane's current run: `run` candidates with digit `cur`
    const int64_t stride = (int64_t)gridDim.x * kBtTile;
    for (int64_t base = (int64_t)blockIdx.x * kBtTile; base < n; base += stride) {
      uint64_t hi[kBtUnroll];
      uint32_t lo[kBtUnroll];
      bool ok[kBtUnroll];
      bt_load<S>(R, mask, n, base, j, true, hi, lo, ok);
#pragma unroll
      for (int u = 0; u < kBtUnroll; ++u) {
        if (!(ok[u] && topk_match(hi[u], lo[u], c.phi, c.plo, p))) continue;
        const uint32_t d = topk_digit(hi[u], lo[u], p);
        if (d == cur) {
          ++run;
        } else {
          if (run) atomicAdd(&hj[cur], run);
          cur = d;
          run = 1;
        }
      }
    }
    if (run) atomicAdd(&hj[cur], run);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S * kTopkBins; i += kBtThreads) {
    const uint32_t v = h[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

// Adds digit d of every valid lane to the histogram hw (wave-uniform call): equal digits of a wave
// are added once (pr_topk.hip wave_hist_add).
__device__ __forceinline__ void bt_wave_hist_add(uint32_t *hw, bool valid, uint32_t d) {
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

// Histogram of digit p over the candidate segment of column blockIdx.y.  All lanes of a workgroup
// are of one column, and the loop count is the same for every lane of it, so the ballots see whole
// waves.
__global__ __launch_bounds__(kBtThreads) void k_btopk_hist_cand(const uint64_t *__restrict__ ckey,
                                                                const uint32_t *__restrict__ cid, int p,
                                                                const BTopkColDev *__restrict__ cols,
                                                                uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[kTopkBins];
  const int j = blockIdx.y;
  const BTopkColDev c = cols[j];
  if (!c.active || c.seg_len == 0) return;  // the whole workgroup
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t *__restrict__ key = ckey + c.seg_base;
  const uint32_t *__restrict__ id = cid + c.seg_base;
  const int64_t len = c.seg_len, stride = (int64_t)gridDim.x * kBtThreads;
  for (int64_t base = (int64_t)blockIdx.x * kBtThreads; base < len; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool ok = i < len;
    const uint64_t hi = ok ? key[i] : 0ull;
    const uint32_t lo = ok ? id[i] : 0u;
    bt_wave_hist_add(h, ok && topk_match(hi, lo, c.phi, c.plo, p), topk_digit(hi, lo, p));
  }
  __syncthreads();
  const uint32_t v = h[threadIdx.x];
  if (v) atomicAdd(&hist[j * kTopkBins + threadIdx.x], v);
}

// Per-wave staging of the appends of a sweep: kBtStageCap slots of (rank key, ~ID, column) in LDS.
// Everything is wave-synchronous: LDS operations of one wave complete in order, the arrays are
// volatile so the compiler keeps that order, and no barrier is needed.  Calls must be wave-uniform.
struct BtStage {
  volatile uint64_t *hi;
  volatile uint32_t *lo;
  volatile uint8_t *col;
  uint32_t cnt;  // staged entries (wave-uniform)
};

// `c` is the calling lane's column: lane j < S of a wave holds column j (64 is a multiple of S).
template <int S>
__device__ __forceinline__ void bt_stage_flush(BtStage &st, const BTopkColDev &c, uint64_t *__restrict__ okey,
                                               uint32_t *__restrict__ oid, uint32_t *__restrict__ counters) {
  if (st.cnt == 0) return;
  const int lane = lane_id();
  const unsigned long long lt = lanemask_lt();
  uint32_t running[S];  // entries of column jj seen so far (wave-uniform)
#pragma unroll
  for (int jj = 0; jj < S; ++jj) running[jj] = 0;
  uint32_t rank[kBtChunks];
  int ce[kBtChunks];
#pragma unroll
  for (int ch = 0; ch < kBtChunks; ++ch) {
    const uint32_t e = (uint32_t)(ch * kWave + lane);
    ce[ch] = e < st.cnt ? (int)st.col[e] : -1;
    rank[ch] = 0;
#pragma unroll
    for (int jj = 0; jj < S; ++jj) {
      const unsigned long long m = __ballot(ce[ch] == jj);
      if (ce[ch] == jj) rank[ch] = running[jj] + (uint32_t)__popcll(m & lt);
      running[jj] += (uint32_t)__popcll(m);
    }
  }
  uint32_t mine = 0;
#pragma unroll
  for (int jj = 0; jj < S; ++jj)
    if (lane == jj) mine = running[jj];
  uint32_t base = 0;
  if (lane < S && mine) base = atomicAdd(&counters[lane], mine);  // one atomic instruction per flush
#pragma unroll
  for (int ch = 0; ch < kBtChunks; ++ch) {
    const int src = ce[ch] >= 0 ? ce[ch] : 0;
    const uint32_t b = (uint32_t)__shfl((int)base, src, kWave);
    const uint32_t len = (uint32_t)__shfl((int)c.seg_len, src, kWave);
    const uint64_t sb = (uint64_t)__shfl((long long)c.seg_base, src, kWave);
    const uint32_t pos = b + rank[ch];
    if (ce[ch] >= 0 && pos < len) {  // len = the entries the histograms counted: a slot past it is never written
      const uint32_t e = (uint32_t)(ch * kWave + lane);
      okey[sb + pos] = st.hi[e];
      oid[sb + pos] = st.lo[e];
    }
  }
  st.cnt = 0;
}

template <int S>
__device__ __forceinline__ void bt_stage_append(BtStage &st, const BTopkColDev &c, bool take, uint64_t hi, uint32_t lo,
                                                int j, uint64_t *__restrict__ okey, uint32_t *__restrict__ oid,
                                                uint32_t *__restrict__ counters) {
  const unsigned long long m = __ballot(take);
  const uint32_t n = (uint32_t)__popcll(m);
  if (n == 0) return;
  if (st.cnt + n > (uint32_t)kBtStageCap) bt_stage_flush<S>(st, c, okey, oid, counters);
  if (take) {
    const uint32_t slot = st.cnt + (uint32_t)__popcll(m & lanemask_lt());
    st.hi[slot] = hi;
    st.lo[slot] = lo;
    st.col[slot] = (uint8_t)j;
  }
  st.cnt += n;
}

// Appends (rank key, ~ID) of the elements it selects to their column's segment of (okey, oid), in
// any order.  kGe: the elements whose composite key is >= the column's (phi, plo) -- the emit pass;
// otherwise those that agree with the column's prefix on digits 0..p-1 -- the narrowing pass.  The
// loop count is the same for every lane of the grid, so the ballots see whole waves.
template <int S, bool kGe>
__global__ __launch_bounds__(kBtThreads) void k_btopk_collect(const double *__restrict__ R,
                                                              const uint16_t *__restrict__ mask, int64_t n, int p,
                                                              const BTopkColDev *__restrict__ cols,
                                                              uint64_t *__restrict__ okey, uint32_t *__restrict__ oid,
                                                              uint32_t *__restrict__ counters) {
  constexpr int kWaves = kBtThreads / kWave;
  __shared__ uint64_t shi[kWaves * kBtStageCap];
  __shared__ uint32_t slo[kWaves * kBtStageCap];
  __shared__ uint8_t scol[kWaves * kBtStageCap];
  BtStage st{shi + wave_id() * kBtStageCap, slo + wave_id() * kBtStageCap, scol + wave_id() * kBtStageCap, 0u};
  const int j = threadIdx.x % S;
  const BTopkColDev c = cols[j];
  const int64_t stride = (int64_t)gridDim.x * kBtTile;
  for (int64_t base = (int64_t)blockIdx.x * kBtTile; base < n; base += stride) {
    uint64_t hi[kBtUnroll];
    uint32_t lo[kBtUnroll];
    bool ok[kBtUnroll];
    bt_load<S>(R, mask, n, base, j, c.active != 0, hi, lo, ok);
#pragma unroll
    for (int u = 0; u < kBtUnroll; ++u) {
      const bool take =
          ok[u] && (kGe ? topk_ge(hi[u], lo[u], c.phi, c.plo) : topk_match(hi[u], lo[u], c.phi, c.plo, p));
      bt_stage_append<S>(st, c, take, hi[u], lo[u], j, okey, oid, counters);
    }
  }
  bt_stage_flush<S>(st, c, okey, oid, counters);
}

int btopk_scratch(BTopkState **st, int device, int S) {
  if (!*st) {
    BTopkState *t = new (std::nothrow) BTopkState();
    if (!t) return fail(PR_ERR_OOM, "host allocation failed");
    *st = t;
  }
  BTopkState *t = *st;
  if (!t->hist.p) {
    int cus = 0;
    PR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    t->grid_max = std::max(1, cus) * kBtBlocksPerCU;
    PR_TRY(t->cols.alloc(sizeof(BTopkColDev) * kBTopkMaxCols));
    PR_TRY(t->hist.alloc(sizeof(uint32_t) * ((size_t)kTopkDigits * S * kTopkBins + 2 * (size_t)S)));
  }
  return PR_OK;
}

struct BtLaunch {
  BTopkState *t;
  hipStream_t s;
  const double *R;
  const uint16_t *mask;
  int64_t n;  // V * S
  unsigned grid;
};

template <int S>
int launch_hist(const BtLaunch &l, int p, uint32_t *dh) {
  hipLaunchKernelGGL(k_btopk_hist<S>, dim3(l.grid), dim3(kBtThreads), 0, l.s, l.R, l.mask, l.n, p,
                     l.t->cols.as<BTopkColDev>(), dh);
  PR_HIP(hipGetLastError());
  return PR_OK;
}

template <int S>
int launch_collect(const BtLaunch &l, bool ge, int p, uint64_t *okey, uint32_t *oid, uint32_t *counters) {
  if (ge)
    hipLaunchKernelGGL((k_btopk_collect<S, true>), dim3(l.grid), dim3(kBtThreads), 0, l.s, l.R, l.mask, l.n, p,
                       l.t->cols.as<BTopkColDev>(), okey, oid, counters);
  else
    hipLaunchKernelGGL((k_btopk_collect<S, false>), dim3(l.grid), dim3(kBtThreads), 0, l.s, l.R, l.mask, l.n, p,
                       l.t->cols.as<BTopkColDev>(), okey, oid, counters);
  PR_HIP(hipGetLastError());
  return PR_OK;
}

#define PR_BTOPK_DISPATCH(fn, S, ...)          \
  ((S) == 1   ? fn<1>(__VA_ARGS__)             \
   : (S) == 2 ? fn<2>(__VA_ARGS__)             \
   : (S) == 4 ? fn<4>(__VA_ARGS__)             \
   : (S) == 8 ? fn<8>(__VA_ARGS__)             \
              : fn<16>(__VA_ARGS__))

}  // namespace

size_t btopk_state_bytes(const BTopkState *t) {
  if (!t) return 0;
  return t->hist.bytes + t->cols.bytes + t->ckey.bytes + t->cid.bytes + t->out_key.bytes + t->out_id.bytes;
}

void btopk_state_free(BTopkState *t) {
  if (!t) return;
  for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
  delete t;  // DevBufs free their memory
}

int64_t btopk_kernel_ns(const BTopkState *t) { return t ? t->kernel_ns : -1; }

int btopk_select(BTopkState **state, int device, hipStream_t s, const double *R, int64_t V, int width, int stride,
                 const uint16_t *mask, const int64_t *n_excl, int64_t k, int64_t narrow_div, int32_t *ids_out,
                 double *ranks_out, int32_t *n_out, int32_t *info) {
  PR_HIP(hipStreamSynchronize(s));
  const int S = stride;
  int64_t n_sel[kBTopkMaxCols] = {0}, out_base[kBTopkMaxCols + 1] = {0};
  BTopkCol cols[kBTopkMaxCols];
  for (int j = 0; j < width; ++j) {
    const int64_t avail = V - n_excl[j];
    n_sel[j] = std::min<int64_t>(k, avail);
    out_base[j + 1] = out_base[j] + n_sel[j];
    btopk_begin(&cols[j], (uint64_t)n_sel[j], (uint64_t)avail);
  }
  const int64_t total = out_base[width];
  int passes = 0, passes_cand = 0, narrowed_at = -1;
  if (total > 0) {
    if (V >= (int64_t(1) << 31)) return fail(PR_ERR_INVALID, "pr_batch_get_topk_all: V >= 2^31");
    PR_TRY(btopk_scratch(state, device, S));
    BTopkState *t = *state;
    if (t->out_cap < total) {
      t->out_cap = 0;
      PR_TRY(t->out_key.alloc(sizeof(uint64_t) * (size_t)total));
      PR_TRY(t->out_id.alloc(sizeof(uint32_t) * (size_t)total));
      t->out_cap = total;
    }
    const size_t hist_words = (size_t)kTopkDigits * S * kTopkBins;
    uint32_t *hist = t->hist.as<uint32_t>();
    uint32_t *cand_ctr = hist + hist_words, *out_ctr = cand_ctr + S;
    PR_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (hist_words + 2 * (size_t)S), s));
    const int64_t n = V * S;
    const BtLaunch l{t, s, R, mask, n, (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBtTile - 1) / kBtTile, t->grid_max))};
    // every upload has a host copy of its own that lives to the end of the call
    size_t n_marks = 0;
    auto mark = [&]() -> int {  // timed calls: the next event of the pool, recorded on s
      if (!info) return PR_OK;
      if (n_marks == t->ev.size()) {
        hipEvent_t e = nullptr;
        PR_HIP(hipEventCreate(&e));
        t->ev.push_back(e);
      }
      PR_HIP(hipEventRecord(t->ev[n_marks++], s));
      return PR_OK;
    };
    std::deque<std::vector<BTopkColDev>> uploads;
    int64_t seg_base[kBTopkMaxCols] = {0};
    uint32_t seg_len[kBTopkMaxCols] = {0};
    auto upload = [&](const BTopkCol *cs, bool emit) -> int {
      uploads.emplace_back((size_t)kBTopkMaxCols, BTopkColDev{0, 0, 0, 0, 0, 0});
      std::vector<BTopkColDev> &d = uploads.back();
      for (int j = 0; j < width; ++j) {
        d[(size_t)j].phi = cs[j].phi;
        d[(size_t)j].plo = cs[j].plo;
        d[(size_t)j].active = emit ? n_sel[j] > 0 : !cs[j].done;
        d[(size_t)j].seg_base = (uint64_t)(emit ? out_base[j] : seg_base[j]);
        d[(size_t)j].seg_len = emit ? (uint32_t)n_sel[j] : seg_len[j];
      }
      PR_HIP(hipMemcpyAsync(t->cols.p, d.data(), sizeof(BTopkColDev) * kBTopkMaxCols, hipMemcpyHostToDevice, s));
      return PR_OK;
    };
    auto hist_pass = [&](int p, const BTopkCol *cs, uint32_t *h) -> int {
      PR_TRY(upload(cs, false));
      uint32_t *dh = hist + (size_t)p * S * kTopkBins;
      PR_TRY(mark());
      if (narrowed_at >= 0) {
        uint32_t longest = 0;
        for (int j = 0; j < width; ++j)
          if (!cs[j].done) longest = std::max(longest, seg_len[j]);
        const unsigned gx = (unsigned)std::max<int64_t>(
            1, std::min<int64_t>(((int64_t)longest + kBtThreads - 1) / kBtThreads, std::max(1, t->grid_max / S)));
        hipLaunchKernelGGL(k_btopk_hist_cand, dim3(gx, (unsigned)width), dim3(kBtThreads), 0, s, t->ckey.as<uint64_t>(),
                           t->cid.as<uint32_t>(), p, t->cols.as<BTopkColDev>(), dh);
        PR_HIP(hipGetLastError());
        ++passes_cand;
      } else {
        PR_TRY(PR_BTOPK_DISPATCH(launch_hist, S, l, p, dh));
      }
      PR_TRY(mark());
      PR_HIP(hipMemcpyAsync(h, dh, sizeof(uint32_t) * (size_t)S * kTopkBins, hipMemcpyDeviceToHost, s));
      PR_HIP(hipStreamSynchronize(s));
      return PR_OK;
    };
    auto narrow = [&](int p, const BTopkCol *cs, uint64_t count) -> int {
      if (t->cand_cap < (int64_t)count) {
        t->cand_cap = 0;
        PR_TRY(t->ckey.alloc(sizeof(uint64_t) * (size_t)count));
        PR_TRY(t->cid.alloc(sizeof(uint32_t) * (size_t)count));
        t->cand_cap = (int64_t)count;
      }
      int64_t at = 0;
      for (int j = 0; j < width; ++j) {
        seg_base[j] = at;
        seg_len[j] = cs[j].done ? 0u : (uint32_t)cs[j].cand;
        at += seg_len[j];
      }
      PR_TRY(upload(cs, false));
      PR_TRY(mark());
      PR_TRY(PR_BTOPK_DISPATCH(launch_collect, S, l, false, p, t->ckey.as<uint64_t>(), t->cid.as<uint32_t>(), cand_ctr));
      PR_TRY(mark());
      narrowed_at = p;
      return PR_OK;
    };
    int drv_passes = 0, drv_narrowed = -1;
    PR_TRY(btopk_select_thresholds(width, cols, btopk_narrow_limit(V, width, narrow_div), hist_pass, narrow, &drv_passes,
                                   &drv_narrowed));
    passes = drv_passes;
    PR_TRY(upload(cols, true));
    PR_TRY(mark());
    PR_TRY(PR_BTOPK_DISPATCH(launch_collect, S, l, true, 0, t->out_key.as<uint64_t>(), t->out_id.as<uint32_t>(), out_ctr));
    PR_TRY(mark());
    uint32_t counts[kBTopkMaxCols] = {0};
    std::vector<uint32_t> hid((size_t)total);
    std::vector<uint64_t> hkey((size_t)total);
    PR_HIP(hipMemcpyAsync(counts, out_ctr, sizeof(uint32_t) * (size_t)S, hipMemcpyDeviceToHost, s));
    PR_HIP(hipMemcpyAsync(hid.data(), t->out_id.p, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
    PR_HIP(hipMemcpyAsync(hkey.data(), t->out_key.p, sizeof(uint64_t) * (size_t)total, hipMemcpyDeviceToHost, s));
    PR_HIP(hipStreamSynchronize(s));
    if (info) {
      double ms_sum = 0.0;
      for (size_t i = 0; i + 1 < n_marks; i += 2) {
        float ms = 0.f;
        PR_HIP(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
        ms_sum += ms;
      }
      t->kernel_ns = (int64_t)(ms_sum * 1e6);
    }
    for (int j = 0; j < width; ++j)
      if ((int64_t)counts[j] != n_sel[j])
        return fail(PR_ERR_HIP, "pr_batch_get_topk_all: column " + std::to_string(j) + " selected " +
                                    std::to_string(counts[j]) + " of " + std::to_string(n_sel[j]) + " pairs");
    std::vector<TopkPair> v;
    for (int j = 0; j < width; ++j) {
      v.resize((size_t)n_sel[j]);
      for (int64_t i = 0; i < n_sel[j]; ++i)
        v[(size_t)i] = {hkey[(size_t)(out_base[j] + i)], (int32_t)~hid[(size_t)(out_base[j] + i)]};
      topk_sort_pairs(&v);
      for (int64_t i = 0; i < n_sel[j]; ++i) {
        ids_out[(int64_t)j * k + i] = v[(size_t)i].id;
        const uint64_t bits = topk_rank_bits(v[(size_t)i].key);
        std::memcpy(&ranks_out[(int64_t)j * k + i], &bits, sizeof(bits));
      }
    }
  }
  for (int j = 0; j < width; ++j) n_out[j] = (int32_t)n_sel[j];
  if (info) {
    info[0] = passes;
    info[1] = passes - passes_cand;
    info[2] = passes_cand;
    info[3] = narrowed_at;
  }
  return PR_OK;
}

}  // namespace pr
