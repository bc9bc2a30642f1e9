// Batched personalised PageRank for gfx950 (pr_batch_*; planner arithmetic in pr_batch.h): up to
// 16 rank vectors advance together over the graph's canonical CSR (original IDs), so the column
// indices are streamed once for all of them and every gather fetches 8 * stride contiguous bytes.
//
// Storage: R (ranks), T (teleport terms) and two C buffers (contributions c = r / out_deg,
// double-buffered) are V x stride doubles, element (v, j) at v * stride + j; stride = the next
// power of two >= width.  Padding columns hold zeros and stay zero; no result reads them.
//
// One iteration is three launches on the batch's stream, with no host sync in between:
//   k_batch_units     one wave per work unit (pr_batch.h): lane = g * stride + j, the 64 / stride
//                     groups each take one in-link per step -- a group's lanes share one canon_col
//                     load and read C[col * stride + j] -- and the group sums are combined by a
//                     fixed butterfly; rows of at most kBatchShortRow in-links are taken one
//                     group per row, G rows at a time, instead.  A PACK unit keeps its rows' sums in LDS and then updates
//                     rows x stride elements with all 64 lanes (affine update, c' = r' / out_deg,
//                     per-column dangling and L1 partials); a CHUNK unit stores its partial sum.
//   k_batch_long      adds the chunk partials of every long row in chunk order and updates it.
//   k_batch_finalize  reduces the per-workgroup partials in fixed order into dc[0..stride) and
//                     l1[0..stride) in device memory, where the next iteration reads dc.
// Units are dealt to the waves of a fixed grid (unit u -> wave u % grid), so every sum -- a row's,
// a column's dangling mass -- has an order that depends on the graph and the stride only.  No
// floating-point atomics anywhere.
//
// The unit and the long-row kernel are each written once, as a body (units_body, long_body) with two
// template switches, UNTIL and TD; the __global__ templates named here are the body's forms and hold
// no code of their own, and launch_iteration picks the form.
//
// pr_batch_step_until runs the iteration in its UNTIL form (k_batch_units_until, k_batch_long_until)
// and through k_batch_finalize_until, which read an active mask (pr_batch_until.h) from device
// memory.  A column whose bit is clear is frozen: its lanes still take part in every row sum, shuffle
// and barrier, but store no rank, no L1 and no new dangling sum; instead they copy their
// contributions cin -> cout and the finalize step copies dc_in -> dc_out, so that both double
// buffers stay valid whatever the parity of the iteration the column stopped at.  A fourth,
// one-thread launch (k_batch_decide) runs after the finalize step, counts the iteration for the
// active columns and clears the bits of those whose L1 is within tol; no kernel of an iteration can
// therefore see that iteration's own decision.  With an empty mask every kernel returns at entry.
// pr_batch_step launches none of these.
//
// pr_batch_run_queue (scheduler: pr_batch_queue.h) refills columns one at a time: k_batch_set_col and
// k_batch_scatter_col write a sparse teleport vector into T on the device, k_batch_reset_col and
// k_batch_finalize_col restart one column in k_batch_reset's order of summation, and
// pr_batch_step_until_any runs the *_until kernels under the mask of the occupied columns with
// k_batch_decide_any in k_batch_decide's place, which empties the mask after the first iteration in
// which a column converged.
//
// pr_batch_set_dangling(PR_BATCH_DANGLING_TELEPORT) replaces the unit and long-row kernels of all of
// the above by their TD forms, k_batch_units_td / k_batch_long_td, which return column j's dangling
// mass along its teleport vector (q_j * t[p], q_j = dc_j / ts_j) where ts_j -- the vector's sum,
// formed by k_batch_tsum_col in k_batch_reset_col's order whenever a vector changed -- is finite and
// not 0, and add the uniform dc_j / N otherwise (pr_batch_dangling.h).  In the default mode none of
// these runs.
//
// The batch only reads the graph's canon_* buffers; it launches none of the graph's kernels and
// owns its stream and all its state.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "pr_batch.h"
#include "pr_batch_dangling.h"
#include "pr_batch_topk.h"
#include "pr_batch_queue.h"
#include "pr_batch_until.h"
#include "pr_device.h"
#include "pr_graph.h"

struct pr_batch {
  pr_graph *g = nullptr;  // borrowed: destroy the batch first
  int device = 0;
  hipStream_t stream = nullptr;
  int width = 0, stride = 0;
  int32_t V = 0;
  bool dangling_none = false;
  int64_t n_units = 0, n_long = 0, n_slots = 0;
  int ugrid = 1, lgrid = 0;  // workgroups of k_batch_units / k_batch_long
  pr::DevBuf units, long_row, long_p0, chunk_part;
  pr::DevBuf R, T, C[2];
  pr::DevBuf dc[2], l1;  // stride doubles each; dc[cur] is what the next iteration reads
  pr::DevBuf part;       // per workgroup: stride dangling partials, then stride L1 partials
  // pr_batch_step_until: the device's BatchUntilState, and per column the dc its last applied
  // iteration of the call used (stride doubles; pr_batch_get_norms reads it while until_norms is set)
  pr::DevBuf until, dcu;
  pr::BatchUntilState h_until{};
  pr::BatchQueueState h_queue{};
  bool until_norms = false;
  pr::DevBuf colbuf;     // V doubles: one column, extracted (ranks, top-K) or on its way into T
  pr::TopkState *topk = nullptr;
  // per-column exclusions of the top-K queries (pr_batch_set_exclude): bit j of mask[v] leaves vertex
  // v out of column j.  Allocated with the first non-empty set; h_mask is the host's copy.
  pr::DevBuf excl_mask;  // uint16_t[V]
  pr::DevBuf excl_oid;   // int32_t[V]: the single-column query's ID array (-1 = excluded), on first need
  std::vector<uint16_t> h_mask;
  int64_t n_excl[pr::kBatchMaxWidth] = {0};
  pr::BTopkState *btopk = nullptr;  // scratch of pr_batch_get_topk_all
  // pr_batch_mix_topk / pr_batch_mix_get (pr_batch_mix.hip): the blend matrix, the per-mix exclusion
  // mask and a select scratch of their own, from the first mix call on
  pr::BatchMixState *mix = nullptr;
  // pr_batch_step_until_any / pr_batch_run_queue: the device's BatchQueueState; a query's seed IDs
  // and values on their way into T (grown on demand); the queue's init_ranks (V doubles, on first
  // need: colbuf is taken by the queries of the done callback)
  pr::DevBuf qstate, qids, qvals, qinit;
  std::vector<int32_t> excl_ids[pr::kBatchMaxWidth];  // the IDs behind n_excl, to clear a set in O(n)
  bool in_done_cb = false;  // pr_batch_run_queue is inside its callback: only the three getters run
  uint32_t vec_mask = 0;  // columns with a teleport vector set
  // pr_batch_set_dangling: the mode; ts (stride doubles, allocated with the first use of teleport mode
  // or of pr_batch_get_teleport_sums) holds the sums of the columns' teleport vectors, 0 without one;
  // bit j of ts_dirty: column j's vector changed since ts[j] was formed
  int32_t dangling_mode = PR_BATCH_DANGLING_UNIFORM;
  pr::DevBuf ts;
  uint32_t ts_dirty = 0;
  double teleport = 0.15, damping = 0.85;
  int cur = 0;
  int64_t iters_done = 0;
  bool ready = false;
  // HIP events around the iterations of the last pr_batch_step call (pr_batch_info reports the time)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;

  size_t device_bytes() const {
    return units.bytes + long_row.bytes + long_p0.bytes + chunk_part.bytes + R.bytes + T.bytes + C[0].bytes +
           C[1].bytes + dc[0].bytes + dc[1].bytes + l1.bytes + part.bytes + colbuf.bytes + pr::topk_state_bytes(topk) +
           until.bytes + dcu.bytes + excl_mask.bytes + excl_oid.bytes + pr::btopk_state_bytes(btopk) + qstate.bytes +
           qids.bytes + qvals.bytes + qinit.bytes + ts.bytes + pr::batch_mix_bytes(mix);
  }
};

namespace pr {
namespace {

constexpr const char *kInDoneCb =
    "inside pr_batch_run_queue's callback only pr_batch_get_ranks, pr_batch_get_topk and pr_batch_get_norms may be called";
static_assert(kBTopkMaxCols == kBatchMaxWidth, "the batch top-K handles every column of a batch");
constexpr int kBatchGridMax = 8192;  // waves of k_batch_units (a constant: sums must not depend on the device)
constexpr int kBatchThreads = 256;   // the element-wise kernels

struct BatchArgs {
  const BatchUnit *units;
  int64_t n_units;
  const int64_t *rowptr;
  const int32_t *col, *deg;
  const uint8_t *vflags;
  const double *cin;
  double *cout, *r;
  const double *t, *dc;
  double *chunk_part, *part;
  double n_vertices, damping;
  int dangling_none;
};

__device__ __forceinline__ double batch_affine(double S, double tdc, double teleport, double damping) {
  return __dadd_rn(teleport, __dmul_rn(damping, __dadd_rn(S, tdc)));
}

// Butterfly over the lane groups of a wave: every lane ends with the sum over the lanes that share
// its column, combined in one fixed order.
template <int S>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
  for (int off = S; off < kWave; off <<= 1) x = __dadd_rn(x, __shfl_xor(x, off, kWave));
  return x;
}

// Column j's sum over in-links [b, e): group g adds b + g, b + g + G, ... in that order (four
// gathers in flight at a time), then the groups are combined.  Valid in every lane.
template <int S>
__device__ __forceinline__ double row_sum(const int32_t *__restrict__ col, const double *__restrict__ cin, int64_t b,
                                          int64_t e, int g, int j) {
  constexpr int G = kWave / S;
  double acc = 0.0;
  int64_t i = b + g;
  for (; i + 3 * G < e; i += 4 * G) {
    const int32_t c0 = col[i], c1 = col[i + G], c2 = col[i + 2 * G], c3 = col[i + 3 * G];
    const double x0 = cin[(int64_t)c0 * S + j], x1 = cin[(int64_t)c1 * S + j];
    const double x2 = cin[(int64_t)c2 * S + j], x3 = cin[(int64_t)c3 * S + j];
    acc = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(acc, x0), x1), x2), x3);
  }
  for (; i < e; i += G) acc = __dadd_rn(acc, cin[(int64_t)col[i] * S + j]);
  return group_sum<S>(acc);
}

// What a lane adds to its in-link sums for column j's dangling mass, formed once at entry from
// dc = dc_j and, in the teleport form, ts = ts_j (ts[0..S) holds the sums of the columns' teleport
// vectors: k_batch_tsum_col; 0 for a column without one and for padding).  Uniform form
// (TD == false): q = dc_j / N, added as it is.  Teleport form: the lane picks, as a select, its
// factor q = dc_j / ts_j (use: an element adds q * t[p]) or the uniform term (pr_batch_dangling.h).
// Nothing that shuffles or waits depends on the pick.
struct LaneTerm {
  bool use;
  double q;
};
template <bool TD>
__device__ __forceinline__ LaneTerm lane_term(double dc, double n_vertices, double ts) {
  const bool use = TD && batch_dangling_uses_teleport(ts);
  return {use, TD ? batch_dangling_factor(use, dc, ts, n_vertices) : dc / n_vertices};
}

// Element (v, j) of a row whose in-link sum is Sv: the update, the new contribution and the
// column's dangling / L1 partials.  Under an active mask (UNTIL) an element of a frozen column
// (act == false) only carries its contribution over to the buffer the next iteration reads (d == 0
// elements are 0 in both buffers).
template <bool UNTIL, bool TD>
__device__ __forceinline__ void update_elem(const BatchArgs &a, int64_t v, int64_t p, double Sv, double rold,
                                            uint32_t f, LaneTerm lt, bool act, double &dcp, double &l1p) {
  if (!UNTIL || act) {
    const double tp = a.t[p];
    const double rn = batch_affine(Sv, TD && lt.use ? batch_dangling_term(lt.q, tp) : lt.q, tp, a.damping);
    a.r[p] = rn;
    const int32_t d = a.deg[v];
    if (d > 0) a.cout[p] = __ddiv_rn(rn, (double)d);
    else if ((f & PR_VF_SINK) && !a.dangling_none) dcp = __dadd_rn(dcp, rn);
    l1p = __dadd_rn(l1p, fabs(rn - rold));
  } else if (a.deg[v] > 0) {
    a.cout[p] = a.cin[p];
  }
}

// The body of the unit kernels below.  UNTIL: the iteration runs under the active mask of `us`
// (pr_batch_until.h), one word that is the same for every lane, so an empty mask is a uniform exit --
// the only early one; everything that shuffles or waits at a barrier runs for frozen columns too.
// TD: the teleport form of the dangling term (lane_term).  `a` comes by value, as a kernel holds it:
// by reference the compiler splits the kernel-argument loads of the prologue and waits for them
// twice (profiles/batch_refactor/).
template <int S, bool UNTIL, bool TD>
__device__ __forceinline__ void units_body(BatchArgs a, const double *__restrict__ ts,
                                           const BatchUntilState *__restrict__ us) {
  constexpr int G = kWave / S;
  __shared__ double sS[kBatchUnitRows * S];
  uint32_t m = 0xffffffffu;
  if (UNTIL) {
    m = us->mask;
    if (m == 0) return;
  }
  const int lane = threadIdx.x, g = lane / S, j = lane % S;
  const bool act = (m >> j) & 1u;
  const LaneTerm lt = lane_term<TD>(a.dc[j], a.n_vertices, TD ? ts[j] : 0.0);
  double dcp = 0.0, l1p = 0.0;
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const BatchUnit un = a.units[u];
    if (un.rows < 0) {  // CHUNK: the partial sum of one piece of a long row
      const double acc = row_sum<S>(a.col, a.cin, un.e0, un.e0 + un.n, g, j);
      if (lane < S) a.chunk_part[(int64_t)un.slot * S + j] = acc;
      continue;
    }
    const int rows = un.rows;  // <= kBatchUnitRows = 64: lane k holds row k's first in-link
    const long long rp_l = (long long)a.rowptr[(int64_t)un.row0 + (lane < rows ? lane : rows)];
    const int64_t uend = un.e0 + un.n;
    // short rows (1 .. kBatchShortRow in-links): one lane group per row, G rows at a time; all the
    // row's gathers are in flight at once and are added in in-link order
    for (int k0 = 0; k0 < rows; k0 += G) {
      const int k = k0 + g;
      const int ks = k < rows ? k : 0;
      const int64_t b = __shfl(rp_l, ks, kWave);
      const int64_t e1 = __shfl(rp_l, ks + 1 < kWave ? ks + 1 : kWave - 1, kWave);
      const int64_t deg = k < rows ? (ks + 1 < rows ? e1 : uend) - b : 0;
      if (deg > 0 && deg <= kBatchShortRow) {
        int32_t c[kBatchShortRow];
        double x[kBatchShortRow];
#pragma unroll
        for (int q = 0; q < kBatchShortRow; ++q) c[q] = q < deg ? a.col[b + q] : 0;
#pragma unroll
        for (int q = 0; q < kBatchShortRow; ++q) x[q] = q < deg ? a.cin[(int64_t)c[q] * S + j] : 0.0;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < kBatchShortRow; ++q)
          if (q < deg) acc = __dadd_rn(acc, x[q]);
        sS[k * S + j] = acc;
      }
    }
    // longer rows: the whole wave per row
    for (int k = 0; k < rows; ++k) {
      const int64_t b = __shfl(rp_l, k, kWave);
      const int64_t e = k + 1 < rows ? (int64_t)__shfl(rp_l, k + 1, kWave) : uend;
      if (e - b <= kBatchShortRow) continue;  // done above, or empty: the update takes the old rank
      const double acc = row_sum<S>(a.col, a.cin, b, e, g, j);
      if (lane < S) sS[k * S + j] = acc;
    }
    __syncthreads();
    const int total = rows * S;
    for (int idx = lane; idx < total; idx += kWave) {  // idx % S == j: 64 is a multiple of S
      const int64_t v = (int64_t)un.row0 + idx / S, p = v * S + j;
      const uint32_t f = a.vflags[v];
      const double rold = a.r[p];
      update_elem<UNTIL, TD>(a, v, p, (f & PR_VF_INDEG0) ? rold : sS[idx], rold, f, lt, act, dcp, l1p);
    }
    __syncthreads();
  }
  dcp = group_sum<S>(dcp);
  l1p = group_sum<S>(l1p);
  if (lane < S) {  // a frozen column's partials are zeros that k_batch_finalize_until never reads
    a.part[((int64_t)blockIdx.x * 2) * S + j] = dcp;
    a.part[((int64_t)blockIdx.x * 2 + 1) * S + j] = l1p;
  }
}

// Per-column sums of a workgroup's (dcp, l1p) in thread order (thread t holds column t % S), stored
// as workgroup `blk` of part.
template <int S>
__device__ __forceinline__ void block_col_part(double dcp, double l1p, double *__restrict__ part, int64_t blk) {
  __shared__ double sh[2][kBatchThreads];
  const int t = threadIdx.x;
  sh[0][t] = dcp;
  sh[1][t] = l1p;
  __syncthreads();
  if (t < S) {
    double x = 0.0, y = 0.0;
    for (int k = t; k < kBatchThreads; k += S) {
      x = __dadd_rn(x, sh[0][k]);
      y = __dadd_rn(y, sh[1][k]);
    }
    part[(blk * 2) * S + t] = x;
    part[(blk * 2 + 1) * S + t] = y;
  }
}

// The body of the long-row kernels below.  One thread per (long row, column): the row's chunk
// partials in chunk order, then the update.  UNTIL and TD as in units_body; the empty mask's exit is
// uniform and comes before the barrier of block_col_part.
template <int S, bool UNTIL, bool TD>
__device__ __forceinline__ void long_body(const BatchArgs &a, const int32_t *__restrict__ long_row,
                                          const int32_t *__restrict__ long_p0, int64_t n_long, int64_t part_block0,
                                          const double *__restrict__ ts, const BatchUntilState *__restrict__ us) {
  uint32_t m = 0xffffffffu;
  if (UNTIL) {
    m = us->mask;
    if (m == 0) return;
  }
  const int64_t idx = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
  const int64_t q = idx / S;
  const int j = threadIdx.x % S;
  double dcp = 0.0, l1p = 0.0;
  if (q < n_long) {
    const int32_t p0 = long_p0[q], p1 = long_p0[q + 1];
    double acc = 0.0;
    for (int32_t k = p0; k < p1; ++k) acc = __dadd_rn(acc, a.chunk_part[(int64_t)k * S + j]);
    const int64_t v = long_row[q], p = v * S + j;
    const double rold = a.r[p];
    const uint32_t f = a.vflags[v];
    const LaneTerm lt = lane_term<TD>(a.dc[j], a.n_vertices, TD ? ts[j] : 0.0);
    update_elem<UNTIL, TD>(a, v, p, acc, rold, f, lt, (m >> j) & 1u, dcp, l1p);
  }
  block_col_part<S>(dcp, l1p, a.part, part_block0 + blockIdx.x);
}

// The kernels of an iteration, one pair per form: plain (pr_batch_step), _until (under the active
// mask), _td (PR_BATCH_DANGLING_TELEPORT; UNTIL selects the masked form, so the two templates stand
// for four kernels).  Each is its body with the form's template arguments and nothing else.
template <int S>
__global__ __launch_bounds__(kWave) void k_batch_units(BatchArgs a) {
  units_body<S, false, false>(a, nullptr, nullptr);
}
template <int S>
__global__ __launch_bounds__(kWave) void k_batch_units_until(BatchArgs a, const BatchUntilState *__restrict__ us) {
  units_body<S, true, false>(a, nullptr, us);
}
template <int S, bool UNTIL>
__global__ __launch_bounds__(kWave) void k_batch_units_td(BatchArgs a, const double *__restrict__ ts,
                                                          const BatchUntilState *__restrict__ us) {
  units_body<S, UNTIL, true>(a, ts, us);
}
template <int S>
__global__ __launch_bounds__(kBatchThreads) void k_batch_long(BatchArgs a, const int32_t *__restrict__ long_row,
                                                              const int32_t *__restrict__ long_p0, int64_t n_long,
                                                              int64_t part_block0) {
  long_body<S, false, false>(a, long_row, long_p0, n_long, part_block0, nullptr, nullptr);
}
template <int S>
__global__ __launch_bounds__(kBatchThreads) void k_batch_long_until(BatchArgs a, const int32_t *__restrict__ long_row,
                                                                    const int32_t *__restrict__ long_p0, int64_t n_long,
                                                                    int64_t part_block0,
                                                                    const BatchUntilState *__restrict__ us) {
  long_body<S, true, false>(a, long_row, long_p0, n_long, part_block0, nullptr, us);
}
template <int S, bool UNTIL>
__global__ __launch_bounds__(kBatchThreads) void k_batch_long_td(BatchArgs a, const int32_t *__restrict__ long_row,
                                                                 const int32_t *__restrict__ long_p0, int64_t n_long,
                                                                 int64_t part_block0, const double *__restrict__ ts,
                                                                 const BatchUntilState *__restrict__ us) {
  long_body<S, UNTIL, true>(a, long_row, long_p0, n_long, part_block0, ts, us);
}

// Workgroup kind * S + j: column j's dangling (kind 0) or L1 (kind 1) partials of n_blocks
// workgroups, in fixed order.
__global__ __launch_bounds__(kBatchThreads) void k_batch_finalize(const double *__restrict__ part, int64_t n_blocks,
                                                                  int S, double *__restrict__ dc_out,
                                                                  double *__restrict__ l1_out) {
  __shared__ double red[kBatchThreads / kWave];
  const int kind = blockIdx.x / S, j = blockIdx.x % S;
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += kBatchThreads) acc = __dadd_rn(acc, part[(b * 2 + kind) * S + j]);
  acc = block_sum<kBatchThreads>(acc, red);
  if (threadIdx.x == 0) (kind ? l1_out : dc_out)[j] = acc;
}

// k_batch_finalize under an active mask.  An active column also records the dc this iteration used
// (dcu); a frozen one -- padding columns are never in the mask -- keeps its L1 and carries its
// next-iteration dc across the swap.  The mask is only read here: k_batch_decide changes it.
__global__ __launch_bounds__(kBatchThreads) void k_batch_finalize_until(const double *__restrict__ part, int64_t n_blocks,
                                                                        int S, const double *__restrict__ dc_in,
                                                                        double *__restrict__ dc_out,
                                                                        double *__restrict__ l1_out,
                                                                        double *__restrict__ dcu,
                                                                        const BatchUntilState *__restrict__ us) {
  __shared__ double red[kBatchThreads / kWave];
  const uint32_t m = us->mask;
  if (m == 0) return;
  const int kind = blockIdx.x / S, j = blockIdx.x % S;
  if (!((m >> j) & 1u)) {  // the whole workgroup: no barrier is skipped by a part of it
    if (kind == 0 && threadIdx.x == 0) dc_out[j] = dc_in[j];
    return;
  }
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += kBatchThreads) acc = __dadd_rn(acc, part[(b * 2 + kind) * S + j]);
  acc = block_sum<kBatchThreads>(acc, red);
  if (threadIdx.x == 0) {
    if (kind) {
      l1_out[j] = acc;
    } else {
      dc_out[j] = acc;
      dcu[j] = dc_in[j];
    }
  }
}

// One thread, after both workgroups of every column have finished: the iteration counts for the
// columns it advanced, and the mask the next iteration runs under.
__global__ __launch_bounds__(kWave) void k_batch_decide(BatchUntilState *__restrict__ us, const double *__restrict__ l1,
                                                        double tol, int width) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t m = us->mask;
  if (m == 0) return;
  for (int j = 0; j < width; ++j)
    if ((m >> j) & 1u) ++us->iters[j];
  ++us->executed;
  us->mask = batch_until_decide(m, l1, tol, width);
}

// k_batch_decide for pr_batch_step_until_any: the same counting, but the mask only ever changes to 0
// -- after the first iteration in which an active column converged (batch_any_decide), so that the
// remaining launches of the block return at entry.
__global__ __launch_bounds__(kWave) void k_batch_decide_any(BatchUntilState *__restrict__ us,
                                                            BatchQueueState *__restrict__ qs,
                                                            const double *__restrict__ l1, double tol, int width) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t m = us->mask;
  if (m == 0) return;
  for (int j = 0; j < width; ++j)
    if ((m >> j) & 1u) ++us->iters[j];
  ++us->executed;
  us->mask = batch_any_decide(m, l1, tol, width, qs);
}

// The first half of a one-column sum (k_batch_tsum_col, k_batch_reset_col): the values x of the
// workgroup's threads of column j (threadIdx.x % S == j), added in thread order -- block_col_part's
// order for that column -- into part1[blockIdx.x].  part1 is a dense array of its own shape in the
// part scratch: every launch that uses the scratch is on the batch's stream, so they take turns.
template <int S>
__device__ __forceinline__ void block_one_col_part(double x, int j, double *__restrict__ part1) {
  __shared__ double sh[kBatchThreads];
  sh[threadIdx.x] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = j; k < kBatchThreads; k += S) s = __dadd_rn(s, sh[k]);
    part1[blockIdx.x] = s;
  }
}

// The second half, in one workgroup (k_batch_tsum_finalize, k_batch_finalize_col): k_batch_finalize's
// strided sums over part1[0..n_blocks) and the same block_sum.
__device__ __forceinline__ double one_col_total(const double *__restrict__ part1, int64_t n_blocks) {
  __shared__ double red[kBatchThreads / kWave];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += kBatchThreads) acc = __dadd_rn(acc, part1[b]);
  return block_sum<kBatchThreads>(acc, red);
}

// The sum of column j of T for teleport mode, in k_batch_reset_col's traversal (launched with
// k_batch_reset's grid): the threads with threadIdx.x % S == j add the elements they visit there, in
// that order.  The order depends on V and S only, not on j: thread S * m + j of workgroup b visits
// the vertices thread S * m of it would.
template <int S>
__global__ __launch_bounds__(kBatchThreads) void k_batch_tsum_col(int64_t V, int j, const double *__restrict__ t,
                                                                  double *__restrict__ part1) {
  const int tx = threadIdx.x;
  double acc = 0.0;
  if (tx % S == j)
    for (int64_t p = (int64_t)blockIdx.x * kBatchThreads + tx; p < V * S; p += (int64_t)gridDim.x * kBatchThreads)
      acc = __dadd_rn(acc, t[p]);
  block_one_col_part<S>(acc, j, part1);
}

__global__ __launch_bounds__(kBatchThreads) void k_batch_tsum_finalize(const double *__restrict__ part1, int64_t n_blocks,
                                                                       int j, double *__restrict__ ts) {
  const double acc = one_col_total(part1, n_blocks);
  if (threadIdx.x == 0) ts[j] = acc;
}

// Ranks to init (or 1.0) in every column, the scalar teleport into the columns without a vector,
// the contributions of those ranks, zeros into the padding columns; per-workgroup dangling partials.
// gridDim.x * kBatchThreads is a multiple of S, so a thread stays in column threadIdx.x % S.
template <int S>
__global__ __launch_bounds__(kBatchThreads) void k_batch_reset(int64_t V, int width, const double *__restrict__ init,
                                                               uint32_t vec_mask, double teleport,
                                                               const int32_t *__restrict__ deg,
                                                               const uint8_t *__restrict__ vflags, int dangling_none,
                                                               double *__restrict__ r, double *__restrict__ t,
                                                               double *__restrict__ c0, double *__restrict__ c1,
                                                               double *__restrict__ part) {
  const int j = threadIdx.x % S;
  double dcp = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; p < V * S; p += (int64_t)gridDim.x * kBatchThreads) {
    const int64_t v = p / S;
    const double x = j < width ? (init ? init[v] : 1.0) : 0.0;
    r[p] = x;
    if (!((vec_mask >> j) & 1u)) t[p] = j < width ? teleport : 0.0;
    const int32_t d = deg[v];
    c0[p] = d > 0 ? __ddiv_rn(x, (double)d) : 0.0;
    c1[p] = 0.0;
    if (d == 0 && (vflags[v] & PR_VF_SINK) && !dangling_none) dcp = __dadd_rn(dcp, x);
  }
  block_col_part<S>(dcp, 0.0, part, blockIdx.x);
}

// k_batch_reset for column j alone, launched with k_batch_reset's grid: the threads of column j
// (threadIdx.x % S == j) visit the elements they visit there, in the same order, so a thread's
// dangling partial has the same bits; the others only wait at the barrier.  T stays as it is.  Both
// contribution buffers get the new contributions (the column may be frozen in the next iteration,
// which copies cin -> cout only where out_deg > 0).  The workgroup's sum goes to part1[blockIdx.x],
// in the part scratch, which no iteration is using (the caller has waited for the stream).
template <int S>
__global__ __launch_bounds__(kBatchThreads) void k_batch_reset_col(int64_t V, int j, const double *__restrict__ init,
                                                                   const int32_t *__restrict__ deg,
                                                                   const uint8_t *__restrict__ vflags, int dangling_none,
                                                                   double *__restrict__ r, double *__restrict__ c0,
                                                                   double *__restrict__ c1, double *__restrict__ part1) {
  const int t = threadIdx.x;
  double dcp = 0.0;
  if (t % S == j)
    for (int64_t p = (int64_t)blockIdx.x * kBatchThreads + t; p < V * S; p += (int64_t)gridDim.x * kBatchThreads) {
      const int64_t v = p / S;
      const double x = init ? init[v] : 1.0;
      r[p] = x;
      const int32_t d = deg[v];
      const double c = d > 0 ? __ddiv_rn(x, (double)d) : 0.0;
      c0[p] = c;
      c1[p] = c;
      if (d == 0 && (vflags[v] & PR_VF_SINK) && !dangling_none) dcp = __dadd_rn(dcp, x);
    }
  block_one_col_part<S>(dcp, j, part1);
}

// k_batch_finalize's dangling workgroup for one column over part1.  The sum goes to both dc buffers
// (either may be read next, and a frozen column copies one to the other) and to dcu, so that
// pr_batch_get_norms finds it whatever advanced the batch last; the column's L1 is the 0 that
// k_batch_finalize sums after a reset.
__global__ __launch_bounds__(kBatchThreads) void k_batch_finalize_col(const double *__restrict__ part1, int64_t n_blocks,
                                                                      int j, double *__restrict__ dc0,
                                                                      double *__restrict__ dc1, double *__restrict__ dcu,
                                                                      double *__restrict__ l1) {
  const double acc = one_col_total(part1, n_blocks);
  if (threadIdx.x == 0) {
    dc0[j] = acc;
    dc1[j] = acc;
    dcu[j] = acc;
    l1[j] = 0.0;
  }
}

// m[ids[i] * S + j] = values[i]: the seeds of a sparse teleport vector, after k_batch_set_col has
// written `rest` everywhere.  The host has checked that the IDs are distinct and inside [0, V).
__global__ __launch_bounds__(kBatchThreads) void k_batch_scatter_col(int32_t n, int S, int j,
                                                                     const int32_t *__restrict__ ids,
                                                                     const double *__restrict__ values,
                                                                     double *__restrict__ m) {
  for (int64_t i = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBatchThreads)
    m[(int64_t)ids[i] * S + j] = values[i];
}

// Column j of m (V x S) from / to V contiguous doubles.
__global__ __launch_bounds__(kBatchThreads) void k_batch_extract(int64_t V, int S, int j, const double *__restrict__ m,
                                                                 double *__restrict__ out) {
  for (int64_t v = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBatchThreads)
    out[v] = m[v * S + j];
}
// k_batch_extract that also writes the column's ID array for topk_select: v, or -1 where bit j of
// mask[v] leaves v out of the column.
__global__ __launch_bounds__(kBatchThreads) void k_batch_extract_excl(int64_t V, int S, int j,
                                                                      const double *__restrict__ m,
                                                                      const uint16_t *__restrict__ mask,
                                                                      double *__restrict__ out, int32_t *__restrict__ oid) {
  for (int64_t v = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBatchThreads) {
    out[v] = m[v * S + j];
    oid[v] = ((mask[v] >> j) & 1u) ? -1 : (int32_t)v;
  }
}
__global__ __launch_bounds__(kBatchThreads) void k_batch_set_col(int64_t V, int S, int j, const double *__restrict__ in,
                                                                 double value, double *__restrict__ m) {
  for (int64_t v = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBatchThreads)
    m[v * S + j] = in ? in[v] : value;
}

struct BatchDeviceGuard {
  int prev = -1;
  explicit BatchDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~BatchDeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// The iteration that reads the buffers of parity `cur`.
BatchArgs batch_args(const pr_batch *b, int cur) {
  const pr_graph *g = b->g;
  BatchArgs a{};
  a.units = b->units.as<BatchUnit>();
  a.n_units = b->n_units;
  a.rowptr = g->canon_rowptr.as<int64_t>();
  a.col = g->canon_col.as<int32_t>();
  a.deg = g->canon_deg.as<int32_t>();
  a.vflags = g->canon_vflags.as<uint8_t>();
  a.cin = b->C[cur].as<double>();
  a.cout = b->C[cur ^ 1].as<double>();
  a.r = b->R.as<double>();
  a.t = b->T.as<double>();
  a.dc = b->dc[cur].as<double>();
  a.chunk_part = b->chunk_part.as<double>();
  a.part = b->part.as<double>();
  a.n_vertices = (double)b->V;
  a.damping = b->damping;
  a.dangling_none = b->dangling_none ? 1 : 0;
  return a;
}

#define PR_BATCH_DISPATCH(fn, b, ...)                                    \
  ((b)->stride == 1   ? fn<1>(b, ##__VA_ARGS__)                          \
   : (b)->stride == 2 ? fn<2>(b, ##__VA_ARGS__)                          \
   : (b)->stride == 4 ? fn<4>(b, ##__VA_ARGS__)                          \
   : (b)->stride == 8 ? fn<8>(b, ##__VA_ARGS__)                          \
                      : fn<16>(b, ##__VA_ARGS__))

// Whether the iterations enqueued now run the teleport-mode kernels.  On a PR_DANGLING_NONE graph
// dc is 0 and both terms vanish: the uniform kernels run.
bool teleport_mode(const pr_batch *b) { return b->dangling_mode == PR_BATCH_DANGLING_TELEPORT && !b->dangling_none; }

// Enqueues the sum of column j of T into ts[j] (k_batch_reset_col's grid and order).
template <int S>
int launch_tsum_column(pr_batch *b, int j) {
  const unsigned grid = grid_for((int64_t)b->V * S, kBatchThreads, kBatchGridMax);  // k_batch_reset's
  hipLaunchKernelGGL(k_batch_tsum_col<S>, dim3(grid), dim3(kBatchThreads), 0, b->stream, (int64_t)b->V, j,
                     b->T.as<double>(), b->part.as<double>());
  PR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_batch_tsum_finalize, dim3(1), dim3(kBatchThreads), 0, b->stream, b->part.as<double>(),
                     (int64_t)grid, j, b->ts.as<double>());
  PR_HIP(hipGetLastError());
  return PR_OK;
}

// Brings ts up to date on the batch's stream: the sum of every column whose vector changed, 0.0 for
// a column whose vector was cleared.  Allocates ts (zeros: padding columns stay 0) on first use.
// Everything that touches the part scratch or T is on the same stream, so no wait is needed.
int ensure_ts(pr_batch *b) {
  if (!b->ts.p) {
    PR_TRY(b->ts.alloc(sizeof(double) * b->stride));
    PR_HIP(hipMemsetAsync(b->ts.p, 0, sizeof(double) * b->stride, b->stream));
    b->ts_dirty = b->vec_mask;
  }
  for (int j = 0; j < b->width && b->ts_dirty; ++j) {
    if (!((b->ts_dirty >> j) & 1u)) continue;
    if ((b->vec_mask >> j) & 1u) PR_TRY(PR_BATCH_DISPATCH(launch_tsum_column, b, j));
    else PR_HIP(hipMemsetAsync(b->ts.as<double>() + j, 0, sizeof(double), b->stream));
    b->ts_dirty &= ~(1u << j);
  }
  return PR_OK;
}

// One iteration, reading the buffers of parity `cur`: the unit kernel, the long-row kernel, the
// finalize step.  until: under the active mask (the host's b->cur then moves only once the executed
// count is known), with a decide kernel at the end -- pr_batch_step_until_any's if `any`.  In
// teleport mode the caller has brought ts up to date.
template <int S>
int launch_iteration(pr_batch *b, int cur, bool until, double tol, bool any) {
  const BatchArgs a = batch_args(b, cur);
  const double *ts = b->ts.as<double>();
  const BatchUntilState *us = until ? b->until.as<BatchUntilState>() : nullptr;
  // a form's two kernels, with the arguments (`form`) that follow the common ones in both; the
  // plain teleport form takes `us` too, nullptr as in every form that is not `until`
  auto units_long = [&](auto units, auto long_rows, auto... form) -> int {
    hipLaunchKernelGGL(units, dim3(b->ugrid), dim3(kWave), 0, b->stream, a, form...);
    PR_HIP(hipGetLastError());
    if (b->n_long > 0) {
      hipLaunchKernelGGL(long_rows, dim3(b->lgrid), dim3(kBatchThreads), 0, b->stream, a, b->long_row.as<int32_t>(),
                         b->long_p0.as<int32_t>(), b->n_long, (int64_t)b->ugrid, form...);
      PR_HIP(hipGetLastError());
    }
    return PR_OK;
  };
  if (teleport_mode(b))
    PR_TRY(until ? units_long(k_batch_units_td<S, true>, k_batch_long_td<S, true>, ts, us)
                 : units_long(k_batch_units_td<S, false>, k_batch_long_td<S, false>, ts, us));
  else if (until) PR_TRY(units_long(k_batch_units_until<S>, k_batch_long_until<S>, us));
  else PR_TRY(units_long(k_batch_units<S>, k_batch_long<S>));
  if (!until) {
    hipLaunchKernelGGL(k_batch_finalize, dim3(2 * S), dim3(kBatchThreads), 0, b->stream, b->part.as<double>(),
                       (int64_t)b->ugrid + b->lgrid, S, b->dc[cur ^ 1].as<double>(), b->l1.as<double>());
    PR_HIP(hipGetLastError());
    return PR_OK;
  }
  hipLaunchKernelGGL(k_batch_finalize_until, dim3(2 * S), dim3(kBatchThreads), 0, b->stream, b->part.as<double>(),
                     (int64_t)b->ugrid + b->lgrid, S, b->dc[cur].as<double>(), b->dc[cur ^ 1].as<double>(),
                     b->l1.as<double>(), b->dcu.as<double>(), us);
  PR_HIP(hipGetLastError());
  if (any)
    hipLaunchKernelGGL(k_batch_decide_any, dim3(1), dim3(kWave), 0, b->stream, b->until.as<BatchUntilState>(),
                       b->qstate.as<BatchQueueState>(), b->l1.as<double>(), tol, b->width);
  else
    hipLaunchKernelGGL(k_batch_decide, dim3(1), dim3(kWave), 0, b->stream, b->until.as<BatchUntilState>(),
                       b->l1.as<double>(), tol, b->width);
  PR_HIP(hipGetLastError());
  return PR_OK;
}

// Enqueues the restart of column j from d_init (V doubles on the device; nullptr: 1.0).  The caller
// has waited for the stream: the part scratch is free.
template <int S>
int launch_reset_column(pr_batch *b, int j, const double *d_init) {
  const pr_graph *g = b->g;
  const unsigned grid = grid_for((int64_t)b->V * S, kBatchThreads, kBatchGridMax);  // k_batch_reset's
  hipLaunchKernelGGL(k_batch_reset_col<S>, dim3(grid), dim3(kBatchThreads), 0, b->stream, (int64_t)b->V, j, d_init,
                     g->canon_deg.as<int32_t>(), g->canon_vflags.as<uint8_t>(), b->dangling_none ? 1 : 0,
                     b->R.as<double>(), b->C[0].as<double>(), b->C[1].as<double>(), b->part.as<double>());
  PR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_batch_finalize_col, dim3(1), dim3(kBatchThreads), 0, b->stream, b->part.as<double>(),
                     (int64_t)grid, j, b->dc[0].as<double>(), b->dc[1].as<double>(), b->dcu.as<double>(),
                     b->l1.as<double>());
  PR_HIP(hipGetLastError());
  return PR_OK;
}

template <int S>
int launch_reset(pr_batch *b, const double *d_init) {
  const pr_graph *g = b->g;
  const unsigned grid = grid_for((int64_t)b->V * S, kBatchThreads, kBatchGridMax);
  hipLaunchKernelGGL(k_batch_reset<S>, dim3(grid), dim3(kBatchThreads), 0, b->stream, (int64_t)b->V, b->width, d_init,
                     b->vec_mask, b->teleport, g->canon_deg.as<int32_t>(), g->canon_vflags.as<uint8_t>(),
                     b->dangling_none ? 1 : 0, b->R.as<double>(), b->T.as<double>(), b->C[0].as<double>(),
                     b->C[1].as<double>(), b->part.as<double>());
  PR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_batch_finalize, dim3(2 * S), dim3(kBatchThreads), 0, b->stream, b->part.as<double>(),
                     (int64_t)grid, S, b->dc[0].as<double>(), b->l1.as<double>());
  PR_HIP(hipGetLastError());
  return PR_OK;
}

// Column j of T: V doubles from the host (through colbuf), or `value` everywhere (host == nullptr).
int upload_column(pr_batch *b, int j, const double *host, double value) {
  PR_HIP(hipStreamSynchronize(b->stream));  // the enqueued steps still read T
  if (host && b->V > 0)
    PR_HIP(hipMemcpyAsync(b->colbuf.p, host, sizeof(double) * (size_t)b->V, hipMemcpyHostToDevice, b->stream));
  hipLaunchKernelGGL(k_batch_set_col, dim3(grid_for(b->V, kBatchThreads, 4096)), dim3(kBatchThreads), 0, b->stream,
                     (int64_t)b->V, b->stride, j, host ? b->colbuf.as<double>() : nullptr, value, b->T.as<double>());
  PR_HIP(hipGetLastError());
  PR_HIP(hipStreamSynchronize(b->stream));  // `host` is borrowed for the call only
  return PR_OK;
}

int extract_column(pr_batch *b, int j) {
  hipLaunchKernelGGL(k_batch_extract, dim3(grid_for(b->V, kBatchThreads, 4096)), dim3(kBatchThreads), 0, b->stream,
                     (int64_t)b->V, b->stride, j, b->R.as<double>(), b->colbuf.as<double>());
  PR_HIP(hipGetLastError());
  return PR_OK;
}

// Column j of R, any column of the layout, to V doubles on the host; waited for.
int download_ranks(pr_batch *b, int j, double *ranks_out) {
  BatchDeviceGuard dg(b->device);
  PR_TRY(extract_column(b, j));
  if (b->V > 0)
    PR_HIP(hipMemcpyAsync(ranks_out, b->colbuf.p, sizeof(double) * (size_t)b->V, hipMemcpyDeviceToHost, b->stream));
  PR_HIP(hipStreamSynchronize(b->stream));
  return PR_OK;
}

// extract_column for a column with an exclusion set: also fills excl_oid (allocated here).
int extract_column_excl(pr_batch *b, int j) {
  if (!b->excl_oid.p) PR_TRY(b->excl_oid.alloc(sizeof(int32_t) * (size_t)std::max<int32_t>(b->V, 1)));
  hipLaunchKernelGGL(k_batch_extract_excl, dim3(grid_for(b->V, kBatchThreads, 4096)), dim3(kBatchThreads), 0, b->stream,
                     (int64_t)b->V, b->stride, j, b->R.as<double>(), b->excl_mask.as<uint16_t>(), b->colbuf.as<double>(),
                     b->excl_oid.as<int32_t>());
  PR_HIP(hipGetLastError());
  return PR_OK;
}

// The device mask the batch top-K reads: nullptr while no column excludes anything.
const uint16_t *active_mask(const pr_batch *b) {
  for (int j = 0; j < b->width; ++j)
    if (b->n_excl[j] > 0) return b->excl_mask.as<uint16_t>();
  return nullptr;
}

int topk_all(pr_batch *b, int32_t k, int64_t narrow_div, int32_t *ids_out, double *ranks_out, int32_t *n_out,
             int32_t *info) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (k < 0) return fail(PR_ERR_INVALID, "k < 0");
  if (narrow_div < 0) return fail(PR_ERR_INVALID, "narrow_div < 0");
  if (!n_out || (k > 0 && (!ids_out || !ranks_out))) return fail(PR_ERR_INVALID, "NULL argument");
  if (b->in_done_cb) return fail(PR_ERR_STATE, kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_get_topk_all before pr_batch_reset");
  BatchDeviceGuard dg(b->device);
  return btopk_select(&b->btopk, b->device, b->stream, b->R.as<double>(), b->V, b->width, b->stride, active_mask(b),
                      b->n_excl, k, narrow_div, ids_out, ranks_out, n_out, info);
}

// pr_batch_mix_topk and its internal form: every PR_ERR_INVALID case on the host first, then the
// state, then the blend and the select over it (pr_batch_mix.hip).
int mix_topk(pr_batch *b, int32_t n_mixes, const double *weights, const int32_t *n_exclude,
             const int32_t *const *exclude, int32_t k, int64_t narrow_div, int64_t grid_cap, int32_t *ids_out,
             double *scores_out, int32_t *n_out, int64_t *info) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (narrow_div < 0 || grid_cap < 0) return fail(PR_ERR_INVALID, "narrow_div < 0 or grid_cap < 0");
  PR_TRY(batch_mix_check_topk(b->V, b->width, n_mixes, weights, n_exclude, exclude, k, ids_out, scores_out, n_out));
  if (b->in_done_cb) return fail(PR_ERR_STATE, kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_mix_topk before pr_batch_reset");
  if (info) info[0] = info[1] = 0, info[2] = info[3] = -1;
  if (k == 0) {
    std::fill(n_out, n_out + n_mixes, 0);
    return PR_OK;
  }
  BatchDeviceGuard dg(b->device);
  return batch_mix_topk(&b->mix, b->device, b->stream, b->R.as<double>(), b->V, b->width, b->stride, n_mixes, weights,
                        n_exclude, exclude, k, narrow_div, grid_cap, ids_out, scores_out, n_out, info);
}

bool bad_tol(double tol) { return !(tol >= 0.0) || std::isinf(tol); }

// The loop of pr_batch_step_until and (any) pr_batch_step_until_any: starts the device's state from
// `mask`, then enqueues up to `block` iterations at a time, up to max_iterations in all, and reads
// the state back after each block -- into h_until, and h_queue if `any` -- until it says to stop: no
// column active, or (any) a column converged.  The launches past the stopping iteration returned at
// entry, so the batch's parity and count follow the device's executed count.  info (may be NULL):
// iterations enqueued, iterations executed.
int run_blocks(pr_batch *b, uint32_t mask, int32_t max_iterations, double tol, int32_t block, bool any, int32_t *info) {
  BatchUntilState &h = b->h_until;
  BatchQueueState &q = b->h_queue;
  h = BatchUntilState{};
  h.mask = mask;
  PR_HIP(hipMemcpyAsync(b->until.p, &h, sizeof(h), hipMemcpyHostToDevice, b->stream));
  if (any) {
    q = BatchQueueState{0, 0};
    PR_HIP(hipMemcpyAsync(b->qstate.p, &q, sizeof(q), hipMemcpyHostToDevice, b->stream));
  }
  int32_t enq = 0;
  while (enq < max_iterations && (any ? q.saved == 0 : h.mask != 0)) {
    const int32_t n = std::min(block, max_iterations - enq);
    for (int32_t i = 0; i < n; ++i, ++enq) PR_TRY(PR_BATCH_DISPATCH(launch_iteration, b, b->cur ^ (enq & 1), true, tol, any));
    // the one read-back per block: the mask, the executed count and the per-column counts
    PR_HIP(hipMemcpyAsync(&h, b->until.p, sizeof(h), hipMemcpyDeviceToHost, b->stream));
    if (any) PR_HIP(hipMemcpyAsync(&q, b->qstate.p, sizeof(q), hipMemcpyDeviceToHost, b->stream));
    PR_HIP(hipStreamSynchronize(b->stream));
  }
  b->cur ^= h.executed & 1;
  b->iters_done += h.executed;
  if (info) {
    info[0] = enq;
    info[1] = h.executed;
  }
  return PR_OK;
}

// pr_batch_step_until with the block size as a parameter; info (may be NULL): iterations enqueued,
// iterations executed.
int step_until(pr_batch *b, int32_t max_iterations, double tol, int32_t block, int32_t *iters_out, int32_t *info) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (max_iterations < 0) return fail(PR_ERR_INVALID, "max_iterations < 0");
  if (bad_tol(tol)) return fail(PR_ERR_INVALID, "tol must be a finite number >= 0");
  if (block < 1) return fail(PR_ERR_INVALID, "block < 1");
  if (b->in_done_cb) return fail(PR_ERR_STATE, kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_step_until before pr_batch_reset");
  if (info) info[0] = info[1] = 0;
  if (max_iterations == 0) {
    if (iters_out) std::fill(iters_out, iters_out + b->width, 0);
    return PR_OK;
  }
  BatchDeviceGuard dg(b->device);
  if (teleport_mode(b)) PR_TRY(ensure_ts(b));
  PR_TRY(run_blocks(b, batch_until_all(b->width), max_iterations, tol, block, false, info));
  const BatchUntilState &h = b->h_until;
  if (h.executed > 0) b->until_norms = true;
  if (iters_out) std::copy(h.iters, h.iters + b->width, iters_out);
  return PR_OK;
}

int check_column(const pr_batch *b, int32_t column) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (column < 0 || column >= b->width)
    return fail(PR_ERR_INVALID, "column " + std::to_string(column) + " is outside [0, width)");
  return PR_OK;
}

// pr_batch_step_until_any with the block size as a parameter; info (may be NULL): iterations
// enqueued, iterations executed.
int step_until_any(pr_batch *b, uint32_t active, int32_t max_iterations, double tol, int32_t block,
                   int32_t *executed_out, uint32_t *converged_out, int32_t *info) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (!executed_out || !converged_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (max_iterations < 0) return fail(PR_ERR_INVALID, "max_iterations < 0");
  if (bad_tol(tol)) return fail(PR_ERR_INVALID, "tol must be a finite number >= 0");
  if (block < 1) return fail(PR_ERR_INVALID, "block < 1");
  if (active & ~batch_until_all(b->width)) return fail(PR_ERR_INVALID, "active names a column at or above width");
  if (b->in_done_cb) return fail(PR_ERR_STATE, kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_step_until_any before pr_batch_reset");
  *executed_out = 0;
  *converged_out = 0;
  if (info) info[0] = info[1] = 0;
  if (active == 0 || max_iterations == 0) return PR_OK;
  BatchDeviceGuard dg(b->device);
  if (teleport_mode(b)) PR_TRY(ensure_ts(b));
  if (!b->until_norms) {
    // the columns outside `active` keep their norms: from now on pr_batch_get_norms reads dcu, which
    // so far holds nothing for them
    const DevBuf &used = b->dc[b->iters_done > 0 ? b->cur ^ 1 : b->cur];
    PR_HIP(hipMemcpyAsync(b->dcu.p, used.p, sizeof(double) * b->stride, hipMemcpyDeviceToDevice, b->stream));
    b->until_norms = true;
  }
  PR_TRY(run_blocks(b, active, max_iterations, tol, block, true, info));
  *executed_out = b->h_until.executed;
  *converged_out = b->h_queue.converged;
  return PR_OK;
}

// IDs inside [0, V) and distinct, without a table of V entries: a sorted copy (tmp) shows duplicates.
int check_ids(const pr_batch *b, int32_t n, const int32_t *ids, std::vector<int32_t> &tmp, const std::string &who) {
  for (int32_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= b->V)
      return fail(PR_ERR_INVALID, who + "[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is outside [0, V)");
  tmp.assign(ids, ids + n);
  std::sort(tmp.begin(), tmp.end());
  const auto dup = std::adjacent_find(tmp.begin(), tmp.end());
  if (dup != tmp.end()) return fail(PR_ERR_INVALID, "vertex " + std::to_string(*dup) + " is listed twice in " + who);
  return PR_OK;
}

// One query of pr_batch_run_queue, by the rules of pr_batch_set_teleport_sparse and pr_batch_set_exclude.
int check_query(const pr_batch *b, const pr_batch_query &q, std::vector<int32_t> &tmp) {
  if (q.n_seeds < 0 || q.n_exclude < 0) return fail(PR_ERR_INVALID, "n < 0");
  if ((q.n_seeds > 0 && (!q.ids || !q.values)) || (q.n_exclude > 0 && !q.exclude)) return fail(PR_ERR_INVALID, "NULL argument");
  if (!std::isfinite(q.rest)) return fail(PR_ERR_INVALID, "rest is not finite");
  for (int32_t i = 0; i < q.n_seeds; ++i)
    if (!std::isfinite(q.values[i])) return fail(PR_ERR_INVALID, "values[" + std::to_string(i) + "] is not finite");
  PR_TRY(check_ids(b, q.n_seeds, q.ids, tmp, "ids"));
  return check_ids(b, q.n_exclude, q.exclude, tmp, "exclude");
}

// Column j of T from a checked sparse vector, on the device: `rest` everywhere, then the n seeds.
// n * 12 bytes cross the bus.  The caller has waited for the stream (the enqueued steps read T).
int set_sparse_dev(pr_batch *b, int j, int32_t n, const int32_t *ids, const double *values, double rest) {
  if (n > 0) {
    if (b->qids.bytes < sizeof(int32_t) * (size_t)n) {
      const size_t cap = std::max<size_t>({(size_t)n, 2 * b->qids.bytes / sizeof(int32_t), 256});
      PR_TRY(b->qids.alloc(sizeof(int32_t) * cap));
      PR_TRY(b->qvals.alloc(sizeof(double) * cap));
    }
    PR_HIP(hipMemcpyAsync(b->qids.p, ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, b->stream));
    PR_HIP(hipMemcpyAsync(b->qvals.p, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, b->stream));
  }
  hipLaunchKernelGGL(k_batch_set_col, dim3(grid_for(b->V, kBatchThreads, 4096)), dim3(kBatchThreads), 0, b->stream,
                     (int64_t)b->V, b->stride, j, (const double *)nullptr, rest, b->T.as<double>());
  PR_HIP(hipGetLastError());
  if (n > 0) {
    hipLaunchKernelGGL(k_batch_scatter_col, dim3(grid_for(n, kBatchThreads, 4096)), dim3(kBatchThreads), 0, b->stream, n,
                       b->stride, j, b->qids.as<int32_t>(), b->qvals.as<double>(), b->T.as<double>());
    PR_HIP(hipGetLastError());
  }
  b->vec_mask |= 1u << j;
  b->ts_dirty |= 1u << j;
  return PR_OK;
}

// Column j's exclusion set becomes the checked ids[0..n) in the host's copy of the mask; *dirty is
// set when the device's copy has to follow (upload_exclude).  Everything that can fail comes before
// the first change, so a failure leaves the sets as they were.
int apply_exclude(pr_batch *b, int j, int32_t n, const int32_t *ids, bool *dirty) {
  if (n == 0 && b->n_excl[j] == 0) return PR_OK;
  if (!b->excl_mask.p) PR_TRY(b->excl_mask.alloc(sizeof(uint16_t) * (size_t)b->V));
  std::vector<int32_t> mine;
  try {
    if (b->h_mask.empty()) b->h_mask.assign((size_t)b->V, 0);
    mine.assign(ids, ids + n);
  } catch (const std::bad_alloc &) {
    return fail(PR_ERR_OOM, "host allocation failed");
  }
  const uint16_t bit = (uint16_t)(1u << j);
  for (int32_t v : b->excl_ids[j]) b->h_mask[(size_t)v] &= (uint16_t)~bit;
  for (int32_t i = 0; i < n; ++i) b->h_mask[(size_t)ids[i]] |= bit;
  b->excl_ids[j].swap(mine);
  b->n_excl[j] = n;
  *dirty = true;
  return PR_OK;
}

// The host's mask to the device, whole (2 V bytes), and waited for: the host copy may change right after.
int upload_exclude(pr_batch *b) {
  PR_HIP(hipMemcpyAsync(b->excl_mask.p, b->h_mask.data(), sizeof(uint16_t) * (size_t)b->V, hipMemcpyHostToDevice,
                        b->stream));
  PR_HIP(hipStreamSynchronize(b->stream));
  return PR_OK;
}

int run_queue(pr_batch *b, int32_t n_queries, const pr_batch_query *queries, int32_t max_iterations, double tol,
              const double *init_ranks, pr_batch_done_cb done, void *user) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (n_queries < 0) return fail(PR_ERR_INVALID, "n_queries < 0");
  if (n_queries > 0 && !queries) return fail(PR_ERR_INVALID, "NULL argument");
  if (max_iterations < 1) return fail(PR_ERR_INVALID, "max_iterations < 1");
  if (bad_tol(tol)) return fail(PR_ERR_INVALID, "tol must be a finite number >= 0");
  if (b->in_done_cb) return fail(PR_ERR_STATE, kInDoneCb);
  {
    std::vector<int32_t> tmp;
    for (int32_t q = 0; q < n_queries; ++q)
      if (check_query(b, queries[q], tmp) != PR_OK)
        return fail(PR_ERR_INVALID, "query " + std::to_string(q) + ": " + pr_last_error());
  }
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_run_queue before pr_batch_reset");
  if (n_queries == 0) return PR_OK;
  BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));
  const double *d_init = nullptr;
  if (init_ranks && b->V > 0) {
    if (!b->qinit.p) PR_TRY(b->qinit.alloc(sizeof(double) * (size_t)b->V));
    PR_HIP(hipMemcpyAsync(b->qinit.p, init_ranks, sizeof(double) * (size_t)b->V, hipMemcpyHostToDevice, b->stream));
    d_init = b->qinit.as<double>();
  }
  QueueSched s;
  s.init(n_queries, b->width, max_iterations);
  int32_t cols[kBatchMaxWidth], qs[kBatchMaxWidth];
  QueueDone dn[kBatchMaxWidth];
  double l1[kBatchMaxWidth];
  while (!s.finished()) {
    // the stream is idle here: the last call and the getters of the callbacks are synchronous
    const int nf = s.refill(cols, qs);
    bool mask_dirty = false;
    for (int i = 0; i < nf; ++i) {
      const pr_batch_query &q = queries[qs[i]];
      PR_TRY(set_sparse_dev(b, cols[i], q.n_seeds, q.ids, q.values, q.rest));
      PR_TRY(apply_exclude(b, cols[i], q.n_exclude, q.exclude, &mask_dirty));
      PR_TRY(PR_BATCH_DISPATCH(launch_reset_column, b, cols[i], d_init));
    }
    if (mask_dirty) PR_TRY(upload_exclude(b));  // once for all the columns refilled together
    int32_t executed = 0;
    uint32_t converged = 0;
    PR_TRY(step_until_any(b, s.active(), s.cap(), tol, kAnyBlock, &executed, &converged, nullptr));
    PR_HIP(hipMemcpyAsync(l1, b->l1.p, sizeof(double) * b->stride, hipMemcpyDeviceToHost, b->stream));
    PR_HIP(hipStreamSynchronize(b->stream));
    const int nd = s.advance(executed, converged, dn);
    for (int i = 0; i < nd && done; ++i) {
      b->in_done_cb = true;
      done(dn[i].query, dn[i].column, dn[i].iterations, dn[i].converged, l1[dn[i].column], user);
      b->in_done_cb = false;
    }
  }
  return PR_OK;
}

int build_batch(pr_batch *b) {
  pr_graph *g = b->g;
  const int S = b->stride;
  const size_t V = (size_t)b->V;
  PR_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  PR_HIP(hipEventCreate(&b->ev0));
  PR_HIP(hipEventCreate(&b->ev1));
  std::vector<int64_t> rp(V + 1, 0);
  PR_HIP(hipStreamSynchronize(g->stream));
  PR_HIP(hipMemcpy(rp.data(), g->canon_rowptr.p, sizeof(int64_t) * (V + 1), hipMemcpyDeviceToHost));
  BatchPlan plan;
  batch_plan(rp.data(), (int64_t)V, S, &plan);
  b->n_units = (int64_t)plan.units.size();
  b->n_long = (int64_t)plan.long_row.size();
  b->n_slots = plan.long_p0.back();
  b->ugrid = (int)std::max<int64_t>(1, std::min<int64_t>(b->n_units, kBatchGridMax));
  b->lgrid = (int)((b->n_long * S + kBatchThreads - 1) / kBatchThreads);
  PR_TRY(b->units.alloc(sizeof(BatchUnit) * plan.units.size()));
  PR_TRY(b->long_row.alloc(sizeof(int32_t) * plan.long_row.size()));
  PR_TRY(b->long_p0.alloc(sizeof(int32_t) * plan.long_p0.size()));
  PR_TRY(b->chunk_part.alloc(sizeof(double) * (size_t)b->n_slots * S));
  if (!plan.units.empty())
    PR_HIP(hipMemcpy(b->units.p, plan.units.data(), sizeof(BatchUnit) * plan.units.size(), hipMemcpyHostToDevice));
  if (!plan.long_row.empty())
    PR_HIP(hipMemcpy(b->long_row.p, plan.long_row.data(), sizeof(int32_t) * plan.long_row.size(), hipMemcpyHostToDevice));
  PR_HIP(hipMemcpy(b->long_p0.p, plan.long_p0.data(), sizeof(int32_t) * plan.long_p0.size(), hipMemcpyHostToDevice));
  const size_t mat = sizeof(double) * V * (size_t)S;
  PR_TRY(b->R.alloc(mat));
  PR_TRY(b->T.alloc(mat));
  PR_TRY(b->C[0].alloc(mat));
  PR_TRY(b->C[1].alloc(mat));
  PR_TRY(b->dc[0].alloc(sizeof(double) * S));
  PR_TRY(b->dc[1].alloc(sizeof(double) * S));
  PR_TRY(b->l1.alloc(sizeof(double) * S));
  // the reset's grid is at most kBatchGridMax workgroups, an iteration's ugrid + lgrid
  PR_TRY(b->part.alloc(sizeof(double) * 2 * S * ((size_t)kBatchGridMax + (size_t)b->lgrid)));
  PR_TRY(b->colbuf.alloc(sizeof(double) * V));
  PR_TRY(b->until.alloc(sizeof(BatchUntilState)));
  PR_TRY(b->dcu.alloc(sizeof(double) * S));
  PR_TRY(b->qstate.alloc(sizeof(BatchQueueState)));
  return PR_OK;
}

}  // namespace
}  // namespace pr

using pr::fail;

extern "C" {

int pr_batch_create(pr_graph *g, int32_t width, pr_batch **out) {
  if (!g || !out) return fail(PR_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (width < 1 || width > pr::kBatchMaxWidth) return fail(PR_ERR_INVALID, "width must be in [1, 16]");
  if (g->nparts != 1 || g->grouped || g->comm)
    return fail(PR_ERR_STATE, "a batch needs a single-part graph (no group, no communicator)");
  if (!g->has_canonical) return fail(PR_ERR_STATE, "a batch needs the canonical CSR (graph built with PR_NO_CANONICAL)");
  pr::BatchDeviceGuard dg(g->device);
  pr_batch *b = new (std::nothrow) pr_batch();
  if (!b) return fail(PR_ERR_OOM, "host allocation failed");
  b->g = g;
  b->device = g->device;
  b->width = width;
  b->stride = pr::batch_stride(width);
  b->V = g->V;
  b->dangling_none = (g->flags & PR_DANGLING_NONE) != 0;
  const int rc = pr::build_batch(b);
  if (rc != PR_OK) {
    const std::string msg = pr_last_error();
    pr_batch_destroy(b);
    pr::set_error(msg);
    return rc;
  }
  *out = b;
  return PR_OK;
}

int pr_batch_set_teleport(pr_batch *b, int32_t column, const double *teleport) {
  PR_TRY(pr::check_column(b, column));
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (teleport)  // host checks first: nothing below touches the device before they pass
    for (int32_t v = 0; v < b->V; ++v)
      if (!std::isfinite(teleport[v])) return fail(PR_ERR_INVALID, "teleport[" + std::to_string(v) + "] is not finite");
  pr::BatchDeviceGuard dg(b->device);
  PR_TRY(pr::upload_column(b, column, teleport, b->teleport));
  if (teleport) b->vec_mask |= 1u << column;
  else b->vec_mask &= ~(1u << column);
  b->ts_dirty |= 1u << column;
  return PR_OK;
}

int pr_batch_set_teleport_sparse(pr_batch *b, int32_t column, int32_t n, const int32_t *ids, const double *values,
                                 double rest) {
  PR_TRY(pr::check_column(b, column));
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (n < 0) return fail(PR_ERR_INVALID, "n < 0");
  if (n > 0 && (!ids || !values)) return fail(PR_ERR_INVALID, "NULL argument");
  if (!std::isfinite(rest)) return fail(PR_ERR_INVALID, "rest is not finite");
  for (int32_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= b->V)
      return fail(PR_ERR_INVALID, "ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is outside [0, V)");
    if (!std::isfinite(values[i])) return fail(PR_ERR_INVALID, "values[" + std::to_string(i) + "] is not finite");
  }
  std::vector<double> dense((size_t)b->V, rest);
  std::vector<uint8_t> seen((size_t)b->V, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (seen[(size_t)ids[i]]) return fail(PR_ERR_INVALID, "vertex " + std::to_string(ids[i]) + " is listed twice in ids");
    seen[(size_t)ids[i]] = 1;
    dense[(size_t)ids[i]] = values[i];
  }
  pr::BatchDeviceGuard dg(b->device);
  PR_TRY(pr::upload_column(b, column, dense.data(), 0.0));
  b->vec_mask |= 1u << column;
  b->ts_dirty |= 1u << column;
  return PR_OK;
}

int pr_batch_reset(pr_batch *b, double teleport, double damping, const double *init_ranks) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  pr::BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));
  b->teleport = teleport;
  b->damping = damping;
  const double *d_init = nullptr;
  if (init_ranks && b->V > 0) {
    PR_HIP(hipMemcpyAsync(b->colbuf.p, init_ranks, sizeof(double) * (size_t)b->V, hipMemcpyHostToDevice, b->stream));
    d_init = b->colbuf.as<double>();
  }
  PR_TRY(PR_BATCH_DISPATCH(pr::launch_reset, b, d_init));
  PR_HIP(hipStreamSynchronize(b->stream));  // init_ranks is borrowed for the call only
  b->cur = 0;
  b->iters_done = 0;
  b->until_norms = false;
  b->ready = true;
  return PR_OK;
}

int pr_batch_step(pr_batch *b, int32_t iterations) {
  if (!b || iterations < 0) return fail(PR_ERR_INVALID, "NULL batch or iterations < 0");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_step before pr_batch_reset");
  pr::BatchDeviceGuard dg(b->device);
  if (iterations > 0 && pr::teleport_mode(b)) PR_TRY(pr::ensure_ts(b));
  if (iterations > 0) {
    PR_HIP(hipEventRecord(b->ev0, b->stream));
    b->until_norms = false;  // every column advances: the last iteration's dc is dc[cur ^ 1] again
  }
  for (int32_t it = 0; it < iterations; ++it) {
    PR_TRY(PR_BATCH_DISPATCH(pr::launch_iteration, b, b->cur, false, 0.0, false));
    b->cur ^= 1;
    ++b->iters_done;
  }
  if (iterations > 0) {
    PR_HIP(hipEventRecord(b->ev1, b->stream));
    b->timed = true;
  }
  return PR_OK;
}

int pr_batch_step_until(pr_batch *b, int32_t max_iterations, double tol, int32_t *iters_out) {
  return pr::step_until(b, max_iterations, tol, pr::kUntilBlock, iters_out, nullptr);
}

// Internal entry point (not part of include/pagerank_hip.h): pr_batch_step_until with the number of
// iterations enqueued between two read-backs as a parameter (>= 1), and info[2] = {iterations
// enqueued, iterations executed}, so that tests can show that the result does not depend on it.
int pr_batch_step_until_ex(pr_batch *b, int32_t max_iterations, double tol, int32_t block, int32_t *iters_out,
                           int32_t *info) {
  return pr::step_until(b, max_iterations, tol, block, iters_out, info);
}

int pr_batch_reset_column(pr_batch *b, int32_t column, const double *init_ranks) {
  PR_TRY(pr::check_column(b, column));
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_reset_column before pr_batch_reset");
  pr::BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));  // the enqueued steps still read and write the column
  const double *d_init = nullptr;
  if (init_ranks && b->V > 0) {
    PR_HIP(hipMemcpyAsync(b->colbuf.p, init_ranks, sizeof(double) * (size_t)b->V, hipMemcpyHostToDevice, b->stream));
    d_init = b->colbuf.as<double>();
  }
  PR_TRY(PR_BATCH_DISPATCH(pr::launch_reset_column, b, column, d_init));
  PR_HIP(hipStreamSynchronize(b->stream));  // init_ranks is borrowed for the call only
  return PR_OK;
}

int pr_batch_step_until_any(pr_batch *b, uint32_t active, int32_t max_iterations, double tol, int32_t *executed_out,
                            uint32_t *converged_out) {
  return pr::step_until_any(b, active, max_iterations, tol, pr::kAnyBlock, executed_out, converged_out, nullptr);
}

// Internal entry point (not part of include/pagerank_hip.h): pr_batch_step_until_any with the number
// of iterations enqueued between two read-backs as a parameter (>= 1), and info[2] = {iterations
// enqueued, iterations executed}.
int pr_batch_step_until_any_ex(pr_batch *b, uint32_t active, int32_t max_iterations, double tol, int32_t block,
                               int32_t *executed_out, uint32_t *converged_out, int32_t *info) {
  return pr::step_until_any(b, active, max_iterations, tol, block, executed_out, converged_out, info);
}

int pr_batch_run_queue(pr_batch *b, int32_t n_queries, const pr_batch_query *queries, int32_t max_iterations,
                       double tol, const double *init_ranks, pr_batch_done_cb done, void *user) {
  return pr::run_queue(b, n_queries, queries, max_iterations, tol, init_ranks, done, user);
}

int pr_batch_set_dangling(pr_batch *b, int32_t mode) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (mode != PR_BATCH_DANGLING_UNIFORM && mode != PR_BATCH_DANGLING_TELEPORT)
    return fail(PR_ERR_INVALID, "mode must be PR_BATCH_DANGLING_UNIFORM or PR_BATCH_DANGLING_TELEPORT");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  pr::BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));
  b->dangling_mode = mode;  // ts follows before the next teleport-mode iteration is enqueued (ensure_ts)
  return PR_OK;
}

int pr_batch_get_dangling(const pr_batch *b, int32_t *mode_out) {
  if (!b || !mode_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  *mode_out = b->dangling_mode;
  return PR_OK;
}

int pr_batch_get_teleport_sums(pr_batch *b, double *sums_out) {
  if (!b || !sums_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  pr::BatchDeviceGuard dg(b->device);
  PR_TRY(pr::ensure_ts(b));
  double ts[pr::kBatchMaxWidth];
  PR_HIP(hipMemcpyAsync(ts, b->ts.p, sizeof(double) * b->stride, hipMemcpyDeviceToHost, b->stream));
  PR_HIP(hipStreamSynchronize(b->stream));
  std::copy(ts, ts + b->width, sums_out);
  return PR_OK;
}

int pr_batch_sync(pr_batch *b) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  pr::BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));
  return PR_OK;
}

int pr_batch_get_ranks(pr_batch *b, int32_t column, double *ranks_out) {
  PR_TRY(pr::check_column(b, column));
  if (!ranks_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_get_ranks before pr_batch_reset");
  return pr::download_ranks(b, column, ranks_out);
}

// Internal entry point (not part of include/pagerank_hip.h): pr_batch_get_ranks for any column of the
// layout, [0, stride), so that tests can show that the padding columns hold zeros.
int pr_batch_get_ranks_ex(pr_batch *b, int32_t column, double *ranks_out) {
  if (!b || !ranks_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (column < 0 || column >= b->stride) return fail(PR_ERR_INVALID, "column is outside [0, stride)");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_get_ranks_ex before pr_batch_reset");
  return pr::download_ranks(b, column, ranks_out);
}

int pr_batch_get_norms(pr_batch *b, double *dc_out, double *l_out) {
  if (!b || !dc_out || !l_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_get_norms before pr_batch_reset");
  pr::BatchDeviceGuard dg(b->device);
  double dc[pr::kBatchMaxWidth], l1[pr::kBatchMaxWidth];
  // the dc *used* by the last iteration lives in the previous buffer (none run: the reset's); after
  // pr_batch_step_until the columns stopped at different iterations and dcu holds each one's
  const pr::DevBuf &used = b->until_norms ? b->dcu : b->dc[b->iters_done > 0 ? b->cur ^ 1 : b->cur];
  PR_HIP(hipMemcpyAsync(dc, used.p, sizeof(double) * b->stride, hipMemcpyDeviceToHost, b->stream));
  PR_HIP(hipMemcpyAsync(l1, b->l1.p, sizeof(double) * b->stride, hipMemcpyDeviceToHost, b->stream));
  PR_HIP(hipStreamSynchronize(b->stream));
  for (int j = 0; j < b->width; ++j) {
    dc_out[j] = dc[j];
    l_out[j] = b->iters_done > 0 ? l1[j] : 0.0;
  }
  return PR_OK;
}

int pr_batch_get_topk(pr_batch *b, int32_t column, int32_t k, int32_t *ids_out, double *ranks_out, int32_t *n_out) {
  PR_TRY(pr::check_column(b, column));
  if (k < 0) return fail(PR_ERR_INVALID, "k < 0");
  if (!n_out || (k > 0 && (!ids_out || !ranks_out))) return fail(PR_ERR_INVALID, "NULL argument");
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_get_topk before pr_batch_reset");
  pr::BatchDeviceGuard dg(b->device);
  if (b->n_excl[column] > 0) {  // the excluded vertices are holes of the select
    PR_TRY(pr::extract_column_excl(b, column));
    return pr::topk_select(&b->topk, b->device, b->stream, b->colbuf.as<double>(), b->excl_oid.as<int32_t>(), b->V,
                           b->V - b->n_excl[column], k, pr::kTopkNarrowDiv, ids_out, ranks_out, n_out, nullptr);
  }
  PR_TRY(pr::extract_column(b, column));
  return pr::topk_select(&b->topk, b->device, b->stream, b->colbuf.as<double>(), nullptr, b->V, b->V, k,
                         pr::kTopkNarrowDiv, ids_out, ranks_out, n_out, nullptr);
}

int pr_batch_set_exclude(pr_batch *b, int32_t column, int32_t n, const int32_t *ids) {
  PR_TRY(pr::check_column(b, column));
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (n < 0) return fail(PR_ERR_INVALID, "n < 0");
  if (n > 0 && !ids) return fail(PR_ERR_INVALID, "NULL argument");
  for (int32_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= b->V)
      return fail(PR_ERR_INVALID, "ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is outside [0, V)");
  try {
    std::vector<uint8_t> seen(n > 0 ? (size_t)b->V : 0, 0);
    for (int32_t i = 0; i < n; ++i) {
      if (seen[(size_t)ids[i]]) return fail(PR_ERR_INVALID, "vertex " + std::to_string(ids[i]) + " is listed twice in ids");
      seen[(size_t)ids[i]] = 1;
    }
  } catch (const std::bad_alloc &) {
    return fail(PR_ERR_OOM, "host allocation failed");
  }
  pr::BatchDeviceGuard dg(b->device);
  PR_HIP(hipStreamSynchronize(b->stream));
  bool dirty = false;
  PR_TRY(pr::apply_exclude(b, column, n, ids, &dirty));  // nothing to do while no set was ever stored and this one is empty
  if (dirty) PR_TRY(pr::upload_exclude(b));
  return PR_OK;
}

int pr_batch_get_topk_all(pr_batch *b, int32_t k, int32_t *ids_out, double *ranks_out, int32_t *n_out) {
  return pr::topk_all(b, k, pr::kTopkNarrowDiv, ids_out, ranks_out, n_out, nullptr);
}

// Internal entry point (not part of include/pagerank_hip.h): pr_batch_get_topk_all with the narrowing
// divisor as a parameter (0: never narrow) and the pass counts in info[4] (pr_graph.h btopk_select),
// so that tests reach both sides of the switch at small sizes.
int pr_batch_topk_all_ex(pr_batch *b, int32_t k, int64_t narrow_div, int32_t *ids_out, double *ranks_out,
                         int32_t *n_out, int32_t *info) {
  return pr::topk_all(b, k, narrow_div, ids_out, ranks_out, n_out, info);
}

// Internal: the summed HIP-event time in ns of the kernels of the last pr_batch_topk_all_ex call (-1: none).
int pr_batch_topk_all_kernel_ns(const pr_batch *b, int64_t *ns_out) {
  if (!b || !ns_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  *ns_out = pr::btopk_kernel_ns(b->btopk);
  return PR_OK;
}

int pr_batch_mix_topk(pr_batch *b, int32_t n_mixes, const double *weights, const int32_t *n_exclude,
                      const int32_t *const *exclude, int32_t k, int32_t *ids_out, double *scores_out, int32_t *n_out) {
  return pr::mix_topk(b, n_mixes, weights, n_exclude, exclude, k, pr::kTopkNarrowDiv, 0, ids_out, scores_out, n_out,
                      nullptr);
}

// Internal entry point (not part of include/pagerank_hip.h): pr_batch_mix_topk with the select's
// narrowing divisor (0: never narrow) and a cap on k_batch_mix's grid in workgroups (0: none), so that
// tests reach the narrowed path and the later trips of the kernel's grid-stride loop at small sizes.
// info[4] (may be NULL) = {histogram passes over the blend matrix, passes over the compacted
// candidates, HIP-event time in ns of k_batch_mix, summed HIP-event time in ns of the select's
// kernels}; the times are -1 where nothing ran.
int pr_batch_mix_topk_ex(pr_batch *b, int32_t n_mixes, const double *weights, const int32_t *n_exclude,
                         const int32_t *const *exclude, int32_t k, int32_t *ids_out, double *scores_out,
                         int32_t *n_out, int64_t narrow_div, int64_t grid_cap, int64_t *info) {
  return pr::mix_topk(b, n_mixes, weights, n_exclude, exclude, k, narrow_div, grid_cap, ids_out, scores_out, n_out, info);
}

int pr_batch_mix_get(pr_batch *b, const double *weights, double *scores_out) {
  if (!b) return fail(PR_ERR_INVALID, "NULL batch");
  PR_TRY(pr::batch_mix_check_get(b->width, weights, scores_out));
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  if (!b->ready) return fail(PR_ERR_STATE, "pr_batch_mix_get before pr_batch_reset");
  pr::BatchDeviceGuard dg(b->device);
  return pr::batch_mix_get(&b->mix, b->device, b->stream, b->R.as<double>(), b->V, b->width, b->stride, weights,
                           b->colbuf.as<double>(), scores_out);
}

int pr_batch_info(const pr_batch *b, int64_t *info, int32_t n_info) {
  if (!b || !info) return fail(PR_ERR_INVALID, "NULL argument");
  if (b->in_done_cb) return fail(PR_ERR_STATE, pr::kInDoneCb);
  int64_t step_ns = -1;  // the last pr_batch_step call's iterations, HIP events; -1: none yet or still running
  float ms = 0.f;
  if (n_info > 6 && b->timed) {
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess) step_ns = (int64_t)((double)ms * 1e6);
    else (void)hipGetLastError();
  }
  const int64_t v[7] = {b->width, b->stride, b->n_units, b->n_long, (int64_t)b->device_bytes(), b->iters_done, step_ns};
  for (int32_t i = 0; i < n_info && i < 7; ++i) info[i] = v[i];
  return PR_OK;
}

void pr_batch_destroy(pr_batch *b) {
  if (!b) return;
  pr::BatchDeviceGuard dg(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  pr::topk_state_free(b->topk);
  b->topk = nullptr;
  pr::btopk_state_free(b->btopk);
  b->btopk = nullptr;
  pr::batch_mix_free(b->mix);
  b->mix = nullptr;
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  hipStream_t s = b->stream;
  b->stream = nullptr;
  delete b;  // DevBufs free their memory
  if (s) (void)hipStreamDestroy(s);
}

}  // extern "C"
