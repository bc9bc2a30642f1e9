// Batch mixes for gfx950 (pr_batch_mix_topk, pr_batch_mix_get; the blend itself in pr_batch_mix.h):
// up to 16 weighted blends of a batch's columns, written as a second interleaved matrix
// M (V x stride_m, element (v, i) at v * stride_m + i) next to the rank matrix R (V x stride), and
// the lockstep select of pr_batch_topk.hip run over M as it runs over R.
//
// k_batch_mix<S_IN, S_OUT> is one streaming sweep.  A wave takes 64 consecutive vertices per trip of
// its grid-stride loop: lane l loads elements l, 64 + l, ... of the tile's 64 x S_IN block of R --
// every element once, by the lane at its position, every 128-byte line once -- into S_IN registers,
// and stores elements l, 64 + l, ... of the tile's 64 x S_OUT block of M.  The S_IN values of a
// vertex reach the lanes that blend them by wave shuffles of one register at a time (at S_IN = 16,
// where a vertex's columns are one row of 16 lanes, by DPP row broadcasts); which register and
// which lane is fixed by (S_IN, S_OUT) and the lane alone:
//   S_IN <= S_OUT  output register t holds 64 / S_OUT vertices, all inside input register
//                  t * S_IN / S_OUT; lane l blends mix l % S_OUT of vertex l / S_OUT there, from
//                  the lanes that hold that vertex's columns.
//   S_IN >  S_OUT  an output register spans S_IN / S_OUT input registers.  Each of them is blended
//                  where it lies (lane l: mix l % S_IN of the vertex its lane group holds; mixes
//                  at or above S_OUT have zero weights), and one more shuffle per input register
//                  moves the results to their places in the output register.
// Either way a lane adds the columns j = 0, 1, ... in that order with batch_mix_add, so the bits of
// m_i[v] do not depend on the pair.  The weights come from a 16 x 16 device table (zeros outside
// n_mixes x width), uploaded once per launch; a lane keeps its mix's row in registers.  Column j is
// skipped by the whole grid when no mix gives it a non-zero weight (`cols`, a kernel argument: a
// scalar branch); within a column, a lane whose own weight is 0 drops the product by a select.
// Padding columns of M get +0.0.  No atomics, no LDS, no scratch.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "pr_batch_mix.h"
#include "pr_batch_topk.h"
#include "pr_device.h"
#include "pr_graph.h"

namespace pr {

struct BatchMixState {
  DevBuf M;     // V x stride_m doubles: the blends
  DevBuf wtab;  // kBatchMaxMixes x kBatchMaxWidth doubles: the weights of the launch
  DevBuf mask;  // uint16_t[V]: bit i leaves the vertex out of mix i; with the first non-empty set
  int stride_m = 0;
  BTopkState *sel = nullptr;  // the select's scratch, sized for stride_m
  // the uploads' host copies: they outlive every call, so a copy still pending when a call returns
  // early with an error reads valid memory
  double h_wtab[kBatchMaxMixes * kBatchMaxWidth] = {0};
  std::vector<uint16_t> h_mask;
  int grid_max = 0;  // workgroups of a full-device launch
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around k_batch_mix in timed calls
};

namespace {

constexpr int kMixThreads = 256;
constexpr int kMixWaves = kMixThreads / kWave;
constexpr int kMixBlocksPerCU = 8;

// x of lane J of the calling lane's row of 16 lanes: a DPP row broadcast (two v_mov_b32 row_newbcast),
// which stays in the vector ALU -- ds_bpermute goes through the LDS crossbar, and at S_IN = 16 its
// rate, not memory, bounded the sweep (profiles/batch_mix/README.md).  All lanes are active.
template <int J>
__device__ __forceinline__ double row_lane(double x) {
  constexpr int kRowNewBcast = 0x150;  // DPP control row_newbcast:0, + J
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), kRowNewBcast + J, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), kRowNewBcast + J, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// mix_blend's loop at S_IN = 16, where a vertex's columns are the 16 lanes of a row: columns J, J + 1, ...
template <int J = 0>
__device__ __forceinline__ double mix_blend_row16(double xu, const double (&w)[16], double acc, uint32_t cols) {
  if constexpr (J < 16) {
    if ((cols >> J) & 1u) acc = batch_mix_add(acc, w[J], row_lane<J>(xu));
    return mix_blend_row16<J + 1>(xu, w, acc, cols);
  } else {
    return acc;
  }
}

// The blend of the vertex whose columns lie in lanes src0 .. src0 + S_IN - 1 of register xu, under
// the weights w of the calling lane's mix (any: one of them is not 0).  Every lane of the wave calls
// it (`cols` is uniform).
template <int S_IN>
__device__ __forceinline__ double mix_blend(double xu, int src0, const double (&w)[S_IN], bool any, uint32_t cols) {
  double acc = batch_mix_start();
  if constexpr (S_IN == 16) {
    acc = mix_blend_row16(xu, w, acc, cols);  // src0 is the first lane of the calling lane's row of 16
  } else {
#pragma unroll
    for (int j = 0; j < S_IN; ++j) {
      if (!((cols >> j) & 1u)) continue;
      acc = batch_mix_add(acc, w[j], __shfl(xu, src0 + j, kWave));
    }
  }
  return batch_mix_result(acc, any);
}

template <int S_IN, int S_OUT>
__global__ __launch_bounds__(kMixThreads) void k_batch_mix(const double *__restrict__ R, double *__restrict__ M,
                                                           const double *__restrict__ wtab, int64_t V, uint32_t cols) {
  constexpr int kVin = kWave / S_IN, kVout = kWave / S_OUT;  // vertices per input / output register
  const int lane = lane_id();
  const int mine = S_IN <= S_OUT ? lane % S_OUT : lane % S_IN;  // the mix this lane blends
  double w[S_IN];
  bool any = false;
#pragma unroll
  for (int j = 0; j < S_IN; ++j) {
    w[j] = wtab[mine * kBatchMaxWidth + j];
    any = any || w[j] != 0.0;
  }
  const int64_t n_in = V * S_IN, n_out = V * S_OUT, tiles = (V + kWave - 1) / kWave;
  const int64_t waves = (int64_t)gridDim.x * kMixWaves;
  for (int64_t tile = (int64_t)blockIdx.x * kMixWaves + wave_id(); tile < tiles; tile += waves) {  // uniform per wave
    const int64_t in0 = tile * kWave * S_IN, out0 = tile * kWave * S_OUT;
    double x[S_IN];
#pragma unroll
    for (int u = 0; u < S_IN; ++u) {
      const int64_t q = in0 + (int64_t)u * kWave + lane;
      x[u] = q < n_in ? R[q] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < S_OUT; ++t) {
      double y = 0.0;
      if constexpr (S_IN <= S_OUT) {
        y = mix_blend<S_IN>(x[(t * S_IN) / S_OUT], ((t * S_IN) % S_OUT) * kVout + (lane / S_OUT) * S_IN, w, any, cols);
      } else {
        constexpr int kRatio = S_IN / S_OUT;
        const int vo = lane / S_OUT;  // the lane's vertex within the output register
#pragma unroll
        for (int c = 0; c < kRatio; ++c) {
          const double z = mix_blend<S_IN>(x[t * kRatio + c], (lane / S_IN) * S_IN, w, any, cols);
          const double zz = __shfl(z, (vo % kVin) * S_IN + lane % S_OUT, kWave);
          y = vo / kVin == c ? zz : y;
        }
      }
      const int64_t q = out0 + (int64_t)t * kWave + lane;
      if (q < n_out) M[q] = y;
    }
  }
}

// Column 0 of M (V x S) to V contiguous doubles.
__global__ __launch_bounds__(kMixThreads) void k_batch_mix_col(int64_t V, int S, const double *__restrict__ m,
                                                               double *__restrict__ out) {
  for (int64_t v = (int64_t)blockIdx.x * kMixThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kMixThreads)
    out[v] = m[v * S];
}

template <int S_IN, int S_OUT>
int launch_mix(const BatchMixState *t, hipStream_t s, const double *R, int64_t V, uint32_t cols, unsigned grid) {
  hipLaunchKernelGGL((k_batch_mix<S_IN, S_OUT>), dim3(grid), dim3(kMixThreads), 0, s, R, t->M.as<double>(),
                     t->wtab.as<double>(), V, cols);
  PR_HIP(hipGetLastError());
  return PR_OK;
}

template <int S_IN>
int launch_mix_in(const BatchMixState *t, hipStream_t s, const double *R, int64_t V, uint32_t cols, unsigned grid) {
  switch (t->stride_m) {
    case 1: return launch_mix<S_IN, 1>(t, s, R, V, cols, grid);
    case 2: return launch_mix<S_IN, 2>(t, s, R, V, cols, grid);
    case 4: return launch_mix<S_IN, 4>(t, s, R, V, cols, grid);
    case 8: return launch_mix<S_IN, 8>(t, s, R, V, cols, grid);
    default: return launch_mix<S_IN, 16>(t, s, R, V, cols, grid);
  }
}

// The state, with M wide enough for n_mixes.  A wider M takes the place of the old one, and the
// select's scratch, whose size follows the stride, is dropped with it.
int mix_state(BatchMixState **st, int device, int64_t V, int n_mixes) {
  if (!*st) {
    BatchMixState *t = new (std::nothrow) BatchMixState();
    if (!t) return fail(PR_ERR_OOM, "host allocation failed");
    *st = t;
  }
  BatchMixState *t = *st;
  if (!t->wtab.p) {
    int cus = 0;
    PR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    t->grid_max = std::max(1, cus) * kMixBlocksPerCU;
    PR_TRY(t->wtab.alloc(sizeof(t->h_wtab)));
  }
  const int S = batch_mix_stride(n_mixes);
  if (S > t->stride_m) {
    btopk_state_free(t->sel);
    t->sel = nullptr;
    t->stride_m = 0;
    PR_TRY(t->M.alloc(sizeof(double) * (size_t)std::max<int64_t>(V, 1) * (size_t)S));
    t->stride_m = S;
  }
  return PR_OK;
}

// Enqueues the upload of the weights and k_batch_mix.  grid_cap > 0 caps the grid.
int run_mix(BatchMixState *t, hipStream_t s, const double *R, int64_t V, int width, int stride, int n_mixes,
            const double *weights, int64_t grid_cap, bool timed) {
  uint32_t cols = 0;
  std::fill(t->h_wtab, t->h_wtab + kBatchMaxMixes * kBatchMaxWidth, 0.0);
  for (int i = 0; i < n_mixes; ++i)
    for (int j = 0; j < width; ++j) {
      const double w = weights[(size_t)i * width + j];
      t->h_wtab[i * kBatchMaxWidth + j] = w;
      if (w != 0.0) cols |= 1u << j;
    }
  PR_HIP(hipMemcpyAsync(t->wtab.p, t->h_wtab, sizeof(t->h_wtab), hipMemcpyHostToDevice, s));
  const int64_t tiles = (V + kWave - 1) / kWave;
  int64_t grid = std::min<int64_t>((tiles + kMixWaves - 1) / kMixWaves, t->grid_max);
  if (grid_cap > 0) grid = std::min(grid, grid_cap);
  grid = std::max<int64_t>(grid, 1);
  if (timed) {
    if (!t->ev0) PR_HIP(hipEventCreate(&t->ev0));
    if (!t->ev1) PR_HIP(hipEventCreate(&t->ev1));
    PR_HIP(hipEventRecord(t->ev0, s));
  }
  switch (stride) {
    case 1: PR_TRY(launch_mix_in<1>(t, s, R, V, cols, (unsigned)grid)); break;
    case 2: PR_TRY(launch_mix_in<2>(t, s, R, V, cols, (unsigned)grid)); break;
    case 4: PR_TRY(launch_mix_in<4>(t, s, R, V, cols, (unsigned)grid)); break;
    case 8: PR_TRY(launch_mix_in<8>(t, s, R, V, cols, (unsigned)grid)); break;
    default: PR_TRY(launch_mix_in<16>(t, s, R, V, cols, (unsigned)grid)); break;
  }
  if (timed) PR_HIP(hipEventRecord(t->ev1, s));
  return PR_OK;
}

int check_weights(int n, const double *weights) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(weights[i])) return fail(PR_ERR_INVALID, "weights[" + std::to_string(i) + "] is not finite");
  return PR_OK;
}

}  // namespace

size_t batch_mix_bytes(const BatchMixState *t) {
  if (!t) return 0;
  return t->M.bytes + t->wtab.bytes + t->mask.bytes + btopk_state_bytes(t->sel);
}

void batch_mix_free(BatchMixState *t) {
  if (!t) return;
  btopk_state_free(t->sel);
  if (t->ev0) (void)hipEventDestroy(t->ev0);
  if (t->ev1) (void)hipEventDestroy(t->ev1);
  delete t;  // DevBufs free their memory
}

int batch_mix_check_topk(int64_t V, int width, int32_t n_mixes, const double *weights, const int32_t *n_exclude,
                         const int32_t *const *exclude, int32_t k, const int32_t *ids_out, const double *scores_out,
                         const int32_t *n_out) {
  if (!weights || !n_out) return fail(PR_ERR_INVALID, "NULL argument");
  if (n_mixes < 1 || n_mixes > kBatchMaxMixes) return fail(PR_ERR_INVALID, "n_mixes must be in [1, 16]");
  PR_TRY(check_weights(n_mixes * width, weights));
  if (k < 0) return fail(PR_ERR_INVALID, "k < 0");
  if (k > 0 && (!ids_out || !scores_out)) return fail(PR_ERR_INVALID, "NULL argument");
  if ((n_exclude == nullptr) != (exclude == nullptr))
    return fail(PR_ERR_INVALID, "n_exclude and exclude must both be given or both be NULL");
  if (!n_exclude) return PR_OK;
  std::vector<int32_t> tmp;
  for (int i = 0; i < n_mixes; ++i) {
    const int32_t n = n_exclude[i];
    const std::string who = "exclude[" + std::to_string(i) + "]";
    if (n < 0) return fail(PR_ERR_INVALID, "n_exclude[" + std::to_string(i) + "] < 0");
    if (n > 0 && !exclude[i]) return fail(PR_ERR_INVALID, who + " is NULL");
    for (int32_t e = 0; e < n; ++e)
      if (exclude[i][e] < 0 || exclude[i][e] >= V)
        return fail(PR_ERR_INVALID, who + "[" + std::to_string(e) + "] = " + std::to_string(exclude[i][e]) + " is outside [0, V)");
    try {
      tmp.assign(exclude[i], exclude[i] + n);
    } catch (const std::bad_alloc &) {
      return fail(PR_ERR_OOM, "host allocation failed");
    }
    std::sort(tmp.begin(), tmp.end());
    const auto dup = std::adjacent_find(tmp.begin(), tmp.end());
    if (dup != tmp.end()) return fail(PR_ERR_INVALID, "vertex " + std::to_string(*dup) + " is listed twice in " + who);
  }
  return PR_OK;
}

int batch_mix_check_get(int width, const double *weights, const double *scores_out) {
  if (!weights || !scores_out) return fail(PR_ERR_INVALID, "NULL argument");
  return check_weights(width, weights);
}

int batch_mix_topk(BatchMixState **state, int device, hipStream_t s, const double *R, int64_t V, int width, int stride,
                   int32_t n_mixes, const double *weights, const int32_t *n_exclude, const int32_t *const *exclude,
                   int32_t k, int64_t narrow_div, int64_t grid_cap, int32_t *ids_out, double *scores_out, int32_t *n_out,
                   int64_t *info) {
  PR_TRY(mix_state(state, device, V, n_mixes));
  BatchMixState *t = *state;
  PR_HIP(hipStreamSynchronize(s));  // the enqueued steps; and no earlier upload still reads a host copy
  int64_t n_excl[kBTopkMaxCols] = {0};
  bool any = false;
  for (int i = 0; i < n_mixes && n_exclude; ++i) {
    n_excl[i] = n_exclude[i];
    any = any || n_exclude[i] > 0;
  }
  if (any) {
    if (!t->mask.p) PR_TRY(t->mask.alloc(sizeof(uint16_t) * (size_t)V));
    try {
      t->h_mask.assign((size_t)V, 0);
    } catch (const std::bad_alloc &) {
      return fail(PR_ERR_OOM, "host allocation failed");
    }
    for (int i = 0; i < n_mixes; ++i)
      for (int32_t e = 0; e < n_exclude[i]; ++e) t->h_mask[(size_t)exclude[i][e]] |= (uint16_t)(1u << i);
    PR_HIP(hipMemcpyAsync(t->mask.p, t->h_mask.data(), sizeof(uint16_t) * (size_t)V, hipMemcpyHostToDevice, s));
  }
  PR_TRY(run_mix(t, s, R, V, width, stride, n_mixes, weights, grid_cap, info != nullptr));
  int32_t sel_info[4] = {0, 0, 0, -1};
  PR_TRY(btopk_select(&t->sel, device, s, t->M.as<double>(), V, n_mixes, t->stride_m, any ? t->mask.as<uint16_t>() : nullptr,
                      n_excl, k, narrow_div, ids_out, scores_out, n_out, info ? sel_info : nullptr));
  if (info) {
    float ms = 0.f;
    PR_HIP(hipEventElapsedTime(&ms, t->ev0, t->ev1));
    info[0] = sel_info[1];
    info[1] = sel_info[2];
    info[2] = (int64_t)((double)ms * 1e6);
    info[3] = btopk_kernel_ns(t->sel);
  }
  return PR_OK;
}

int batch_mix_get(BatchMixState **state, int device, hipStream_t s, const double *R, int64_t V, int width, int stride,
                  const double *weights, double *colbuf, double *scores_out) {
  PR_TRY(mix_state(state, device, V, 1));
  BatchMixState *t = *state;
  PR_HIP(hipStreamSynchronize(s));  // the enqueued steps; and no earlier upload still reads a host copy
  PR_TRY(run_mix(t, s, R, V, width, stride, 1, weights, 0, false));
  const double *col = t->M.as<double>();
  if (t->stride_m > 1) {
    hipLaunchKernelGGL(k_batch_mix_col, dim3(grid_for(V, kMixThreads, 4096)), dim3(kMixThreads), 0, s, V, t->stride_m,
                       t->M.as<double>(), colbuf);
    PR_HIP(hipGetLastError());
    col = colbuf;
  }
  if (V > 0) PR_HIP(hipMemcpyAsync(scores_out, col, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  PR_HIP(hipStreamSynchronize(s));
  return PR_OK;
}

}  // namespace pr
