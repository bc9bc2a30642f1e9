/*
 * libpagerank_hip -- C ABI of the MI355X (gfx950) PageRank engine that replaces the power
 * iteration of Sparky.java (mayursharma/PageRank-using-Apache-Spark).
 *
 * The reference has no plugin/FFI interface: its hot path is inline Spark transformations in
 * main() (Sparky.java:124-238).  This header is the drop-in boundary a JVM host binds through
 * Panama FFM or JNI.  Each entry point names the reference code it
 * replaces.  Plain pointers and sizes only; every function returns PR_OK (0) or a negative
 * PR_ERR_* code with a thread-local message in pr_last_error(); nothing throws across the ABI.
 *
 * Ownership: pointer inputs are caller-owned and borrowed only for the duration of the call.
 * Device memory is owned by the library and released by pr_graph_destroy().  Outputs are
 * caller-allocated.  A pr_graph handle is not re-entrant; distinct handles may be used from
 * distinct threads.
 *
 * Vertex IDs are dense int32 IDs produced by the host's URL interner (first appearance,
 * src before dst).  Every ID in [0, n_vertices) must appear in the edge list.  dst[i] == -1
 * marks a record without any type=="a" link (Sparky.java:114-118: "(url, null)").
 */
#ifndef PAGERANK_HIP_H
#define PAGERANK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PR_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------------------- */
#define PR_OK 0
#define PR_ERR_INVALID (-1)  /* bad argument / malformed edge list                        */
#define PR_ERR_HIP (-2)      /* HIP runtime failure                                        */
#define PR_ERR_OOM (-3)      /* device or host allocation failed                           */
#define PR_ERR_COMM (-4)     /* RCCL failure                                               */
#define PR_ERR_STATE (-5)    /* call not valid in the handle's current state               */
#define PR_ERR_NODEVICE (-6) /* no usable GPU                                              */

/* ---- graph creation flags ------------------------------------------------------------ */
#define PR_DANGLING_LOCAL 0u /* Spark local[N] semantics: D = sink-only vertices (default) */
#define PR_DANGLING_NONE 1u  /* cluster-mode semantics: dangUrls empty on the driver, dc=0 */
#define PR_INPUT_DEVICE 2u   /* src/dst are device pointers on `device` (not host)        */
#define PR_NO_CANONICAL 4u   /* drop the canonical CSR after the build (no export)        */
#define PR_LAYOUT_FUSED 8u   /* force the single-pass layout (default: chosen by size)    */
#define PR_LAYOUT_SPLIT 16u  /* force the per-XCD column-class layout                     */

/* ---- vertex flag bits (pr_graph_export_csr vflags) ---------------------------------- */
#define PR_VF_KEY 1u    /* vertex is a record key / src          Sparky.java:127-135      */
#define PR_VF_SINK 2u   /* target never seen as a record         Sparky.java:146-149      */
#define PR_VF_NOLINK 4u /* record whose only value is null       Sparky.java:114-118      */
#define PR_VF_INDEG0 8u /* no in-link: keeps its old rank as sum Sparky.java:224-225      */

/* ---- pr_graph_info indices ------------------------------------------------------------ */
#define PR_INFO_N_VERTICES 0   /* N = totalUrlCount (Sparky.java:162)                       */
#define PR_INFO_N_EDGES 1      /* E' = distinct edges (Sparky.java:124)                      */
#define PR_INFO_N_SINK 2       /* |D| in local mode (Sparky.java:172-184)                    */
#define PR_INFO_N_NOLINK 3     /* keys without links (their mass leaks)                     */
#define PR_INFO_N_INDEG0 4     /* vertices hit by the subtractByKey quirk                   */
#define PR_INFO_MAX_INDEG 5
#define PR_INFO_LOCAL_ROWS 6   /* rows owned by this part                                   */
#define PR_INFO_LOCAL_EDGES 7  /* in-links owned by this part                               */
#define PR_INFO_PART 8
#define PR_INFO_N_PARTS 9
#define PR_INFO_N_UNITS 10     /* work units of the SpMV launch                             */
#define PR_INFO_N_LONG_ROWS 11 /* rows split across several units                          */
#define PR_INFO_DEVICE_BYTES 12
#define PR_INFO_CLASSES 13     /* column classes of the layout (1 = fused single pass)     */
#define PR_INFO_XCHG_SEND 14   /* doubles this part sends per iteration (P > 1)           */
#define PR_INFO_XCHG_RECV 15   /* doubles this part receives per iteration (P > 1)        */
#define PR_INFO_PARTIAL_SLOTS 16 /* (row, column class) segment sums of the split layout     */
#define PR_INFO_HOT_SLOTS 17   /* LDS hot-set contributions per class (split layout)        */
#define PR_INFO_EPILOGUE 18    /* 0 fused units, 3 grouped (split)                           */
#define PR_INFO_GATHER_EST 19  /* bytes of the part's expected gather space (class policy)   */
#define PR_INFO_WALK_GROUPS 20 /* epilogue groups (8 x 64 rows) that walk their rows' own slots */
#define PR_INFO_LAYOUT 21      /* 0 fused, 1 split (column classes + partial slots)          */
#define PR_INFO_HOT_COVER 22   /* in-links read from the LDS hot sets, parts per million      */
#define PR_INFO_CODE_BITS 23   /* bits per in-link of the split layout's entry codes: 20 / 24 compact, 32 */
#define PR_INFO_HOT_GATHER 24  /* cold gathers of the next k_spmv_hot launch: 0 per position, 1 dense (PR_OPT_HOT_GATHER); 0 fused */
#define PR_INFO_COUNT 25

/* ---- pr_get_stats indices ------------------------------------------------------------- */
#define PR_STAT_ITERS 0          /* iterations run since the last reset                     */
#define PR_STAT_LAST_DC 1        /* danglingContrib used by the last iteration              */
#define PR_STAT_LAST_L1 2        /* sum |r_k - r_{k-1}| of the last iteration                */
#define PR_STAT_SPMV_MS_MEAN 3   /* mean HIP-event time of one SpMV pass, kernels only: exchange waits excluded (timing on);
                                    one part: the whole iteration (k_finalize included), one
                                    interval per pr_step call with no event between kernels */
#define PR_STAT_SPMV_LAUNCHES 4  /* SpMV passes timed */
#define PR_STAT_ITER_MS_MEAN 5   /* mean HIP-event time of a whole iteration, its exchange
                                    included (timing on)                                    */
#define PR_STAT_BUILD_MS 6       /* wall time of the graph build                            */
#define PR_STAT_EXCHANGE_MS_MEAN 7 /* mean time of the RCCL exchange (parts > 1)            */
#define PR_STAT_COUNT 8

typedef struct pr_graph pr_graph;

/* Per-iteration callback (runs on the calling thread between iterations).
 * ranks_or_null: V doubles in original-ID order when PR_CB_RANKS is set (else NULL);
 * for a part, only the part's own vertices are written, the rest hold the previous content. */
typedef void (*pr_iter_cb)(int32_t iter, const double *ranks_or_null, double dangling_sum,
                           double l1_delta, double ms, void *user);
#define PR_CB_RANKS 1u

int pr_abi_version(void);
const char *pr_last_error(void);
int pr_device_count(int32_t *out);

/* Graph construction: replaces Sparky.java:124-184 (distinct/groupByKey, key broadcast,
 * sink completion, union/count, dangling fixup).  Builds the canonical in-link CSR on the
 * GPU (radix sort + dedupe) and the internal degree-ordered layout used by the iteration.
 * src/dst: n_edges raw interned edges (duplicates and self-loops allowed, dst = -1 for a
 * record without links).  Host pointers unless PR_INPUT_DEVICE. */
int pr_graph_create(int32_t device, int32_t n_vertices, int64_t n_edges, const int32_t *src,
                    const int32_t *dst, uint32_t flags, pr_graph **out);

/* The same, keeping only the rows of `part` out of `n_parts` (1D row partition for one
 * process per GPU; 1 <= n_parts <= 64).  Every part must be created from the same edge list;
 * the part also derives which contributions it exchanges with every peer. */
int pr_graph_create_part(int32_t device, int32_t part, int32_t n_parts, int32_t n_vertices,
                         int64_t n_edges, const int32_t *src, const int32_t *dst, uint32_t flags,
                         pr_graph **out);

/* The same with build options: n_options (key, value) pairs of int64 in `options` (may be NULL
 * when n_options is 0).  They tune the layout (A/B, tests); results do not depend on them beyond
 * summation order.  An unknown key or an out-of-range value fails with PR_ERR_INVALID.  The library
 * reads no environment variables: every choice is an explicit option. */
#define PR_BOPT_CLASSES 1     /* column classes of the split layout: 0 (size policy), 8, 16, 32, 64, 128 */
#define PR_BOPT_HOT_SLOTS 2   /* LDS hot-set slots per class: -1 (default 18429) or 0..18429            */
#define PR_BOPT_EXCHANGE 3    /* P > 1: 0 per-peer runs (default), 1 whole-slice all-gather (all parts alike) */
#define PR_BOPT_XCHG_CHUNKS 4 /* P > 1: 1 = the overlapped exchange from the start (PR_OPT_XCHG_CHUNKS) */
#define PR_BOPT_HOT_RESERVE 5 /* CUs per XCD the heavy SpMV kernel leaves free, 0..3 (PR_OPT_HOT_RESERVE) */
#define PR_BOPT_EPI_WALK 6    /* split layout: 1 (default) per-row walk of sparse epilogue groups, 0 never */
#define PR_BOPT_EPI_NARROW 7  /* split layout: -1 auto (default), 0 four-wave, 1 one-wave epilogue workgroups */
#define PR_BOPT_CODES 8       /* split layout: -1 (default) compact entry codes where they fit (P = 1: 2.5 bytes
                                 for class regions < 2^19 positions, 3 bytes < 2^20; P = 2..8: piece codes,
                                 2.5 / 3 bytes when hot slots + a class's pieces < 2^19 / 2^20), 0 always
                                 4-byte codes; same sums either way (PR_INFO code_bits: 20 / 24 / 32) */
#define PR_BOPT_PACK_FUSED 9  /* P > 1 (per-peer runs, split layout): 1 (default) the epilogue writes the
                                 contributions every peer reads straight into the send runs, 0 a separate
                                 pack kernel gathers them after the pass; same values either way */
#define PR_BOPT_XCHG_SDMA 10  /* group path (pr_group_*, P > 1 per-peer runs): 0 (default) the runs move by
                                 device copies (ROCclr blit kernels on the CUs), 1 by the copy engines
                                 (hipMemcpyDeviceToDeviceNoCU), which leave k_spmv_hot every CU */
#define PR_BOPT_EPI_ORDER 11  /* split layout: the epilogue's dispatch order, -1 (default) auto: 2 for a
                                 part of a row partition (n_parts > 1), 0 for one part; 0 row order, 1 runs
                                 of 8 consecutive groups heaviest first (most partial slots; within each
                                 exchange chunk when the epilogue runs chunk by chunk), 2 single groups
                                 heaviest first; same sums either way */
int pr_graph_create_ex(int32_t device, int32_t part, int32_t n_parts, int32_t n_vertices, int64_t n_edges,
                       const int32_t *src, const int32_t *dst, uint32_t flags, const int64_t *options,
                       int32_t n_options, pr_graph **out);

/* info[i] for i < min(n_info, PR_INFO_COUNT). */
int pr_graph_info(const pr_graph *g, int64_t *info, int32_t n_info);

/* Canonical CSR (rows = dst, columns = src ascending, deduplicated) in original IDs, for
 * bit-exact tests.  row_ptr[V+1], col_idx[E'], out_deg[V], vflags[V]; any may be NULL. */
int pr_graph_export_csr(const pr_graph *g, int64_t *row_ptr, int32_t *col_idx, int32_t *out_deg,
                        uint8_t *vflags);

/* Whole job: replaces Sparky.java:164-238.  Resets ranks to init_ranks (NULL = 1.0 for every
 * vertex, Sparky.java:165-170), runs `iterations` steps of
 * r' = teleport + damping * (S + dc / N) and copies the final ranks (original-ID order, V
 * doubles) to ranks_out (may be NULL).  cb (may be NULL) is called after every iteration. */
int pr_run(pr_graph *g, int32_t iterations, double teleport, double damping,
           const double *init_ranks, double *ranks_out, pr_iter_cb cb, uint32_t cb_flags,
           void *user);

/* Lower-level stepping (resume from saved ranks, benchmarking).  pr_step enqueues work on
 * the library's stream and returns; pr_sync waits for it.  init_ranks (pr_run, pr_reset,
 * pr_group_reset): NULL (every rank 1.0, Sparky.java:165-170) or V doubles in original-ID
 * order; the library reads exactly V of them. */
int pr_reset(pr_graph *g, double teleport, double damping, const double *init_ranks);
int pr_step(pr_graph *g, int32_t iterations);
int pr_sync(pr_graph *g);
int pr_get_ranks(pr_graph *g, double *ranks_out);

/* Personalised (topic-sensitive) PageRank: a per-vertex teleport vector t in the scalar's place.
 * With a vector set, one iteration is r'[v] = t[v] + damping * (S[v] + dc / N), evaluated exactly
 * as the scalar form (rounded add and multiply, no contraction).  t holds the teleport *term
 * itself*, not a probability: a vector of all 0.15 gives ranks bitwise equal to the scalar run.
 * While a vector is set, the scalar `teleport` of pr_reset / pr_run / pr_group_reset is ignored;
 * `damping` still applies.  Everything else stays Sparky's: ranks are never normalised, S = r_old
 * for rows without in-links, and the dangling term is the uniform dc / N unless
 * pr_set_teleport_dangling (below) returns the dangling mass along t.
 * The vector is a property of the handle: it survives pr_reset and pr_run (which reset ranks
 * only), takes effect from the next iteration enqueued after the call, and is cleared by passing
 * NULL (back to the scalar).  Both calls wait for the enqueued steps, like pr_get_ranks, and are
 * valid any time after create, before or after pr_reset.  On a part the call is local, not
 * collective: the part keeps only the rows it owns, so callers of a group (pr_group_*) or of RCCL
 * ranks call it on every part with the same arguments.
 * The first set allocates 8 bytes per local row, counted in PR_INFO_DEVICE_BYTES from then until
 * pr_graph_destroy (NULL keeps the allocation); a handle that never sets a vector allocates
 * nothing and launches exactly the kernels of the scalar run.
 * Errors: a NULL graph, n < 0, NULL ids / values with n > 0, an ID outside [0, V), a duplicate
 * ID, or a non-finite value or `rest`: PR_ERR_INVALID (checked on the host before any device call);
 * an allocation failure: PR_ERR_OOM.  Nothing changes in either case. */
/* V doubles in original-ID order (this part keeps its own rows'), or NULL: back to the scalar. */
int pr_set_teleport(pr_graph *g, const double *teleport);
/* t[ids[i]] = values[i], every other vertex `rest`.  ids must be distinct and in [0, V). */
int pr_set_teleport_sparse(pr_graph *g, int32_t n, const int32_t *ids, const double *values, double rest);

/* Where the dangling mass goes while a teleport vector is set.  PR_TELEPORT_DANGLING_UNIFORM (the
 * default) is the iteration above, bit for bit.  PR_TELEPORT_DANGLING_TELEPORT returns it along the
 * vector, as textbook personalised PageRank does and as PR_BATCH_DANGLING_TELEPORT does for a batch
 * column: with ts = sum_v t[v],
 *     q     = dc / ts                               (one rounded divide, per launch)
 *     r'[v] = t[v] + damping * (S[v] + q * t[v])
 * every operation rounded on its own (no contraction); S, dc, the in-degree-0 rule, c' = r' / d, the
 * norms, the slots and the exchange are those of the uniform mode, and PR_STAT_LAST_DC and the
 * callback's dangling_sum stay dc.  With t = (0.15 N) p for a probability vector p the term is
 * dc * p[v]: the mass goes back to the seeds, and a vertex the seeds cannot reach drains towards 0.
 * ts runs over all V original IDs, not over a part's rows.  Every part forms it on the host from the
 * arguments of its own pr_set_teleport / pr_set_teleport_sparse call, in one fixed order: blocks of
 * 1024 consecutive IDs (the last one shorter), each summed sequentially in ID order from +0.0, the
 * block sums added sequentially in block order.  So ts depends on the vector and V only: it has the
 * same bits on every part, in every layout, and for a sparse set and the equal dense vector, and the
 * mode needs no communication beyond the exchange of the uniform mode.
 * Fallback, decided on the host when an iteration is enqueued: with the mode off, without a vector,
 * on a PR_DANGLING_NONE graph, or with a ts that is exactly 0 or not finite (a negative ts is
 * allowed), the handle launches exactly the kernels it launches without the mode.
 * The mode is a property of the handle, next to the vector: it survives pr_reset, pr_run, and
 * clearing and re-setting the vector.  pr_set_teleport_dangling waits for the enqueued steps, like
 * pr_set_teleport, is valid any time after create and takes effect from the next iteration
 * enqueued; it allocates no device memory (PR_INFO_DEVICE_BYTES does not move).  Like the vector it
 * is local, not collective: the parts of a group or of RCCL ranks are set alike.
 * pr_get_teleport_sum gives ts of the vector in force (0.0 without one), in either mode.
 * A NULL graph or output, or a mode other than the two constants: PR_ERR_INVALID, nothing changed. */
#define PR_TELEPORT_DANGLING_UNIFORM 0
#define PR_TELEPORT_DANGLING_TELEPORT 1
int pr_set_teleport_dangling(pr_graph *g, int32_t mode);
int pr_get_teleport_dangling(const pr_graph *g, int32_t *mode_out);
int pr_get_teleport_sum(pr_graph *g, double *sum_out);

/* Top-K query, selected on the device: the k highest-ranked vertices of this part (the rows it
 * owns; with one part, of the graph), rank descending, ties broken by original vertex ID
 * ascending.  Ranks compare by the order-preserving map of their IEEE-754 bits to a u64 (sign bit
 * set for a non-negative value, all bits inverted for a negative one: any finite or infinite
 * double works, -0.0 sorts just below +0.0; a NaN's position is unspecified).  Ties are exact: when
 * the k-th vertex falls inside a class of bit-identical ranks, the lowest IDs of that class are
 * returned.  Writes n = min(k, rows owned) pairs to ids_out / ranks_out (caller-allocated, k
 * entries each) and n to *n_out; the ranks are the bits pr_get_ranks returns for those IDs.  Only K
 * pairs cross to the host (pr_get_ranks copies and scatters all V).  Like pr_get_ranks the call
 * waits for the enqueued steps.  k < 0 or a NULL pointer: PR_ERR_INVALID; before pr_reset:
 * PR_ERR_STATE; k == 0: PR_OK with *n_out = 0.  The first call uploads the row -> original ID map
 * and allocates scratch (4 bytes per row + 12 per candidate and selected pair; PR_INFO_DEVICE_BYTES
 * counts them from then on); graphs that never ask pay nothing. */
int pr_get_topk(pr_graph *g, int32_t k, int32_t *ids_out, double *ranks_out, int32_t *n_out);
/* Pure host, needs no GPU: merges n_lists lists that are already in top-K order into the k best
 * (n = min(k, total entries)).  For one process per GPU (RCCL): every rank calls pr_get_topk on
 * its part and the host merges the lists it collects.  counts[l] entries in ids[l] / ranks[l]. */
int pr_topk_merge(int32_t n_lists, const int32_t *const *ids, const double *const *ranks,
                  const int32_t *counts, int32_t k, int32_t *ids_out, double *ranks_out, int32_t *n_out);
int pr_set_timing(pr_graph *g, int32_t enable);
int pr_get_stats(pr_graph *g, double *stats, int32_t n_stats);

/* Execution options (no effect on results; A/B and tuning).  PR_OPT_XCHG_CHUNKS: 1 = the
 * exchange of a part with peers travels in one chunk per SpMV phase and the next iteration's
 * phase c waits only for chunk c (overlap), 0 = whole runs (the default; PR_BOPT_XCHG_CHUNKS sets
 * it at build).  With RCCL every rank must make the same call (it is collective: the ranks check
 * that they agree, so a mismatch fails instead of hanging); in a group, set every part alike. */
#define PR_OPT_XCHG_CHUNKS 1
/* PR_OPT_HOT_RESERVE: CUs per XCD that the heavy SpMV kernel leaves free (0..3, default 0), for
 * the overlapped exchange's transfer kernels, which cannot share a CU with it (LDS, registers). */
#define PR_OPT_HOT_RESERVE 2
/* PR_OPT_XCHG_IPC (RCCL path, ranks on one node): 1 = every rank pulls the runs it reads straight
 * out of its peers' send buffers (IPC-mapped) with the copy engines, ordered by interprocess
 * events, so no transfer kernel takes a CU from the SpMV; 0 = RCCL send/recv (the default);
 * 2 = as 1, and the epilogue runs chunk by chunk, publishing each chunk's runs as soon as they are
 * written, so (with PR_OPT_XCHG_CHUNKS) a peer's pull of chunk c overlaps this rank's epilogue of
 * the later chunks (the split layout's fused pack with several chunks; otherwise as 1).
 * Collective like PR_OPT_XCHG_CHUNKS (which it combines with): every rank must pass the same value
 * (ranks that disagree all fail with PR_ERR_STATE, nothing changed); the first enable maps the
 * peers' buffers and fails with PR_ERR_COMM on every rank if any rank cannot. */
#define PR_OPT_XCHG_IPC 3
/* PR_OPT_XCHG_IPC_BLIT: how this rank's IPC pulls move the bytes: 0 = the copy engines
 * (hipMemcpyDeviceToDeviceNoCU, the default: no CU taken from the SpMV, but ~60 GB/s per engine),
 * 1 = the runtime's blit kernel on the CUs (link speed; it competes with the SpMV for CUs).  Local
 * to the rank (not collective); no effect on results. */
#define PR_OPT_XCHG_IPC_BLIT 4
/* PR_OPT_HOT_GATHER (test hook): how k_spmv_hot gathers a unit's cold entries: -1 = auto (the default:
 * dense gathers once a pass has enough wave units per CU, per-position gathers below), 0 = one gather
 * per entry position, 1 = dense gathers.  Both give the same bits; the option lets a small graph run
 * the path the size rule keeps for large ones.  Any other value: PR_ERR_INVALID.  Accepted without
 * effect on a handle of the fused layout (PR_INFO_CLASSES == 1).  PR_INFO_HOT_GATHER reports the path
 * the next launch takes. */
#define PR_OPT_HOT_GATHER 5
int pr_set_option(pr_graph *g, int32_t option, int64_t value);

/* Multi-process (one process per GPU): rank 0 creates an id, the host ships the 128 bytes
 * to every rank (any channel), every rank attaches it to its part.  Once per iteration each
 * part sends every peer exactly the contributions (and the two dangling/L1 slots) that the
 * peer's in-links read, with grouped RCCL ncclSend/ncclRecv over xGMI (PR_BOPT_EXCHANGE = 1:
 * one ncclAllGather of whole slices instead).  Attach cross-checks the per-peer run lengths. */
#define PR_COMM_ID_BYTES 128
int pr_comm_unique_id(uint8_t *id_out);
int pr_graph_attach_comm(pr_graph *g, int32_t rank, int32_t n_ranks, const uint8_t *id);

/* Single process, one host thread, n_parts parts (one per GPU -- or several on one GPU): the
 * parts exchange contributions by device-to-device copies (peer copies over xGMI between GPUs)
 * instead of RCCL.  parts[p] must be part p of n_parts, created from the same edge list.
 * Ranks: pr_get_ranks on every part (each fills its own vertices). */
int pr_group_reset(pr_graph *const *parts, int32_t n_parts, double teleport, double damping,
                   const double *init_ranks);
int pr_group_step(pr_graph *const *parts, int32_t n_parts, int32_t iterations);
int pr_group_sync(pr_graph *const *parts, int32_t n_parts);
/* pr_get_topk over a single-process group: every part's list, merged (pr_topk_merge). */
int pr_group_topk(pr_graph *const *parts, int32_t n_parts, int32_t k, int32_t *ids_out,
                  double *ranks_out, int32_t *n_out);

void pr_graph_destroy(pr_graph *g);

/* ---- batched personalised PageRank ---------------------------------------------------- */
/* A batch advances `width` (1..16) rank vectors over one graph together: every column j has its
 * own teleport vector and runs exactly the personalised iteration documented at pr_set_teleport,
 * r'_j[v] = t_j[v] + damping * (S_j[v] + dc_j / N) with rounded add / multiply / divide, S_j = r_old_j
 * for rows without in-links, dc_j = the sum of column j's ranks over the vertices the graph treats
 * as dangling (0 under PR_DANGLING_NONE), ranks never normalised.  The columns are stored
 * interleaved (stride = the next power of two >= width), so one pass streams the column indices
 * once for all of them and every gather fetches 8 * stride contiguous bytes.  A column without a
 * vector uses the scalar `teleport` of pr_batch_reset (the plain Sparky run); a column's vector
 * survives pr_batch_reset and is cleared by pr_batch_set_teleport(b, column, NULL).  Every sum has
 * a fixed order that depends on the graph and the stride only: two runs agree bitwise, a column's
 * bits do not depend on its position or on its neighbours.  Against pr_step with the same vector the
 * ranks agree to rounding (the orders of summation differ), not bitwise.
 * Scope (each an error, not a fallback): the graph must be a single part (n_parts == 1, not in a
 * pr_group_*, no communicator) and must have kept its canonical CSR (no PR_NO_CANONICAL), else
 * PR_ERR_STATE.  The batch runs over that canonical CSR in original IDs with kernels, a stream and
 * state of its own; it only reads the graph's buffers, so the graph's own iteration and its
 * PR_INFO_DEVICE_BYTES are unaffected (the batch reports its bytes through pr_batch_info).  The
 * batch borrows the graph: destroy the batch first.  A pr_batch handle is not re-entrant.
 * Errors of the setters match pr_set_teleport*: a NULL batch, a column outside [0, width), an ID
 * outside [0, V), a duplicate ID, a non-finite value: PR_ERR_INVALID, checked on the host before any
 * device call, nothing changed.  pr_batch_step / get_* before pr_batch_reset: PR_ERR_STATE. */
typedef struct pr_batch pr_batch;
int pr_batch_create(pr_graph *g, int32_t width, pr_batch **out); /* 1 <= width <= 16 */
/* V doubles in original-ID order, or NULL: back to the scalar.  Waits for the enqueued steps. */
int pr_batch_set_teleport(pr_batch *b, int32_t column, const double *teleport);
/* t[ids[i]] = values[i], every other vertex `rest`; bitwise the equivalent dense vector. */
int pr_batch_set_teleport_sparse(pr_batch *b, int32_t column, int32_t n, const int32_t *ids,
                                 const double *values, double rest);
/* init_ranks: NULL (1.0) or V doubles, used for every column. */
int pr_batch_reset(pr_batch *b, double teleport, double damping, const double *init_ranks);
/* Enqueues `iterations` iterations of every column; no host sync between iterations. */
int pr_batch_step(pr_batch *b, int32_t iterations);
/* Iterates until every column has converged or `max_iterations` iterations have run, deciding per
 * column on the device.  Every call starts with all `width` columns active.  After each iteration
 * a column whose L1 delta l1_j = sum_v |r'_j[v] - r_j[v]| (the value pr_batch_get_norms reports)
 * satisfies l1_j <= tol is frozen for the rest of the call: its ranks, contributions,
 * next-iteration dangling sum and L1 no longer change.  The test is absolute, on Sparky's
 * unnormalised ranks (they sum to about V, not to 1: scale tol accordingly), and a NaN L1 never
 * satisfies it; tol == 0 freezes a column only on an L1 of exactly 0.
 * iters_out (`width` entries, may be NULL): the iterations applied to column j in this call,
 * max_iterations for a column that did not converge.  Column j ends bitwise where
 * pr_batch_step(b, iters_out[j]) from the same state ends (a column's bits do not depend on its
 * neighbours), and pr_batch_get_norms afterwards reports per column the dc used by and the L1 of
 * that column's last applied iteration, bitwise those values too -- so l1_j <= tol says whether
 * column j converged.  The batch is left in an ordinary state: a later pr_batch_step(b, m) advances
 * every column, the frozen ones included, by m iterations.  pr_batch_info's iteration count grows
 * by the count of the column that advanced furthest.  Top-K queries and exclusions are unaffected.
 * The call is synchronous: it returns when the result is final.  Iterations are enqueued in blocks;
 * between iterations there is no host synchronisation except one read-back of a few words per
 * block, and once every column is frozen the rest of a block returns at kernel entry.  The result
 * does not depend on the block size.  The few words per column this needs on the device are part
 * of pr_batch_info's device bytes.
 * A NULL batch, max_iterations < 0, a tol that is NaN, negative or infinite: PR_ERR_INVALID, checked
 * before any device call; before pr_batch_reset: PR_ERR_STATE; max_iterations == 0: PR_OK, every
 * iters_out[j] == 0, nothing changes. */
int pr_batch_step_until(pr_batch *b, int32_t max_iterations, double tol, int32_t *iters_out);
/* Restarts column `column` alone: its ranks become init_ranks (NULL: 1.0; V doubles in original-ID
 * order), with the scalar teleport and damping of the last pr_batch_reset and the column's teleport
 * vector as it stands.  Afterwards the column holds bit for bit what it holds after pr_batch_reset
 * with the same arguments in a batch of the same width -- ranks, contributions, dangling sum (formed
 * in pr_batch_reset's order of summation) -- and every later iteration of it equals that batch's;
 * every other column, the padding included, is bitwise unaffected, now and later.  Valid at either
 * parity of the iteration count and after pr_batch_step or pr_batch_step_until* alike.
 * pr_batch_get_norms then reports for the column the dangling sum of init_ranks and an L1 of 0, the
 * other columns' norms unchanged.  pr_batch_info's iteration count does not move.  Waits for the
 * enqueued steps.  Like pr_batch_reset, the call does not check init_ranks for non-finite entries.
 * A NULL batch, a column outside [0, width): PR_ERR_INVALID; before pr_batch_reset: PR_ERR_STATE. */
int pr_batch_reset_column(pr_batch *b, int32_t column, const double *init_ranks);
/* pr_batch_step_until for the columns of the bit mask `active` only, ending at the first
 * convergence.  Columns outside `active` are frozen for the whole call, ranks and norms.  After
 * every iteration an active column with l1_j <= tol (pr_batch_step_until's test) has converged; the
 * call returns after the first iteration in which at least one did, else after max_iterations.
 * *executed_out: the iterations applied (the same for every active column); *converged_out: the
 * columns that converged in the last of them, 0 at the cap.  Every active column ends bitwise where
 * pr_batch_step(b, executed) would leave it; pr_batch_get_norms follows pr_batch_step_until's rules;
 * pr_batch_info's iteration count grows by `executed`.  Synchronous.  Iterations are enqueued in
 * blocks with one read-back per block; the device itself stops the rest of a block once a column
 * has converged (those launches return at kernel entry), and the result does not depend on the
 * block size.
 * A NULL batch or output, max_iterations < 0, a tol that is NaN, negative or infinite, an `active`
 * bit at or above width: PR_ERR_INVALID; before pr_batch_reset: PR_ERR_STATE; active == 0 or
 * max_iterations == 0: PR_OK, executed = 0, converged = 0, nothing changes. */
int pr_batch_step_until_any(pr_batch *b, uint32_t active, int32_t max_iterations, double tol,
                            int32_t *executed_out, uint32_t *converged_out);
/* A queue of seed sets served by the batch's `width` columns: a column whose query is done hands
 * over its result and starts the next query of the queue in the following iteration, while the
 * others carry on undisturbed.
 * A query is a sparse teleport vector (as pr_batch_set_teleport_sparse) and an exclusion set for its
 * top-K list (as pr_batch_set_exclude; n_exclude == 0: none).  Every query is checked on the host
 * by those calls' rules before any device call: one bad query fails the call with PR_ERR_INVALID
 * and changes nothing.  No table of V entries is built per query, and a refill moves 12 bytes per
 * seed to the device (plus one upload of the exclusion mask, 2 V bytes, for all the columns refilled
 * together, when one of their queries or of the queries they replace has a set).
 * Queries enter the columns in queue order (query q in column q for q < width).  A query starts
 * from pr_batch_reset_column(column, init_ranks) with its own vector and runs until l1 <= tol or
 * until it has had max_iterations iterations of its own.  When queries finish in an iteration,
 * `done` (may be NULL) runs for each on the calling thread in ascending column order: `iterations`
 * is the query's count, `converged` whether it met tol, `l1` its last L1.  The column still holds
 * the result: inside the callback, and only there, pr_batch_get_ranks, pr_batch_get_topk (it honours
 * the query's exclusion set) and pr_batch_get_norms may be called on the batch; every other call on
 * the handle returns PR_ERR_STATE.  Freed columns then take the next queries in order; with fewer
 * queries left than columns the spare columns do not iterate.  Returns when every query has been
 * reported.
 * A query's iteration count and rank bits do not depend on the column it ran in, on when it
 * started or on what ran beside it: they equal those of a fresh batch of the same width after
 * pr_batch_reset, the vector in column 0 and pr_batch_step(iterations).  The order of the callbacks
 * is a function of the queries' iteration counts, width and max_iterations only.
 * Afterwards the batch is in an ordinary state: pr_batch_step advances all columns; the columns keep
 * the teleport vectors and exclusion sets of the last queries they served (spare columns: what they
 * had before).
 * A NULL batch, n_queries < 0, NULL queries with n_queries > 0, max_iterations < 1, a bad tol:
 * PR_ERR_INVALID; before pr_batch_reset: PR_ERR_STATE; n_queries == 0: PR_OK. */
typedef struct pr_batch_query {
  int32_t n_seeds;
  const int32_t *ids;
  const double *values;
  double rest;
  int32_t n_exclude;
  const int32_t *exclude;
} pr_batch_query;
typedef void (*pr_batch_done_cb)(int32_t query, int32_t column, int32_t iterations, int32_t converged,
                                 double l1, void *user);
int pr_batch_run_queue(pr_batch *b, int32_t n_queries, const pr_batch_query *queries,
                       int32_t max_iterations, double tol, const double *init_ranks,
                       pr_batch_done_cb done, void *user);
/* Where a column's dangling mass goes.  PR_BATCH_DANGLING_UNIFORM (the default) is the iteration
 * above, bit for bit: every vertex receives dc_j / N.  PR_BATCH_DANGLING_TELEPORT returns the mass
 * along the column's teleport vector, as textbook personalised PageRank does: with
 * ts_j = sum_v t_j[v],
 *     q_j   = dc_j / ts_j                               (one rounded divide)
 *     r'[v] = t_j[v] + damping * (S_j[v] + q_j * t_j[v])
 * every operation rounded on its own (no contraction), S_j and dc_j exactly as in uniform mode.
 * With t = (0.15 N) p for a probability vector p the term is dc_j * p[v]: the mass goes back to the
 * seeds, and a vertex the seeds cannot reach keeps a rank of 0.  Everything else stays Sparky's:
 * unnormalised ranks, S = r_old for rows without in-links, the leak of no-link keys.
 * Fallback, per column: a column without a vector, a padding column, and a column whose ts_j is
 * exactly 0 or not finite use the uniform dc_j / N, bit for bit; a negative ts_j is allowed.  On a
 * PR_DANGLING_NONE graph dc is 0 and the mode has no effect (the uniform kernels run).
 * ts_j is formed on the device from the column of T in a fixed order that depends on V and the
 * stride only (pr_batch_reset_column's traversal and summation): a sparse set and the equal dense
 * vector give the same bits, as does the same vector in any column of a batch of the same stride,
 * and two runs agree.  It is brought up to date, for every column whose vector changed (set, clear,
 * queue refill, or the mode switched on), before the next teleport-mode iteration is enqueued and
 * before pr_batch_get_teleport_sums returns; with the mode off no existing call launches anything
 * for it.  The mode holds for pr_batch_step, pr_batch_step_until, pr_batch_step_until_any and
 * pr_batch_run_queue, and every statement made for them above stays true with "in the same mode"
 * added (a column's bits do not depend on its position or neighbours, step_until leaves column j
 * where step(iters_j) leaves it, a frozen column keeps its bits, a queue query equals a fresh batch
 * of the same width in the same mode).  pr_batch_reset, pr_batch_reset_column, the norms (dc used,
 * L1) and the top-K queries are the same in both modes.
 * pr_batch_set_dangling waits for the enqueued steps, is valid any time after create, survives
 * pr_batch_reset and takes effect from the next iteration enqueued.  The width doubles of ts are
 * allocated with the first use of the mode or of the getter and counted in pr_batch_info's device
 * bytes from then on.  The mode is the batch's: there is no per-column or per-query mode; the
 * engine's own iteration (pr_set_teleport, pr_step, pr_group_*) has the same choice per handle,
 * pr_set_teleport_dangling.
 * A NULL batch or output, a mode other than the two constants: PR_ERR_INVALID, nothing changed;
 * inside pr_batch_run_queue's callback: PR_ERR_STATE. */
#define PR_BATCH_DANGLING_UNIFORM 0
#define PR_BATCH_DANGLING_TELEPORT 1
int pr_batch_set_dangling(pr_batch *b, int32_t mode);
int pr_batch_get_dangling(const pr_batch *b, int32_t *mode_out);
/* ts_j of every column: width doubles; 0.0 for a column without a vector.  Synchronous. */
int pr_batch_get_teleport_sums(pr_batch *b, double *sums_out);
int pr_batch_sync(pr_batch *b);
/* Column `column`: V doubles in original-ID order.  Waits for the enqueued steps. */
int pr_batch_get_ranks(pr_batch *b, int32_t column, double *ranks_out);
/* `width` doubles each: per column the dc used by the last iteration and its L1 delta (after
 * pr_batch_step_until: of that column's own last applied iteration). */
int pr_batch_get_norms(pr_batch *b, double *dc_out, double *l_out);
/* pr_get_topk over one column (same order, same exact ties, same bits as pr_batch_get_ranks). */
int pr_batch_get_topk(pr_batch *b, int32_t column, int32_t k, int32_t *ids_out, double *ranks_out,
                      int32_t *n_out);
/* Per-column exclusions of the top-K queries.  A column's set names vertices that do not take part
 * in that column's lists; it affects pr_batch_get_topk and pr_batch_get_topk_all alike (the two never
 * disagree) and nothing else: the iteration, pr_batch_get_ranks and pr_batch_get_norms do not see
 * it, and a column without a set behaves bit for bit as before.  A set is valid any time after
 * create and survives pr_batch_reset.  With a set, column j yields min(k, V - |set_j|) pairs;
 * excluding every vertex gives 0 pairs and PR_OK.  Memory: one uint16_t per vertex (bit j = "left
 * out of column j"), allocated with the first non-empty set; an int32 per vertex with the first
 * pr_batch_get_topk of a column that has a set; the scratch of pr_batch_get_topk_all (histograms, the
 * candidate buffer and width * k output pairs at most) with its first non-empty result.  All of it
 * is counted in pr_batch_info's device bytes from then on and freed with the batch; a batch that
 * calls neither function allocates nothing for them.
 * Column `column` leaves out ids[0..n) from its top-K queries (both forms below). Replaces the column's
 * previous set; n == 0 (ids may be NULL) clears it.  Waits for the enqueued steps.  A NULL batch, a
 * column outside [0, width), n < 0, NULL ids with n > 0, an ID outside [0, V) or a duplicate ID:
 * PR_ERR_INVALID, checked on the host before any device call, nothing changed; PR_ERR_OOM when the
 * mask cannot be allocated. */
int pr_batch_set_exclude(pr_batch *b, int32_t column, int32_t n, const int32_t *ids);
/* pr_batch_get_topk for every column in one select: column j's list is ids_out / ranks_out[j*k .. j*k + n_out[j]),
 * n_out has `width` entries.  The order is pr_get_topk's (rank descending by the IEEE bits' order,
 * ties by original ID ascending, exact inside tie classes), the ranks are the bits
 * pr_batch_get_ranks returns, and every column's list equals pr_batch_get_topk(b, j, k, ...)'s in
 * IDs and rank bits.  All columns advance in lockstep over the interleaved rank matrix: one sweep
 * and one host synchronisation per radix pass for all of them.  k < 0, NULL n_out, NULL ids_out /
 * ranks_out with k > 0: PR_ERR_INVALID; before pr_batch_reset: PR_ERR_STATE; k == 0: PR_OK and
 * every n_out[j] == 0.  Waits for the enqueued steps. */
int pr_batch_get_topk_all(pr_batch *b, int32_t k, int32_t *ids_out, double *ranks_out, int32_t *n_out);
/* Batch mixes: top-K lists of weighted blends of the batch's columns, with no iteration.  The
 * iteration is linear in the teleport vector, so `width` computed columns (topics, single seeds, the
 * plain run) answer any number of weighted combinations of them; negative weights list what is
 * distinctive for a column (r_j - lambda * r_plain).
 * The blend.  Mix i scores every vertex by m_i[v], formed over the columns j = 0 .. width-1 in
 * ascending order under the weights w = weights[i*width .. (i+1)*width): a column whose weight is
 * exactly 0.0 (either sign) takes no part; the first participating column gives acc = w_j * r_j[v],
 * each later one acc = acc + w_j * r_j[v]; every product and every sum is rounded on its own (no
 * fused multiply-add); a mix with no non-zero weight scores every vertex +0.0.  So a one-hot mix
 * with weight 1.0 on column j is column j bit for bit, and a column driven to inf or NaN does not
 * touch a mix that gives it weight 0.  r_j is what pr_batch_get_ranks(b, j, ...) returns at that
 * moment; the mix does not care how the columns were produced (pr_batch_step, pr_batch_step_until,
 * pr_batch_run_queue, either dangling mode).  Reading a mix whose weights sum to 1 as "the PageRank
 * of the blended seeds" holds in PR_BATCH_DANGLING_UNIFORM (and under PR_DANGLING_NONE), for columns
 * run the same number of iterations from the same init_ranks or to their fixed points; it does not
 * hold in PR_BATCH_DANGLING_TELEPORT, whose dangling term is not linear in the teleport vector.
 * pr_batch_mix_topk: mix i's list is ids_out / scores_out[i*k .. i*k + n_out[i]) with n_out[i] =
 * min(k, V - n_exclude[i]); order, ties and the ordering of the IEEE bits are pr_get_topk's (score
 * descending, ties by original ID ascending, exact inside tie classes); the scores are the bits
 * pr_batch_mix_get returns for the same weights.  exclude[i][0 .. n_exclude[i]) are the vertices left
 * out of mix i's list (n_exclude and exclude both NULL: none); a mix's set is its own: the columns'
 * sets from pr_batch_set_exclude play no part, and those sets and every existing call are
 * unaffected.  Waits for the enqueued steps; only the selected pairs cross to the host.
 * pr_batch_mix_get: the dense blend of one mix (weights: width entries), V doubles in original-ID
 * order.
 * Errors.  A NULL batch, weights or n_out (scores_out for pr_batch_mix_get), n_mixes outside
 * [1, PR_BATCH_MAX_MIXES], a non-finite weight, k < 0, NULL ids_out / scores_out with k > 0, exactly
 * one of n_exclude / exclude NULL, n_exclude[i] < 0, NULL exclude[i] with n_exclude[i] > 0, an ID
 * outside [0, V), a duplicate ID within one set: PR_ERR_INVALID, all checked on the host before any
 * device call, nothing changed.  Before pr_batch_reset, or inside pr_batch_run_queue's callback:
 * PR_ERR_STATE.  k == 0: PR_OK and every n_out[i] == 0.
 * Memory.  The blends are materialised as a second interleaved matrix of V x stride_m doubles,
 * stride_m = the next power of two >= the largest n_mixes seen; a uint16_t per vertex (bit i = "left
 * out of mix i") once a mix has an exclusion set; the select over the blends has a scratch of its
 * own.  All of it is allocated on first use, counted in pr_batch_info's device bytes from then on
 * and freed with the batch; a batch that never mixes allocates nothing and launches nothing new. */
#define PR_BATCH_MAX_MIXES 16
int pr_batch_mix_topk(pr_batch *b, int32_t n_mixes, const double *weights /* n_mixes x width, row-major */,
                      const int32_t *n_exclude, const int32_t *const *exclude /* per mix; both NULL: none */,
                      int32_t k, int32_t *ids_out, double *scores_out, int32_t *n_out /* n_mixes */);
int pr_batch_mix_get(pr_batch *b, const double *weights /* width */, double *scores_out /* V */);
/* info[i] for i < min(n_info, 7): width, stride, work units, rows split over several units,
 * device bytes held by the batch, iterations done since the last reset, HIP-event time in ns of
 * the iterations of the last pr_batch_step call (-1: none yet, or they are still running). */
int pr_batch_info(const pr_batch *b, int64_t *info, int32_t n_info);
void pr_batch_destroy(pr_batch *b);

/* ---- synthetic inputs and device-side interning (benchmark front-end) ----------------- */
/* R-MAT (Graph500 parameters a,b,c, d = 1-a-b-c), n_edges edges over 2^scale labels, labels
 * scrambled by a seeded bijection.  d_src/d_dst: device arrays of n_edges int32. */
int pr_gen_rmat(int32_t device, int32_t scale, int64_t n_edges, double a, double b, double c,
                uint64_t seed, int32_t *d_src, int32_t *d_dst);
/* Uniform Erdos-Renyi G(n, m): src, dst uniform over 2^scale labels. */
int pr_gen_er(int32_t device, int32_t scale, int64_t n_edges, uint64_t seed, int32_t *d_src,
              int32_t *d_dst);
/* Chung-Lu graph with power-law weights (the LiveJournal- and Twitter-shaped
 * configs): n_edges edges whose source rank follows w(r) ~ (r + v0_out)^(-1/(gamma_out-1)) over
 * ranks [0, src_frac * n_labels) and whose target rank follows the same law with gamma_in, v0_in
 * over [0, n_labels); then n_nolink records (label, -1) for the ranks just past the source range
 * (keys without links).  Ranks map to labels by a seeded bijection of [0, n_labels).
 * d_src/d_dst: device arrays of n_edges + n_nolink int32. */
int pr_gen_chunglu(int32_t device, int32_t n_labels, int64_t n_edges, double gamma_out, double v0_out,
                   double gamma_in, double v0_in, double src_frac, int64_t n_nolink, uint64_t seed,
                   int32_t *d_src, int32_t *d_dst);
/* Relabel raw labels in [0, label_bound) to dense IDs in first-appearance order (src before
 * dst, edge by edge) -- the same mapping the host URL interner produces -- in place.
 * dst == -1 entries are kept.  *n_vertices_out = number of distinct labels. */
int pr_intern_device(int32_t device, int64_t n_edges, int32_t label_bound, int32_t *d_src,
                     int32_t *d_dst, int32_t *n_vertices_out);

#ifdef __cplusplus
}
#endif

#endif /* PAGERANK_HIP_H */
