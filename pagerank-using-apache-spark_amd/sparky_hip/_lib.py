"""ctypes binding of libpagerank_hip (include/pagerank_hip.h).

This is what a Python host binds; the JVM host binds the same symbols through Panama FFM or
JNI.  The library is loaded from the in-tree build directory; there is no
fallback -- a missing or unloadable library raises immediately.
"""
from __future__ import annotations

import ctypes
import os
import sys

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
BUILD_DIR = os.path.join(os.path.dirname(_PKG_DIR), "build")
# PR_LIB_PATH: another build of the same library (A/B of two kernel versions on one box)
LIB_PATH = os.environ.get("PR_LIB_PATH") or os.path.join(BUILD_DIR, "libpagerank_hip.so")

ABI_VERSION = 2  # include/pagerank_hip.h PR_ABI_VERSION this binding was written against

PR_OK = 0
PR_ERR_INVALID = -1
PR_ERR_HIP = -2
PR_ERR_OOM = -3
PR_ERR_COMM = -4
PR_ERR_STATE = -5
PR_ERR_NODEVICE = -6

PR_DANGLING_LOCAL = 0
PR_DANGLING_NONE = 1
PR_INPUT_DEVICE = 2
PR_NO_CANONICAL = 4
PR_LAYOUT_FUSED = 8
PR_LAYOUT_SPLIT = 16

PR_VF_KEY, PR_VF_SINK, PR_VF_NOLINK, PR_VF_INDEG0 = 1, 2, 4, 8

INFO_NAMES = ["n_vertices", "n_edges", "n_sink", "n_nolink", "n_indeg0", "max_indeg", "local_rows",
              "local_edges", "part", "n_parts", "n_units", "n_long_rows", "device_bytes", "classes",
              "xchg_send", "xchg_recv", "partial_slots", "hot_slots", "epilogue", "gather_est",
              "walk_groups", "layout", "hot_cover_ppm", "code_bits", "hot_gather"]
# build options of pr_graph_create_ex (PR_BOPT_*), by the keyword PageRankGraph(options=...) takes
BUILD_OPTIONS = {"classes": 1, "hot_slots": 2, "exchange_allgather": 3, "xchg_chunks": 4, "hot_reserve": 5,
                 "epi_walk": 6, "epi_narrow": 7, "codes": 8, "pack_fused": 9, "xchg_sdma": 10,
                 "epi_order": 11}
STAT_NAMES = ["iters", "last_dc", "last_l1", "spmv_ms_mean", "spmv_launches", "iter_ms_mean",
              "build_ms", "exchange_ms_mean"]
PR_CB_RANKS = 1
PR_OPT_XCHG_CHUNKS = 1
PR_OPT_HOT_RESERVE = 2
PR_OPT_XCHG_IPC = 3
PR_OPT_XCHG_IPC_BLIT = 4
PR_OPT_HOT_GATHER = 5
PR_COMM_ID_BYTES = 128

# Every symbol include/pagerank_hip.h declares (checked by tests/test_abi.py).
EXPORTED = [
    "pr_abi_version", "pr_last_error", "pr_device_count", "pr_graph_create", "pr_graph_create_part",
    "pr_graph_create_ex",
    "pr_graph_info", "pr_graph_export_csr", "pr_run", "pr_reset", "pr_step", "pr_sync",
    "pr_get_ranks", "pr_set_timing", "pr_set_option", "pr_get_stats", "pr_comm_unique_id", "pr_graph_attach_comm",
    "pr_graph_destroy", "pr_gen_rmat", "pr_gen_er", "pr_gen_chunglu", "pr_intern_device", "pr_group_reset",
    "pr_group_step", "pr_group_sync", "pr_get_topk", "pr_group_topk", "pr_topk_merge",
    "pr_set_teleport", "pr_set_teleport_sparse",
    "pr_set_teleport_dangling", "pr_get_teleport_dangling", "pr_get_teleport_sum",
    "pr_batch_create", "pr_batch_set_teleport", "pr_batch_set_teleport_sparse", "pr_batch_reset", "pr_batch_step",
    "pr_batch_sync", "pr_batch_get_ranks", "pr_batch_get_norms", "pr_batch_get_topk", "pr_batch_info",
    "pr_batch_destroy", "pr_batch_set_exclude", "pr_batch_get_topk_all", "pr_batch_step_until",
    "pr_batch_reset_column", "pr_batch_step_until_any", "pr_batch_run_queue",
    "pr_batch_set_dangling", "pr_batch_get_dangling", "pr_batch_get_teleport_sums",
    "pr_batch_mix_topk", "pr_batch_mix_get",
]
# pr_batch_info, in order
BATCH_INFO_NAMES = ["width", "stride", "n_units", "n_long_rows", "device_bytes", "iters", "last_step_ns"]
BATCH_MAX_WIDTH = 16
BATCH_MAX_MIXES = 16  # PR_BATCH_MAX_MIXES
# pr_batch_set_dangling's modes (PR_BATCH_DANGLING_*), by the name PageRankBatch.set_dangling takes
PR_BATCH_DANGLING_UNIFORM = 0
PR_BATCH_DANGLING_TELEPORT = 1
BATCH_DANGLING_MODES = {"uniform": PR_BATCH_DANGLING_UNIFORM, "teleport": PR_BATCH_DANGLING_TELEPORT}
# pr_set_teleport_dangling's modes (PR_TELEPORT_DANGLING_*), by the name PageRankGraph.set_teleport_dangling takes
PR_TELEPORT_DANGLING_UNIFORM = 0
PR_TELEPORT_DANGLING_TELEPORT = 1
TELEPORT_DANGLING_MODES = {"uniform": PR_TELEPORT_DANGLING_UNIFORM, "teleport": PR_TELEPORT_DANGLING_TELEPORT}

ITER_CB = ctypes.CFUNCTYPE(None, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_double,
                           ctypes.c_double, ctypes.c_double, ctypes.c_void_p)


class BatchQuery(ctypes.Structure):
    """pr_batch_query (include/pagerank_hip.h): one entry of pr_batch_run_queue's queue."""
    _fields_ = [("n_seeds", ctypes.c_int32), ("ids", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("rest", ctypes.c_double), ("n_exclude", ctypes.c_int32), ("exclude", ctypes.c_void_p)]


# pr_batch_done_cb: query, column, iterations, converged, l1, user
BATCH_DONE_CB = ctypes.CFUNCTYPE(None, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                 ctypes.c_void_p)


class PageRankError(RuntimeError):
    """A non-zero status from libpagerank_hip (the JVM shim maps it to RuntimeException)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libpagerank_hip error {code}: {msg}")
        self.code = code


_lib = None
# Symbols that may be missing from the library PR_LIB_PATH names: a measuring tool that times an older
# build (tools/batch_queue_bench.py --baseline-lib) lists here, before load(), what that build lacks.
# load() then leaves them unbound; calling one still fails.  Empty in every other use.
OPTIONAL = set()


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 / librccl.so.1.  If
    # this library loaded /opt/rocm's copies first, the process would hold two HIP runtimes and
    # torch would see no GPU (and device pointers from one would be foreign to the other).
    # Loading torch first makes the loader resolve our NEEDED sonames to torch's copies: one
    # runtime per process.  Without torch installed, /opt/rocm's runtime is used.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `make -C pagerank-using-apache-spark_amd/csrc` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    i32, i64, u32, u64, dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    sig = {
        "pr_abi_version": ([], ctypes.c_int),
        "pr_last_error": ([], ctypes.c_char_p),
        "pr_device_count": ([P], ctypes.c_int),
        "pr_graph_create": ([i32, i32, i64, P, P, u32, P], ctypes.c_int),
        "pr_graph_create_part": ([i32, i32, i32, i32, i64, P, P, u32, P], ctypes.c_int),
        "pr_graph_create_ex": ([i32, i32, i32, i32, i64, P, P, u32, P, i32, P], ctypes.c_int),
        "pr_graph_info": ([P, P, i32], ctypes.c_int),
        "pr_graph_export_csr": ([P, P, P, P, P], ctypes.c_int),
        "pr_run": ([P, i32, dbl, dbl, P, P, ITER_CB, u32, P], ctypes.c_int),
        "pr_reset": ([P, dbl, dbl, P], ctypes.c_int),
        "pr_step": ([P, i32], ctypes.c_int),
        "pr_sync": ([P], ctypes.c_int),
        "pr_get_ranks": ([P, P], ctypes.c_int),
        "pr_set_timing": ([P, i32], ctypes.c_int),
        "pr_set_option": ([P, i32, i64], ctypes.c_int),
        "pr_get_stats": ([P, P, i32], ctypes.c_int),
        "pr_comm_unique_id": ([P], ctypes.c_int),
        "pr_graph_attach_comm": ([P, i32, i32, P], ctypes.c_int),
        "pr_graph_destroy": ([P], None),
        "pr_gen_rmat": ([i32, i32, i64, dbl, dbl, dbl, u64, P, P], ctypes.c_int),
        "pr_gen_er": ([i32, i32, i64, u64, P, P], ctypes.c_int),
        "pr_gen_chunglu": ([i32, i32, i64, dbl, dbl, dbl, dbl, dbl, i64, u64, P, P], ctypes.c_int),
        "pr_intern_device": ([i32, i64, i32, P, P, P], ctypes.c_int),
        "pr_group_reset": ([P, i32, dbl, dbl, P], ctypes.c_int),
        "pr_group_step": ([P, i32, i32], ctypes.c_int),
        "pr_group_sync": ([P, i32], ctypes.c_int),
        "pr_get_topk": ([P, i32, P, P, P], ctypes.c_int),
        "pr_group_topk": ([P, i32, i32, P, P, P], ctypes.c_int),
        "pr_topk_merge": ([i32, P, P, P, i32, P, P, P], ctypes.c_int),
        "pr_set_teleport": ([P, P], ctypes.c_int),
        "pr_set_teleport_sparse": ([P, i32, P, P, dbl], ctypes.c_int),
        "pr_set_teleport_dangling": ([P, i32], ctypes.c_int),
        "pr_get_teleport_dangling": ([P, P], ctypes.c_int),
        "pr_get_teleport_sum": ([P, P], ctypes.c_int),
        "pr_batch_create": ([P, i32, P], ctypes.c_int),
        "pr_batch_set_teleport": ([P, i32, P], ctypes.c_int),
        "pr_batch_set_teleport_sparse": ([P, i32, i32, P, P, dbl], ctypes.c_int),
        "pr_batch_reset": ([P, dbl, dbl, P], ctypes.c_int),
        "pr_batch_step": ([P, i32], ctypes.c_int),
        "pr_batch_sync": ([P], ctypes.c_int),
        "pr_batch_get_ranks": ([P, i32, P], ctypes.c_int),
        "pr_batch_get_norms": ([P, P, P], ctypes.c_int),
        "pr_batch_get_topk": ([P, i32, i32, P, P, P], ctypes.c_int),
        "pr_batch_info": ([P, P, i32], ctypes.c_int),
        "pr_batch_destroy": ([P], None),
        "pr_batch_set_exclude": ([P, i32, i32, P], ctypes.c_int),
        "pr_batch_get_topk_all": ([P, i32, P, P, P], ctypes.c_int),
        "pr_batch_step_until": ([P, i32, dbl, P], ctypes.c_int),
        # internal (not in the header): pr_get_topk / pr_batch_get_topk_all with the narrowing threshold
        # and the pass counts
        "pr_topk_select_ex": ([P, i32, i64, P, P, P, P], ctypes.c_int),
        "pr_batch_topk_all_ex": ([P, i32, i64, P, P, P, P], ctypes.c_int),
        "pr_batch_topk_all_kernel_ns": ([P, P], ctypes.c_int),  # HIP-event kernel time of the last _ex call
        # internal: pr_batch_step_until with the block size and the enqueued / executed iteration counts
        "pr_batch_step_until_ex": ([P, i32, dbl, i32, P, P], ctypes.c_int),
        "pr_batch_reset_column": ([P, i32, P], ctypes.c_int),
        "pr_batch_step_until_any": ([P, u32, i32, dbl, P, P], ctypes.c_int),
        # the callback as a plain pointer (ctypes.cast of a BATCH_DONE_CB), so that None is NULL
        "pr_batch_run_queue": ([P, i32, P, i32, dbl, P, P, P], ctypes.c_int),
        # internal: pr_batch_step_until_any with the block size and the enqueued / executed counts
        "pr_batch_step_until_any_ex": ([P, u32, i32, dbl, i32, P, P, P], ctypes.c_int),
        "pr_batch_set_dangling": ([P, i32], ctypes.c_int),
        "pr_batch_get_dangling": ([P, P], ctypes.c_int),
        "pr_batch_get_teleport_sums": ([P, P], ctypes.c_int),
        # internal: pr_batch_get_ranks for any column of the layout, [0, stride) -- the padding columns too
        "pr_batch_get_ranks_ex": ([P, i32, P], ctypes.c_int),
        # b, n_mixes, weights, n_exclude, exclude (an array of pointers), k, ids_out, scores_out, n_out
        "pr_batch_mix_topk": ([P, i32, P, P, P, i32, P, P, P], ctypes.c_int),
        "pr_batch_mix_get": ([P, P, P], ctypes.c_int),
        # internal: pr_batch_mix_topk with the select's narrowing divisor, a cap on the mix kernel's grid and info[4]
        "pr_batch_mix_topk_ex": ([P, i32, P, P, P, i32, P, P, P, i64, i64, P], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        if name in OPTIONAL and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    v = L.pr_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {v}; this binding needs {ABI_VERSION} (rebuild the library)")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != PR_OK:
        msg = load().pr_last_error()
        raise PageRankError(rc, msg.decode() if msg else "")
