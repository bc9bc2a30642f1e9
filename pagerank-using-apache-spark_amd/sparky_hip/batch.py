"""Batched personalised PageRank on top of libpagerank_hip's pr_batch_* (include/pagerank_hip.h).

``PageRankBatch(graph, width)`` advances up to 16 rank vectors over one ``PageRankGraph`` together:
one pass streams the graph's column indices once for all of them.  Every column has its own
teleport vector (``set_teleport`` / ``set_teleport_sparse``; a column without one uses the scalar
of ``reset``) and runs exactly the iteration ``PageRankGraph.set_teleport`` documents.  The graph
must be a single part that kept its canonical CSR; the batch borrows it, so close the batch first
(the context manager does).  ``topk_all(k)`` returns every column's top-K list from one select over
all columns; ``set_exclude(column, ids)`` leaves vertices (a seed set, known items) out of a
column's lists.  ``step_until(max_iterations, tol)`` stops every column at its own convergence, decided
on the device.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .graph import PageRankGraph, _init_array, _ptr, _sparse_arrays, _teleport_array


class PageRankBatch:
    """One ``pr_batch`` handle: ``width`` personalised runs over ``graph``, stepped together."""

    def __init__(self, graph: PageRankGraph, width: int):
        self._h = ctypes.c_void_p()
        self._graph = graph  # keeps the borrowed graph alive
        self.n_vertices = graph.n_vertices
        self.width = int(width)
        check(_lib.load().pr_batch_create(graph._h, self.width, ctypes.byref(self._h)))

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib.load().pr_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- teleport vectors --------------------------------------------------------------------
    def set_teleport(self, column: int, teleport) -> None:
        """pr_batch_set_teleport: float64[V] in original-ID order (the teleport *term* of every
        vertex), or None: the column is back to the scalar of reset().  Survives reset()."""
        t = _teleport_array(teleport, self.n_vertices)
        check(_lib.load().pr_batch_set_teleport(self._h, int(column), _ptr(t)))

    def set_teleport_sparse(self, column: int, ids, values, rest: float = 0.0) -> None:
        """pr_batch_set_teleport_sparse: t[ids[i]] = values[i], every other vertex ``rest``."""
        i, v = _sparse_arrays(ids, values)
        check(_lib.load().pr_batch_set_teleport_sparse(self._h, int(column), int(i.shape[0]), _ptr(i), _ptr(v),
                                                       float(rest)))

    # -- iteration ---------------------------------------------------------------------------
    def reset(self, *, teleport: float = 0.15, damping: float = 0.85, init_ranks=None) -> None:
        init = _init_array(init_ranks, self.n_vertices)
        check(_lib.load().pr_batch_reset(self._h, teleport, damping, _ptr(init)))

    def step(self, iterations: int) -> None:
        check(_lib.load().pr_batch_step(self._h, int(iterations)))

    def step_until(self, max_iterations: int, tol: float) -> np.ndarray:
        """pr_batch_step_until: iterate until every column's L1 delta is at most ``tol`` (absolute, on
        the unnormalised ranks) or ``max_iterations`` have run; a column that gets there is frozen on
        the device for the rest of the call, bitwise where ``step(iters[j])`` would leave it.
        Returns int32[width], the iterations applied to each column (``max_iterations``: not
        converged; ``norms()`` then shows its L1 above ``tol``).  Synchronous."""
        iters = np.zeros(self.width, np.int32)
        check(_lib.load().pr_batch_step_until(self._h, int(max_iterations), float(tol), _ptr(iters)))
        return iters

    def _step_until_ex(self, max_iterations: int, tol: float, block: int):
        """The library's internal entry point behind step_until(): the same call with the number of
        iterations enqueued between two read-backs as a parameter.  Returns (iters, info) with
        info = (iterations enqueued, iterations executed).  For tests and tools/batch_until_bench.py."""
        iters, info = np.zeros(self.width, np.int32), np.zeros(2, np.int32)
        check(_lib.load().pr_batch_step_until_ex(self._h, int(max_iterations), float(tol), int(block), _ptr(iters),
                                                 _ptr(info)))
        return iters, (int(info[0]), int(info[1]))

    def sync(self) -> None:
        check(_lib.load().pr_batch_sync(self._h))

    # -- results -----------------------------------------------------------------------------
    def ranks(self, column: int) -> np.ndarray:
        out = np.zeros(max(self.n_vertices, 1), np.float64)
        check(_lib.load().pr_batch_get_ranks(self._h, int(column), _ptr(out)))
        return out[: self.n_vertices]

    def norms(self):
        """(dc, l1): float64[width] each -- per column the dangling sum the last iteration used and
        the L1 distance it moved the ranks (after step_until: of each column's own last iteration)."""
        dc, l1 = np.zeros(self.width, np.float64), np.zeros(self.width, np.float64)
        check(_lib.load().pr_batch_get_norms(self._h, _ptr(dc), _ptr(l1)))
        return dc, l1

    def topk(self, column: int, k: int):
        """pr_batch_get_topk: PageRankGraph.topk over one column; (ids int32[n], ranks float64[n])."""
        k = int(k)
        ids, rk = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        n = ctypes.c_int32(0)
        check(_lib.load().pr_batch_get_topk(self._h, int(column), k, _ptr(ids), _ptr(rk), ctypes.byref(n)))
        return ids[: n.value], rk[: n.value]

    def set_exclude(self, column: int, ids) -> None:
        """pr_batch_set_exclude: the vertices ``ids`` do not take part in ``column``'s top-K lists
        (``topk`` and ``topk_all`` alike); replaces the column's previous set, an empty ``ids`` (or
        None) clears it.  Ranks, norms and the iteration never see it; it survives reset()."""
        i = np.zeros(0, np.int32) if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        if i.ndim != 1:
            raise ValueError("ids must be a 1-D array")
        check(_lib.load().pr_batch_set_exclude(self._h, int(column), int(i.shape[0]), _ptr(i) if i.shape[0] else None))

    def topk_all(self, k: int):
        """pr_batch_get_topk_all: every column's top-K from one lockstep select; a list of ``width``
        pairs (ids int32[n_j], ranks float64[n_j]), each equal to ``topk(j, k)``."""
        return self._topk_all(k, None)[0]

    def _topk_all_ex(self, k: int, narrow_div: int):
        """The library's internal entry point behind topk_all(): the same query with the narrowing
        divisor as a parameter (the candidates are compacted once the active columns hold at most
        V * width / narrow_div together; 0: never).  Returns (lists, info) with info = {passes,
        matrix_passes, cand_passes, narrowed_at, kernel_ns}.  For tests and tools/batch_topk_bench.py."""
        return self._topk_all(k, int(narrow_div))

    def _topk_all(self, k: int, narrow_div):
        k = int(k)
        ids, rk = np.zeros(max(k, 1) * self.width, np.int32), np.zeros(max(k, 1) * self.width, np.float64)
        n = np.zeros(self.width, np.int32)
        info = np.zeros(4, np.int32)
        L = _lib.load()
        if narrow_div is None:
            check(L.pr_batch_get_topk_all(self._h, k, _ptr(ids), _ptr(rk), _ptr(n)))
        else:
            check(L.pr_batch_topk_all_ex(self._h, k, narrow_div, _ptr(ids), _ptr(rk), _ptr(n), _ptr(info)))
        lists = [(ids[j * k: j * k + int(n[j])].copy(), rk[j * k: j * k + int(n[j])].copy()) for j in range(self.width)]
        out = dict(zip(("passes", "matrix_passes", "cand_passes", "narrowed_at"), (int(x) for x in info)))
        if narrow_div is not None:  # the summed HIP-event time of the call's kernels (-1: it launched none)
            ns = ctypes.c_int64(-1)
            check(L.pr_batch_topk_all_kernel_ns(self._h, ctypes.byref(ns)))
            out["kernel_ns"] = ns.value
        return lists, out

    def info(self) -> dict:
        a = np.zeros(len(_lib.BATCH_INFO_NAMES), np.int64)
        check(_lib.load().pr_batch_info(self._h, _ptr(a), len(a)))
        return dict(zip(_lib.BATCH_INFO_NAMES, (int(x) for x in a)))
