"""Batched personalised PageRank on top of libpagerank_hip's pr_batch_* (include/pagerank_hip.h).

``PageRankBatch(graph, width)`` advances up to 16 rank vectors over one ``PageRankGraph`` together:
one pass streams the graph's column indices once for all of them.  Every column has its own
teleport vector (``set_teleport`` / ``set_teleport_sparse``; a column without one uses the scalar
of ``reset``) and runs exactly the iteration ``PageRankGraph.set_teleport`` documents.  The graph
must be a single part that kept its canonical CSR; the batch borrows it, so close the batch first
(the context manager does).  ``topk_all(k)`` returns every column's top-K list from one select over
all columns; ``set_exclude(column, ids)`` leaves vertices (a seed set, known items) out of a
column's lists.  ``step_until(max_iterations, tol)`` stops every column at its own convergence, decided
on the device.  ``run_queue(queries, max_iterations, tol)`` serves any number of seed sets through the
columns, refilling a column (``reset_column``) as soon as its query is done (``step_until_any``).
``set_dangling("teleport")`` returns every column's dangling mass along its own teleport vector
instead of spreading it over all vertices; ``teleport_sums()`` reports the vectors' sums it divides by.
``mix_topk(weights, k)`` returns the top-K lists of up to 16 weighted blends of the columns, formed and
selected on the device with no further iteration; ``mix(weights)`` returns one dense blend.
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

    def set_dangling(self, mode: str) -> None:
        """pr_batch_set_dangling: "uniform" (the default: every vertex receives dc_j / N) or "teleport"
        (column j's dangling mass returns along its teleport vector: the term is dc_j / ts_j * t_j[v]
        with ts_j = sum(t_j); a column without a vector, or whose vector sums to 0 or overflows, keeps
        the uniform term).  The batch's mode: it holds for step, step_until, step_until_any and
        run_queue from the next iteration on, and survives reset().  Waits for the enqueued steps."""
        if mode not in _lib.BATCH_DANGLING_MODES:
            raise ValueError('mode must be "uniform" or "teleport"')
        check(_lib.load().pr_batch_set_dangling(self._h, _lib.BATCH_DANGLING_MODES[mode]))

    @property
    def dangling(self) -> str:
        """The mode set_dangling() set: "uniform" or "teleport"."""
        m = ctypes.c_int32(0)
        check(_lib.load().pr_batch_get_dangling(self._h, ctypes.byref(m)))
        return next(k for k, v in _lib.BATCH_DANGLING_MODES.items() if v == m.value)

    def teleport_sums(self) -> np.ndarray:
        """pr_batch_get_teleport_sums: float64[width], the sum ts_j of every column's teleport vector
        as the device forms it (a fixed order; 0.0 for a column without a vector)."""
        out = np.zeros(self.width, np.float64)
        check(_lib.load().pr_batch_get_teleport_sums(self._h, _ptr(out)))
        return out

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

    def reset_column(self, column: int, init_ranks=None) -> None:
        """pr_batch_reset_column: restart one column (its teleport vector as it stands, the scalar
        teleport and damping of the last reset()); bitwise what reset() leaves in that column, the
        other columns untouched."""
        init = _init_array(init_ranks, self.n_vertices)
        check(_lib.load().pr_batch_reset_column(self._h, int(column), _ptr(init)))

    def step_until_any(self, active: int, max_iterations: int, tol: float):
        """pr_batch_step_until_any: iterate the columns of the bit mask ``active`` (the others are
        frozen) until the first iteration in which at least one of them has an L1 delta <= ``tol``, or
        ``max_iterations`` have run.  Returns (executed, converged_mask); the mask is 0 at the cap."""
        ex, conv = ctypes.c_int32(0), ctypes.c_uint32(0)
        check(_lib.load().pr_batch_step_until_any(self._h, int(active), int(max_iterations), float(tol),
                                                  ctypes.byref(ex), ctypes.byref(conv)))
        return ex.value, conv.value

    def _step_until_any_ex(self, active: int, max_iterations: int, tol: float, block: int):
        """The internal entry point behind step_until_any() with the number of iterations enqueued
        between two read-backs as a parameter.  Returns (executed, converged_mask, info) with
        info = (iterations enqueued, iterations executed).  For tests and tools/batch_queue_bench.py."""
        ex, conv, info = ctypes.c_int32(0), ctypes.c_uint32(0), np.zeros(2, np.int32)
        check(_lib.load().pr_batch_step_until_any_ex(self._h, int(active), int(max_iterations), float(tol), int(block),
                                                     ctypes.byref(ex), ctypes.byref(conv), _ptr(info)))
        return ex.value, conv.value, (int(info[0]), int(info[1]))

    def run_queue(self, queries, max_iterations: int, tol: float, *, k=None, init_ranks=None, on_done=None):
        """pr_batch_run_queue: serve ``queries`` -- a sequence of (ids, values), (ids, values, rest) or
        (ids, values, rest, exclude) -- through the batch's columns, refilling a column as soon as its
        query has converged (L1 <= ``tol``) or has had ``max_iterations`` iterations of its own.
        Returns one record per query, in queue order: a dict with ``iterations``, ``converged``, ``l1``,
        ``column`` and, when ``k`` is given, ``topk`` = (ids, ranks) of the query's top-``k`` list
        (its exclusion set left out).  ``on_done(query, column, record)`` runs as each query
        finishes, while the column still holds its result: it may call ``self.ranks(column)``,
        ``self.topk(column, k)`` and ``self.norms()``, nothing else on the batch."""
        keep, arr = [], (_lib.BatchQuery * max(len(queries), 1))()
        for n, q in enumerate(queries):
            if not 2 <= len(q) <= 4:
                raise ValueError("a query is (ids, values[, rest[, exclude]])")
            i, v = _sparse_arrays(q[0], q[1])
            x = np.zeros(0, np.int32) if len(q) < 4 or q[3] is None else np.ascontiguousarray(q[3], dtype=np.int32)
            if x.ndim != 1:
                raise ValueError("exclude must be a 1-D array")
            keep.append((i, v, x))
            arr[n] = _lib.BatchQuery(int(i.shape[0]), i.ctypes.data if i.shape[0] else None,
                                     v.ctypes.data if v.shape[0] else None, float(q[2]) if len(q) > 2 else 0.0,
                                     int(x.shape[0]), x.ctypes.data if x.shape[0] else None)
        init = _init_array(init_ranks, self.n_vertices)
        records, errors = [None] * len(queries), []

        def _cb(query, column, iterations, converged, l1, _user):
            try:
                rec = {"iterations": int(iterations), "converged": bool(converged), "l1": float(l1), "column": int(column)}
                if k is not None:
                    rec["topk"] = self.topk(column, k)
                records[query] = rec
                if on_done is not None and not errors:
                    on_done(int(query), int(column), rec)
            except BaseException as e:  # never unwind through the C frames
                errors.append(e)

        cb = _lib.BATCH_DONE_CB(_cb)
        check(_lib.load().pr_batch_run_queue(self._h, len(queries), ctypes.cast(arr, ctypes.c_void_p), int(max_iterations),
                                             float(tol), _ptr(init), ctypes.cast(cb, ctypes.c_void_p), None))
        if errors:
            raise errors[0]
        return records

    def sync(self) -> None:
        check(_lib.load().pr_batch_sync(self._h))

    # -- results -----------------------------------------------------------------------------
    def ranks(self, column: int) -> np.ndarray:
        out = np.zeros(max(self.n_vertices, 1), np.float64)
        check(_lib.load().pr_batch_get_ranks(self._h, int(column), _ptr(out)))
        return out[: self.n_vertices]

    def _ranks_ex(self, column: int) -> np.ndarray:
        """The library's internal entry point behind ranks() for any column of the layout, [0, stride):
        a padding column (>= width) holds zeros.  For tests."""
        out = np.zeros(max(self.n_vertices, 1), np.float64)
        check(_lib.load().pr_batch_get_ranks_ex(self._h, int(column), _ptr(out)))
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

    # -- mixes -------------------------------------------------------------------------------
    def _mix_weights(self, weights, one: bool) -> np.ndarray:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim == 1 and w.shape[0] == self.width:
            w = w.reshape(1, self.width)
        if w.ndim != 2 or w.shape[1] != self.width or (one and w.shape[0] != 1):
            raise ValueError("weights must have shape (width,)" + ("" if one else " or (n_mixes, width)"))
        return w

    def mix(self, weights) -> np.ndarray:
        """pr_batch_mix_get: float64[V], the blend sum_j weights[j] * ranks(j) as the device forms it
        (columns ascending, a weight of exactly 0 skipped, every product and sum rounded on its own)."""
        w = self._mix_weights(weights, True)
        out = np.zeros(max(self.n_vertices, 1), np.float64)
        check(_lib.load().pr_batch_mix_get(self._h, _ptr(w), _ptr(out)))
        return out[: self.n_vertices]

    def mix_topk(self, weights, k: int, exclude=None):
        """pr_batch_mix_topk: the top-``k`` lists of up to 16 weighted blends of the columns, selected on
        the device with no iteration.  ``weights``: (n_mixes, width) or (width,); ``exclude``: None, or
        per mix a sequence of vertex IDs left out of that mix's list (None or empty: none).  Returns a
        list of n_mixes pairs (ids int32[n_i], scores float64[n_i]) in ``topk``'s order; the scores are
        the bits ``mix`` returns for the same weights."""
        return self._mix_topk(weights, k, exclude, None)[0]

    def _mix_topk_ex(self, weights, k: int, exclude=None, *, narrow_div: int = 8, grid_cap: int = 0):
        """The library's internal entry point behind mix_topk(): the same query with the select's
        narrowing divisor (0: never) and a cap on the mix kernel's grid in workgroups (0: none).
        Returns (lists, info) with info = {matrix_passes, cand_passes, mix_ns, select_ns}.  For tests and
        tools/batch_mix_bench.py."""
        return self._mix_topk(weights, k, exclude, (int(narrow_div), int(grid_cap)))

    def _mix_topk(self, weights, k: int, exclude, ex):
        w = self._mix_weights(weights, False)
        m, k = int(w.shape[0]), int(k)
        n_ex, ptrs, keep = None, None, []
        if exclude is not None:
            if len(exclude) != m:
                raise ValueError("exclude needs one entry per mix")
            n_ex, ptrs = np.zeros(m, np.int32), (ctypes.c_void_p * m)()
            for i, ids in enumerate(exclude):
                x = np.zeros(0, np.int32) if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
                if x.ndim != 1:
                    raise ValueError("an exclusion set must be a 1-D array")
                keep.append(x)
                n_ex[i] = x.shape[0]
                ptrs[i] = x.ctypes.data if x.shape[0] else None
        ids, sc = np.zeros(max(k, 1) * m, np.int32), np.zeros(max(k, 1) * m, np.float64)
        n = np.zeros(m, np.int32)
        info = np.zeros(4, np.int64)
        L = _lib.load()
        head = (self._h, m, _ptr(w), _ptr(n_ex) if n_ex is not None else None,
                ctypes.cast(ptrs, ctypes.c_void_p) if ptrs is not None else None, k, _ptr(ids), _ptr(sc), _ptr(n))
        if ex is None:
            check(L.pr_batch_mix_topk(*head))
        else:
            check(L.pr_batch_mix_topk_ex(*head, ex[0], ex[1], _ptr(info)))
        lists = [(ids[i * k: i * k + int(n[i])].copy(), sc[i * k: i * k + int(n[i])].copy()) for i in range(m)]
        return lists, dict(zip(("matrix_passes", "cand_passes", "mix_ns", "select_ns"), (int(x) for x in info)))

    def info(self) -> dict:
        a = np.zeros(len(_lib.BATCH_INFO_NAMES), np.int64)
        check(_lib.load().pr_batch_info(self._h, _ptr(a), len(a)))
        return dict(zip(_lib.BATCH_INFO_NAMES, (int(x) for x in a)))
