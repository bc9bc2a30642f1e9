"""Top-K query: the device select (PageRankGraph.topk) against today's path (all ranks to the
host, then a host select), on the bench's R-MAT graph.

    python tools/topk_bench.py [--scale 26|20] [--repeats 7] [--timeout SECONDS]

Builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor 16,
interned on the device), runs 10 iterations, then for K in {10, 1000, 1 000 000} (capped at V)
times in one process, after a warm-up, the median of --repeats runs of
  * today's path: g.ranks() -- V doubles over PCIe and the host scatter -- then np.argpartition and
    an exact (rank desc, ID asc) ordering of the K; the g.ranks() share is reported separately;
  * g.topk(K).
It checks that both give the same IDs and the same rank bits, and prints for each K how many
vertices share the K-th rank value, the histogram passes of the select, and a byte model of its
device passes (12 bytes per row and row pass, 12 per compacted candidate and candidate pass, 12
per row for the emit pass; the candidate count is bounded by rows / 8 here, not measured).
One JSON line per K and a final summary line on stdout.  The measurement runs in one child
process under a time limit of its own; the first failure ends the run with a non-zero status.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pagerank-using-apache-spark_amd"))


def host_topk(r, k):
    """The exact host answer from the full vector: rank descending, ties by ID ascending."""
    V = r.shape[0]
    if k >= V:
        o = np.lexsort((np.arange(V), -r))
        return o.astype(np.int32), r[o]
    part = np.argpartition(r, V - k)[V - k:]
    kth = r[part].min()
    above = np.nonzero(r > kth)[0]
    ties = np.nonzero(r == kth)[0][: k - above.shape[0]]  # already in ID order
    above = above[np.lexsort((above, -r[above]))]
    ids = np.concatenate([above, ties]).astype(np.int32)
    return ids, r[ids]


def worker(a) -> int:
    import torch

    import sparky_hip
    from sparky_hip.workloads import generate

    t0 = time.perf_counter()
    wl = generate("rmat", scale=a.scale, edge_factor=16, device=0)
    V, E = wl.n_vertices, wl.n_edges
    g = sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True, n_edges=E,
                                 keep_canonical=False)
    del wl
    torch.cuda.empty_cache()
    rows = None
    print(f"# {V} vertices, {E} edges, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    g.reset()
    g.step(10)
    g.sync()
    out = np.zeros(V, np.float64)
    results = []
    for K in (10, 1000, 1_000_000):
        k = min(K, V)
        t_ranks, t_host, t_topk = [], [], []
        ref = got = None
        for rep in range(a.repeats + 1):  # the first is the warm-up
            t0 = time.perf_counter()
            r = g.ranks(out)
            t1 = time.perf_counter()
            ref = host_topk(r, k)
            t2 = time.perf_counter()
            got = g.topk(k)
            t3 = time.perf_counter()
            if rep:
                t_ranks.append(t1 - t0)
                t_host.append(t2 - t0)
                t_topk.append(t3 - t2)
        if not (np.array_equal(ref[0], got[0]) and np.array_equal(ref[1].view(np.uint64), got[1].view(np.uint64))):
            print(json.dumps({"k": k, "error": "topk and the host path disagree"}), flush=True)
            return 1
        _, _, info = g._topk_ex(k, 8)
        rows = g.info()["local_rows"] if rows is None else rows
        ms = lambda v: round(statistics.median(v) * 1e3, 3)  # noqa: E731
        model = 12 * rows * (info["row_passes"] + 1 + (1 if info["narrowed_at"] >= 0 else 0))
        res = {"scale": a.scale, "k": k, "tie_class_of_kth": int(np.sum(out == got[1][-1])),
               "today_ms": ms(t_host), "ranks_share_ms": ms(t_ranks), "topk_ms": ms(t_topk),
               "topk_min_ms": round(min(t_topk) * 1e3, 3), "repeats": a.repeats, "select": info,
               "row_pass_bytes_model": int(model), "cand_pass_bytes_bound": int(12 * (rows // 8) * info["cand_passes"]),
               "faster_than_ranks_share": ms(t_topk) < ms(t_ranks)}
        print(json.dumps(res), flush=True)
        results.append(res)
    ok = all(r["faster_than_ranks_share"] for r in results)
    print(json.dumps({"scale": a.scale, "vertices": V, "all_k_faster_than_ranks_share": ok}), flush=True)
    g.close()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scale", str(a.scale), "--repeats", str(a.repeats)]
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
