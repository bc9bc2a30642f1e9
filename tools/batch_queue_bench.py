"""pr_batch_run_queue against waves of 16, on the bench's R-MAT graphs, one GPU.

    python tools/batch_queue_bench.py [--scales 22] [--queries 128] [--tol 1e-6] [--cap 400] [--top 100]
                                      [--repeats 3] [--blocks 1,4,8,16,32] [--baseline-lib PATH]
                                      [--out FILE] [--timeout SECONDS]

Workload: Q single-seed and few-seed queries (one to three seeds, fixed RNG) whose masses span two
and a half decades around V, so that their convergence counts spread.  Per scale, with a width-16
batch over the graph bench.py times (seeded R-MAT, edge factor 16, canonical CSR kept):
  (a) queue:  run_queue(queries, cap, tol, k=top) -- the column of a finished query is refilled at once;
  (b) waves:  what a caller had before: per wave of 16 queries set_teleport_sparse x 16, reset(),
      step_until(cap, tol), topk_all(top).  With --baseline-lib PATH a second child process times
      (b) on that build of libpagerank_hip.so (the parent commit's), which is the baseline the
      ratios use; without it (b) runs on the current build only.
Per variant: wall time (host clock around synchronous calls; --repeats runs after a warm-up; median,
minimum, maximum), iterations executed, and the time outside iterations = wall - executed x the
per-iteration time of step() at this width (HIP events over 20 iterations).  Also:
  predicted ratio  sum of the waves' slowest counts / the queue schedule's iterations, both from the
                   per-query counts alone (the schedule from the host model of pr_batch_queue.h);
  refill           run_queue over 16 queries with a cap of one iteration, minus that iteration,
                   per query (teleport set on the device + reset_column; no column holds an
                   exclusion set), the same with exclusion sets of 10 IDs per query (one upload of
                   the 2 V-byte mask for the 16 columns refilled together; the difference of the two
                   medians x 16 is that upload), against set_teleport_sparse's dense path;
  blocks           the first 32 queries through a Python copy of the scheduler that calls
                   _step_until_any_ex with every block size of --blocks.
One JSON line per scale and child on stdout.  --out gets one list: per scale the current build's
record, then the baseline's (without the per-query counts, which `baseline_counts_equal` compares
with the current build's).  Each child runs under a time limit of its own; the first failure ends
the run with a non-zero status.
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
NEW_SYMBOLS = ("pr_batch_reset_column", "pr_batch_step_until_any", "pr_batch_run_queue", "pr_batch_step_until_any_ex")
W = 16


def make_queries(V, n):
    rng = np.random.default_rng(12345)
    qs = []
    for q in range(n):
        k = int(rng.integers(1, 4))
        ids = rng.choice(V, k, replace=False).astype(np.int32)
        mass = 0.15 * V * 10.0 ** rng.uniform(-1.0, 1.5)
        qs.append((ids, mass * (1.0 + np.arange(k)) / k, 0.0))
    return qs


def schedule_iterations(need, width, cap):
    """The queue schedule's total iterations for per-query counts `need` (> cap: never converges)."""
    slot, age, nxt, done, total = [None] * width, [0] * width, 0, 0, 0
    while done < len(need):
        for j in range(width):
            if slot[j] is None and nxt < len(need):
                slot[j], age[j] = nxt, 0
                nxt += 1
        occ = [j for j in range(width) if slot[j] is not None]
        n = min(min(cap - age[j] for j in occ), min(need[slot[j]] - age[j] for j in occ))
        total += n
        for j in occ:
            age[j] += n
            if age[j] == need[slot[j]] or age[j] >= cap:
                slot[j] = None
                done += 1
    return total


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def waves(b, queries, a):
    """Variant (b).  Returns (per-query counts, iterations executed)."""
    counts, executed = [], 0
    for w0 in range(0, len(queries), W):
        wave = queries[w0:w0 + W]
        for j, (ids, values, rest) in enumerate(wave):
            b.set_teleport_sparse(j, ids, values, rest)
        b.reset()
        it = b.step_until(a.cap, a.tol)
        b.topk_all(a.top)
        counts += [int(x) for x in it[:len(wave)]]
        executed += int(it[:len(wave)].max())  # spare columns of a last, short wave keep their old vectors
    return counts, executed


def py_queue(b, queries, a, block):
    """The scheduler in Python over _step_until_any_ex, for the block-size sweep."""
    slot, age, nxt, done, executed, enqueued = [None] * W, [0] * W, 0, 0, 0, 0
    while done < len(queries):
        for j in range(W):
            if slot[j] is None and nxt < len(queries):
                b.set_teleport_sparse(j, *queries[nxt])
                b.reset_column(j)
                slot[j], age[j] = nxt, 0
                nxt += 1
        occ = [j for j in range(W) if slot[j] is not None]
        n, conv, info = b._step_until_any_ex(sum(1 << j for j in occ), min(a.cap - age[j] for j in occ), a.tol, block)
        executed += n
        enqueued += info[0]
        for j in occ:
            age[j] += n
            if (conv >> j) & 1 or age[j] >= a.cap:
                slot[j] = None
                done += 1
    return executed, enqueued


def measure(b, V, a, new_lib):
    queries = make_queries(V, a.queries)
    res = {}
    b.reset()
    b.step(3)
    b.step_until(3, 0.0)
    ev = []
    for _ in range(a.repeats):
        b.reset()
        b.step(20)
        b.sync()
        ev.append(b.info()["last_step_ns"] * 1e-6 / 20)
    iter_ms = statistics.median(ev)
    res["step_ms_per_iter"] = spread(ev)
    t_w, t_q = [], []
    for rep in range(a.repeats + 1):  # the first round is the warm-up; the variants alternate
        ms, (counts_w, ex_w) = timed(lambda: waves(b, queries, a))
        if rep:
            t_w.append(ms)
        if new_lib:
            b.reset()
            ms, recs = timed(lambda: b.run_queue(queries, a.cap, a.tol, k=a.top))
            if rep:
                t_q.append(ms)
    res.update({"waves_ms": spread(t_w), "waves_iterations": ex_w,
                "waves_outside_ms": round(statistics.median(t_w) - ex_w * iter_ms, 3), "counts": counts_w})
    if not new_lib:
        return res
    counts_q = [r["iterations"] for r in recs]
    need = [r["iterations"] if r["converged"] else a.cap + 1 for r in recs]
    ex_q = schedule_iterations(need, W, a.cap)
    res.update({"queue_ms": spread(t_q), "queue_iterations": ex_q,
                "queue_outside_ms": round(statistics.median(t_q) - ex_q * iter_ms, 3),
                "counts_equal_waves": counts_q == counts_w,
                "predicted_waves_over_queue": round(ex_w / ex_q, 4),
                "measured_waves_over_queue_this_build": round(statistics.median(t_w) / statistics.median(t_q), 4)})
    # the cost of a refill
    rng = np.random.default_rng(1)
    first = queries[:W]
    with_ex = [q + (rng.choice(V, 10, replace=False).astype(np.int32),) for q in first]
    t_plain, t_ex, t_dense = [], [], []

    def clear_sets():  # reset() keeps the exclusion sets: a run that follows must not pay for clearing them
        for j in range(W):
            b.set_exclude(j, None)

    for _ in range(a.repeats + 1):
        clear_sets()
        b.reset()
        t_plain.append(timed(lambda: b.run_queue(first, 1, a.tol))[0])
        b.reset()  # no column has a set here, so every refill below stores one
        t_ex.append(timed(lambda: b.run_queue(with_ex, 1, a.tol))[0])
        t_dense.append(timed(lambda: b.set_teleport_sparse(0, *first[0]))[0])
    clear_sets()
    res["refill_ms_per_query"] = round((statistics.median(t_plain[1:]) - iter_ms) / W, 4)
    res["refill_with_exclusions_ms_per_query"] = round((statistics.median(t_ex[1:]) - iter_ms) / W, 4)
    res["refill_round_ms"] = spread(t_plain[1:])
    res["refill_round_with_exclusions_ms"] = spread(t_ex[1:])
    res["exclusion_mask_upload_ms"] = round(statistics.median(t_ex[1:]) - statistics.median(t_plain[1:]), 4)
    res["dense_set_teleport_sparse_ms"] = spread(t_dense[1:])
    # the block size
    blocks = {}
    for blk in a.blocks:
        t, out = [], None
        for _ in range(a.repeats):
            b.reset()
            ms, out = timed(lambda: py_queue(b, queries[:32], a, blk))
            t.append(ms)
        blocks[str(blk)] = {"ms": spread(t), "executed": out[0], "enqueued": out[1]}
    res["blocks_first_32_queries"] = blocks
    return res


def worker(a) -> int:
    new_lib = not a.old_lib
    import torch

    import sparky_hip
    if a.old_lib:  # a build from before this feature: the binding leaves the symbols it lacks unbound
        sparky_hip._lib.OPTIONAL.update(NEW_SYMBOLS)
    from sparky_hip.workloads import generate

    results = []
    for scale in a.scales:
        t0 = time.perf_counter()
        wl = generate("rmat", scale=scale, edge_factor=16, device=0)
        V, E = wl.n_vertices, wl.n_edges
        g = sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True, n_edges=E)
        del wl
        torch.cuda.empty_cache()
        print(f"# scale {scale}: {V} vertices, {E} edges, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr,
              flush=True)
        with sparky_hip.PageRankBatch(g, W) as b:
            res = measure(b, V, a, new_lib)
        res = {"scale": scale, "vertices": V, "edges": g.info()["n_edges"], "width": W, "queries": a.queries,
               "tol": a.tol, "cap": a.cap, "top": a.top, "repeats": a.repeats,
               "library": "baseline" if a.old_lib else "current", **res}
        print(json.dumps(res), flush=True)
        results.append(res)
        g.close()
        del g
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scales", default="22")
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--blocks", default="1,4,8,16,32")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--cap", type=int, default=400)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="a libpagerank_hip.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of each measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--old-lib", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
        a.blocks = [int(s) for s in a.blocks.split(",")]
    except ValueError:
        ap.error("--scales and --blocks take comma-separated lists of integers")
    if a.repeats < 1 or a.cap < 1 or a.queries < 1 or a.top < 1 or any(x < 1 for x in a.blocks):
        ap.error("--repeats, --cap, --queries, --top and the blocks must be at least 1")
    if not (a.tol >= 0.0 and a.tol != float("inf")):
        ap.error("--tol: not a finite number >= 0")
    if a.worker:
        return worker(a)
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--queries",
            str(a.queries), "--blocks", ",".join(map(str, a.blocks)), "--tol", repr(a.tol), "--cap", str(a.cap), "--top",
            str(a.top), "--repeats", str(a.repeats)]
    parts = [a.out + ".current.tmp", a.out + ".baseline.tmp"] if a.out else [None, None]
    runs = [(base + (["--out", parts[0]] if a.out else []), dict(os.environ))]
    if a.baseline_lib:
        runs.append((base + ["--old-lib"] + (["--out", parts[1]] if a.out else []),
                     dict(os.environ, PR_LIB_PATH=os.path.abspath(a.baseline_lib))))
    for cmd, env in runs:  # this parent never touches the GPU; one child at a time
        try:
            rc = subprocess.run(cmd, timeout=a.timeout, env=env).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"error": f"the measuring process exceeded {a.timeout} s"}), flush=True)
            return 1
        if rc != 0:
            return rc
    if a.out:  # one list: per scale the current build's record, then the baseline's
        lists = []
        for path in parts[:len(runs)]:
            with open(path) as f:
                lists.append(json.load(f))
            os.remove(path)
        merged = []
        for i, cur in enumerate(lists[0]):
            merged.append(cur)
            if len(lists) > 1:
                old = dict(lists[1][i])
                old["baseline_counts_equal"] = old.pop("counts") == cur["counts"]
                old["waves_baseline_over_queue"] = round(old["waves_ms"]["median"] / cur["queue_ms"]["median"], 4)
                merged.append(old)
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
