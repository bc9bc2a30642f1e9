"""The batch's two dangling modes on the bench's R-MAT graphs, one GPU, one process per build.

    python tools/batch_dangling_bench.py [--scales 20,22] [--widths 8,16] [--steps 20] [--repeats 3]
                                         [--baseline-lib PATH] [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device) with its canonical CSR kept, then for every width W a PageRankBatch with a
sparse seed vector in every column (three seeds that share the mass 0.15 V), and measures
  step      ms per iteration of step(--steps) followed by sync(), on the host clock, --repeats times
            after a warm-up, in uniform and in teleport mode; the HIP-event time of the same
            iterations (pr_batch_info's last_step_ns) next to it;
  refill    tools/batch_queue_bench.py's refill figure in both modes: run_queue over W queries with a
            cap of one iteration is one round that refills all W columns, runs one iteration and
            calls back W times; (round - one iteration of step_until_any) / W is one refill.  In
            teleport mode a refill also forms the column's ts (k_batch_tsum_col + its finalize).
With --baseline-lib PATH a second child process measures `step` in uniform mode on that build of
libpagerank_hip.so (the parent commit's).  Every figure is reported with all its repeats, their
median and their spread (max - min) / median.  One JSON line per (build, scale, width) on stdout and
the list of them in --out.  Each build runs in one child process under a time limit of its own; the
first failure ends the run with a non-zero status.
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

NEW_SYMBOLS = ("pr_batch_set_dangling", "pr_batch_get_dangling", "pr_batch_get_teleport_sums", "pr_batch_get_ranks_ex")


def seeds(V, j):
    ids = np.array([(7919 * j + 13) % V, (104729 * j + 1013) % V, (1299709 * j + 500009) % V], np.int32)
    ids = np.unique(ids).astype(np.int32)
    return ids, np.full(len(ids), 0.15 * V / len(ids))


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 5), "all": [round(x, 5) for x in v], "spread": round((max(v) - min(v)) / med, 4)}


def measure_step(b, steps, repeats):
    """(host-clock, HIP-event) ms per iteration of step(steps); sync(), `repeats` times after a warm-up."""
    b.reset()
    b.step(3)
    b.sync()
    host, dev = [], []
    for _ in range(repeats):
        b.reset()
        b.sync()
        t0 = time.perf_counter()
        b.step(steps)
        b.sync()
        host.append(1e3 * (time.perf_counter() - t0) / steps)
        dev.append(b.info()["last_step_ns"] * 1e-6 / steps)
    return host, dev


def measure_refill(b, V, W, repeats):
    """ms of one refill: (a run_queue round of W queries capped at one iteration - one iteration) / W."""
    queries = [seeds(V, W + j) + (0.0,) for j in range(W)]
    b.reset()
    b.run_queue(queries, 1, 1e-6)  # warm-up
    rounds, iters = [], []
    for _ in range(repeats):
        b.reset()
        b.sync()
        t0 = time.perf_counter()
        b.run_queue(queries, 1, 1e-6)
        rounds.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        b.step_until_any((1 << W) - 1, 1, 0.0)
        iters.append(1e3 * (time.perf_counter() - t0))
    return [(r - i) / W for r, i in zip(rounds, iters)], rounds, iters


def worker(a) -> int:
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
        for W in a.widths:
            res = {"build": "baseline" if a.old_lib else "current", "scale": scale, "vertices": V,
                   "edges": g.info()["n_edges"], "width": W, "steps": a.steps, "repeats": a.repeats}
            with sparky_hip.PageRankBatch(g, W) as b:
                for j in range(W):
                    b.set_teleport_sparse(j, *seeds(V, j))
                for mode in ("uniform",) if a.old_lib else ("uniform", "teleport", "uniform", "teleport"):
                    if not a.old_lib:
                        b.set_dangling(mode)
                    host, dev = measure_step(b, a.steps, a.repeats)
                    key = mode if mode + "_step_ms_per_iter" not in res else mode + "_again"
                    res[key + "_step_ms_per_iter"] = summary(host)
                    res[key + "_step_ms_per_iter_hip_events"] = summary(dev)
                if not a.old_lib:
                    dc, _ = b.norms()
                    res["teleport_dc_min"] = float(dc.min())  # > 0: the teleport term was at work
                    for mode in ("uniform", "teleport"):
                        b.set_dangling(mode)
                        refill, rounds, iters = measure_refill(b, V, W, a.repeats)
                        res[mode + "_refill_ms"] = summary(refill)
                        res[mode + "_refill_round_ms"] = summary(rounds)
                        res[mode + "_refill_iteration_ms"] = summary(iters)
                    res["batch_device_bytes"] = b.info()["device_bytes"]
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
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="a libpagerank_hip.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=600, help="time limit of each measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--old-lib", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
        a.widths = [int(s) for s in a.widths.split(",")]
    except ValueError:
        ap.error("--scales and --widths take comma-separated lists of integers")
    if a.steps < 1 or a.repeats < 1 or any(w < 1 or w > 16 for w in a.widths):
        ap.error("--steps and --repeats must be at least 1, widths in 1..16")
    if a.worker:
        return worker(a)
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--widths",
            ",".join(map(str, a.widths)), "--steps", str(a.steps), "--repeats", str(a.repeats)]
    parts = [a.out + ".current.tmp", a.out + ".baseline.tmp"] if a.out else [None, None]
    runs = [(base + (["--out", parts[0]] if a.out else []), dict(os.environ))]
    if a.baseline_lib:
        runs.append((base + ["--old-lib"] + (["--out", parts[1]] if a.out else []),
                     dict(os.environ, PR_LIB_PATH=os.path.abspath(a.baseline_lib))))
    for cmd, env in runs:  # this parent never touches the GPU; one child at a time
        try:
            rc = subprocess.run(cmd, env=env, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
            return 124
        if rc != 0:
            return rc
    if a.out:
        merged = []
        for p in parts[: len(runs)]:
            with open(p) as f:
                merged += json.load(f)
            os.remove(p)
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
