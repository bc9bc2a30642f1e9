"""Batched personalised PageRank against sequential single-vector runs on the bench's R-MAT
graphs, one GPU, one process per run.

    python tools/batch_bench.py [--scales 20,22,24] [--widths 1,2,4,8,16] [--steps 20] [--repeats 3]
                                [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device) with its canonical CSR kept, then for every width W
  baseline  W sequential single-vector personalised runs on the engine's own path
            (PageRankGraph.set_teleport; PR_STAT_SPMV_MS_MEAN: HIP events around the --steps
            iterations of a pr_step call), one vector after the other: the time of a pass is the sum
            over the W runs;
  batch     one PageRankBatch of width W (pr_batch_info's last_step_ns: HIP events around the
            --steps iterations of a pr_batch_step call),
each as --repeats measurements after a warm-up, reported with their median as ms per iteration and
ms per iteration per column, with the time of pr_batch_create (wall clock) and the batch's device
bytes.  Column 0 of the widest batch is compared with the single-vector run of the same vector as a
guard (relative bound 1e-9).  One JSON line per (scale, width) on stdout and the list of them in
--out.  The measurement runs in one child process under a time limit of its own; the first failure
ends the run with a non-zero status.
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


def vector(V, j):
    return 0.02 * (j + 1) + 1e-7 * ((np.arange(V) * (2 * j + 1)) % 1000)


def measure_single(g, V, W, steps, repeats):
    """ms per iteration of W sequential runs (their sum), `repeats` times; the ranks of vector 0."""
    sums = [0.0] * repeats
    ranks0 = None
    for j in range(W):
        g.set_teleport(vector(V, j))
        g.reset()
        g.step(3)  # warm-up
        g.sync()
        for k in range(repeats):
            g.reset()  # also clears the timing intervals
            g.step(steps)
            g.sync()
            sums[k] += g.stats()["spmv_ms_mean"]
        if j == 0:
            ranks0 = g.ranks().copy()
    g.set_teleport(None)
    return sums, ranks0


def measure_batch(sparky_hip, g, V, W, steps, repeats):
    t0 = time.perf_counter()
    b = sparky_hip.PageRankBatch(g, W)
    create_ms = 1e3 * (time.perf_counter() - t0)
    with b:
        for j in range(W):
            b.set_teleport(j, vector(V, j))
        b.reset()
        b.step(3)  # warm-up
        b.sync()
        out = []
        for _ in range(repeats):
            b.reset()
            b.step(steps)
            b.sync()
            out.append(b.info()["last_step_ns"] * 1e-6 / steps)
        inf = b.info()
        return out, create_ms, inf, b.ranks(0).copy()


def worker(a) -> int:
    import torch

    import sparky_hip
    from sparky_hip.workloads import generate

    results = []
    for scale in a.scales:
        t0 = time.perf_counter()
        wl = generate("rmat", scale=scale, edge_factor=16, device=0)
        V, E = wl.n_vertices, wl.n_edges
        g = sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True, n_edges=E)
        del wl
        torch.cuda.empty_cache()
        ginf = g.info()
        print(f"# scale {scale}: {V} vertices, {E} edges, layout {ginf['layout']}, {ginf['classes']} classes, built in "
              f"{time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        g.set_timing(True)
        med = lambda v: round(statistics.median(v), 5)  # noqa: E731
        for W in a.widths:
            single, r_single = measure_single(g, V, W, a.steps, a.repeats)
            batch, create_ms, binf, r_batch = measure_batch(sparky_hip, g, V, W, a.steps, a.repeats)
            err = float(np.max(np.abs(r_batch - r_single) / np.maximum(1.0, np.abs(r_single))))
            res = {"scale": scale, "vertices": V, "edges": ginf["n_edges"], "width": W, "stride": binf["stride"],
                   "steps": a.steps, "repeats": a.repeats,
                   "single_ms_per_iter": med(single), "batch_ms_per_iter": med(batch),
                   "single_ms_per_iter_per_column": round(med(single) / W, 5),
                   "batch_ms_per_iter_per_column": round(med(batch) / W, 5),
                   "batch_over_single": round(med(batch) / med(single), 4),
                   "single_ms_all": [round(x, 5) for x in single], "batch_ms_all": [round(x, 5) for x in batch],
                   "batch_create_ms": round(create_ms, 2), "batch_device_bytes": binf["device_bytes"],
                   "batch_units": binf["n_units"], "batch_long_rows": binf["n_long_rows"],
                   "graph_device_bytes": ginf["device_bytes"], "column0_max_rel_err": err}
            print(json.dumps(res), flush=True)
            results.append(res)
            if not err <= 1e-9:
                print(json.dumps({"scale": scale, "width": W, "error": "batch and single-vector ranks disagree"}),
                      flush=True)
                return 1
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
    ap.add_argument("--scales", default="20,22,24")
    ap.add_argument("--widths", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
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
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--widths",
           ",".join(map(str, a.widths)), "--steps", str(a.steps), "--repeats", str(a.repeats)]
    cmd += ["--out", a.out] if a.out else []
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
