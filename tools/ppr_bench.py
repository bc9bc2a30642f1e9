"""What the per-row teleport vector costs a pass: scalar / vector / scalar (ABA) on the bench's
R-MAT graphs, one GPU, one process per run.

    python tools/ppr_bench.py [--scales 20,22,26] [--steps 20] [--repeats 3] [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device), turns the library's timing on and measures PR_STAT_SPMV_MS_MEAN (one
part: the whole iteration, one event interval over the --steps iterations of a pr_step call) for
  A   the scalar teleport (the kernels of a handle without a vector),
  B   pr_set_teleport with a dense vector (the TELE kernels: 8 more bytes read per row and pass),
  A'  the scalar again after pr_set_teleport(NULL),
each as --repeats measurements after a warm-up, reported with their median.  The vector is all 0.15,
so leg B must reproduce leg A's ranks bit for bit: the top 64 (ID, rank) pairs of the three legs are
compared as a guard.  |A - A'| is the run-to-run spread against which B - A is to be read.  One JSON
line per scale on stdout and the list of them in --out.  The measurement runs in one child process
under a time limit of its own; the first failure ends the run with a non-zero status.
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


def measure(g, steps, repeats):
    g.reset()
    g.step(3)  # warm-up
    g.sync()
    out = []
    for _ in range(repeats):
        g.reset()  # also clears the timing intervals
        g.step(steps)
        g.sync()
        out.append(g.stats()["spmv_ms_mean"])
    ids, ranks = g.topk(64)
    return out, (ids.tolist(), ranks.view(np.uint64).tolist())


def worker(a) -> int:
    import torch

    import sparky_hip
    from sparky_hip.workloads import generate

    results = []
    for scale in a.scales:
        t0 = time.perf_counter()
        wl = generate("rmat", scale=scale, edge_factor=16, device=0)
        V, E = wl.n_vertices, wl.n_edges
        g = sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True, n_edges=E,
                                     keep_canonical=False)
        del wl
        torch.cuda.empty_cache()
        inf = g.info()
        print(f"# scale {scale}: {V} vertices, {E} edges, layout {inf['layout']}, {inf['classes']} classes, built in "
              f"{time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        g.set_timing(True)
        bytes0 = inf["device_bytes"]
        a1, top_a1 = measure(g, a.steps, a.repeats)
        g.set_teleport(np.full(V, 0.15))
        b, top_b = measure(g, a.steps, a.repeats)
        g.set_teleport(None)
        a2, top_a2 = measure(g, a.steps, a.repeats)
        med = lambda v: round(statistics.median(v), 5)  # noqa: E731
        res = {"scale": scale, "vertices": V, "edges": E, "layout": inf["layout"], "classes": inf["classes"],
               "steps": a.steps, "repeats": a.repeats,
               "scalar_ms": med(a1), "vector_ms": med(b), "scalar_again_ms": med(a2),
               "scalar_ms_all": [round(x, 5) for x in a1], "vector_ms_all": [round(x, 5) for x in b],
               "scalar_again_ms_all": [round(x, 5) for x in a2],
               "aa_spread_pct": round(100.0 * abs(med(a2) - med(a1)) / med(a1), 3),
               "vector_over_scalar_pct": round(100.0 * (med(b) - 0.5 * (med(a1) + med(a2))) / (0.5 * (med(a1) + med(a2))), 3),
               "vector_bytes": g.info()["device_bytes"] - bytes0, "same_bits": top_a1 == top_b == top_a2}
        print(json.dumps(res), flush=True)
        results.append(res)
        g.close()
        del g
        torch.cuda.empty_cache()
        if not res["same_bits"]:
            print(json.dumps({"scale": scale, "error": "the all-0.15 vector and the scalar disagree"}), flush=True)
            return 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scales", default="20,22,26")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
    except ValueError:
        ap.error("--scales takes a comma-separated list of R-MAT scales")
    if a.steps < 1 or a.repeats < 1:
        ap.error("--steps and --repeats must be at least 1")
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--steps",
           str(a.steps), "--repeats", str(a.repeats)] + (["--out", a.out] if a.out else [])
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
