"""Batch top-K (PageRankBatch.topk_all) against the per-column queries (PageRankBatch.topk) on the
bench's R-MAT graphs, one GPU, one process per run.

    python tools/batch_topk_bench.py [--scales 20,22,24] [--widths 8,16] [--ks 10,1000,100000] [--steps 20]
                                     [--repeats 3] [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device) with its canonical CSR kept, then for every width W a PageRankBatch whose
columns are seed sets (column j: 1 + 3 j seeds sharing the teleport mass 0.15 V) runs --steps
iterations, and for every K
  per_column  the W calls topk(j, K), one after the other (no exclusion set: the code path of the
              single-vector select over an extracted column), wall clock of all W;
  all         one topk_all(K), wall clock;
each as --repeats measurements, the two paths alternating and every measurement after a warm-up
call of its own, reported with their median and all values in ms.  Also reported: the passes of the
lockstep select over the matrix and over the compacted candidates, the pass at which it narrowed,
and the summed HIP-event time of its kernels (from one extra call of the internal entry point after
the timed ones; it records an event around every launch).  The lists of the two paths are compared
(IDs and rank bits) before anything is timed.  One JSON line per (scale, width, K) on stdout and the
list of them in --out.  The measurement runs in one child process under a time limit of its own;
the first failure ends the run with a non-zero status.
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


def timed(fn, repeats):
    fn()  # warm-up: allocations, code objects
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


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
        print(f"# scale {scale}: {V} vertices, {E} edges, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr,
              flush=True)
        rng = np.random.default_rng(scale)
        for W in a.widths:
            with sparky_hip.PageRankBatch(g, W) as b:
                for j in range(W):
                    seeds = rng.permutation(V)[: 1 + 3 * j].astype(np.int32)
                    b.set_teleport_sparse(j, seeds, np.full(len(seeds), 0.15 * V / len(seeds)))
                b.reset()
                b.step(a.steps)
                b.sync()
                for K in a.ks:
                    per = [b.topk(j, K) for j in range(W)]
                    lists, info = b._topk_all_ex(K, 8)
                    same = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64))
                               for x, y in zip(per, lists))
                    t_per, t_all = [], []  # the two paths alternate (both are warm from the calls above)
                    for _ in range(a.repeats):
                        t_per += timed(lambda: [b.topk(j, K) for j in range(W)], 1)
                        t_all += timed(lambda: b.topk_all(K), 1)
                    _, info = b._topk_all_ex(K, 8)  # warm by now: pass counts and the kernels' event time
                    med = statistics.median
                    res = {"scale": scale, "vertices": V, "width": W, "stride": b.info()["stride"], "k": K,
                           "steps": a.steps, "repeats": a.repeats,
                           "per_column_ms": round(med(t_per), 3), "all_ms": round(med(t_all), 3),
                           "per_column_over_all": round(med(t_per) / med(t_all), 3),
                           "per_column_ms_all": [round(x, 3) for x in t_per], "all_ms_all": [round(x, 3) for x in t_all],
                           "separated": min(t_per) > max(t_all),  # every per-column repeat above every topk_all repeat
                           "matrix_passes": info["matrix_passes"], "cand_passes": info["cand_passes"],
                           "narrowed_at": info["narrowed_at"], "all_kernel_ms": round(info["kernel_ns"] * 1e-6, 3),
                           "batch_device_bytes": b.info()["device_bytes"], "lists_equal": bool(same)}
                    print(json.dumps(res), flush=True)
                    results.append(res)
                    if not same:
                        print(json.dumps({"scale": scale, "width": W, "k": K, "error": "topk_all and topk disagree"}),
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
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--ks", default="10,1000,100000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
        a.widths = [int(s) for s in a.widths.split(",")]
        a.ks = [int(s) for s in a.ks.split(",")]
    except ValueError:
        ap.error("--scales, --widths and --ks take comma-separated lists of integers")
    if a.steps < 0 or a.repeats < 1 or any(w < 1 or w > 16 for w in a.widths) or any(k < 1 for k in a.ks):
        ap.error("--repeats must be at least 1, widths in 1..16, every K at least 1")
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--widths",
           ",".join(map(str, a.widths)), "--ks", ",".join(map(str, a.ks)), "--steps", str(a.steps), "--repeats",
           str(a.repeats)]
    cmd += ["--out", a.out] if a.out else []
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
