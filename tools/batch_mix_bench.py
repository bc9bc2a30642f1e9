"""Batch mixes (PageRankBatch.mix_topk) against the host route on the bench's R-MAT graphs, one GPU,
one process per run.

    python tools/batch_mix_bench.py [--scales 20,22,24] [--width 16] [--mixes 1,16] [--ks 10,1000,100000]
                                    [--steps 20] [--repeats 3] [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device) with its canonical CSR kept; a PageRankBatch of --width seed-set columns
(column j: 1 + 3 j seeds sharing the teleport mass 0.15 V) runs --steps iterations.  For every
number of mixes M (random weights, every column taking part) and every K, in the same process:
  host  what a caller could do before mix_topk: ranks(j) for the participating columns (8 V bytes
        each over the bus, every column once per call), then per mix the numpy blend in the model's
        order, np.argpartition and a sort of the K best; wall clock of all M;
  mix   one mix_topk(weights, K); wall clock;
each as --repeats measurements, the two routes alternating, after one warm-up call each, reported
with their median and all values in ms.  Also reported, from one extra call of the internal entry
point: the mix kernel's HIP-event time and its rate under the byte model 8 V (S_IN + S_OUT), the
select's passes over the blends and over the compacted candidates and its kernels' summed event
time.  The two routes' lists are compared before anything is timed: IDs and score bits of mix_topk
against the model's listing of the model's blend (tests/batch_mix_model.py).  One JSON line per
(scale, M, K) on stdout and the list of them in --out.  The measurement runs in one child process
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "pagerank-using-apache-spark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_route(b, weights, K):
    """Fetch every column that takes part in a mix, once; per mix blend them, select and order the K best."""
    import batch_mix_model as bmm

    out = []
    cols = [b.ranks(j) if (weights[:, j] != 0.0).any() else None for j in range(b.width)]
    for w in weights:
        m = bmm.blend([x for x in w if x != 0.0], [c for x, c in zip(w, cols) if x != 0.0])
        k = min(K, len(m))
        part = np.argpartition(-m, k - 1)[:k] if k < len(m) else np.arange(len(m))
        order = part[np.lexsort((part, -m[part]))]
        out.append((order.astype(np.int32), m[order]))
    return out


def worker(a) -> int:
    import torch

    import batch_mix_model as bmm
    import sparky_hip
    from sparky_hip.workloads import generate

    results = []
    med = statistics.median
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
        W = a.width
        with sparky_hip.PageRankBatch(g, W) as b:
            for j in range(W):
                seeds = rng.permutation(V)[: 1 + 3 * j].astype(np.int32)
                b.set_teleport_sparse(j, seeds, np.full(len(seeds), 0.15 * V / len(seeds)))
            b.reset()
            b.step(a.steps)
            b.sync()
            s_in = b.info()["stride"]
            for M in a.mixes:
                weights = rng.standard_normal((M, W))
                for K in a.ks:
                    # correctness first, on mix 0 and the last mix: the model's listing of the model's blend
                    lists = b.mix_topk(weights, K)
                    same = True
                    for i in sorted({0, M - 1}):
                        m = bmm.blend(weights[i], [b.ranks(j) for j in range(W)])
                        same = same and bmm.same(lists[i], bmm.listing(m, K))
                    host_route(b, weights[:1], K)  # warm-up of the host route
                    t_host, t_mix = [], []
                    for _ in range(a.repeats):  # the two routes alternate
                        t1 = time.perf_counter()
                        host_route(b, weights, K)
                        t_host.append(1e3 * (time.perf_counter() - t1))
                        t1 = time.perf_counter()
                        b.mix_topk(weights, K)
                        t_mix.append(1e3 * (time.perf_counter() - t1))
                    _, info = b._mix_topk_ex(weights, K)  # warm by now: event times and pass counts
                    s_out = 1
                    while s_out < M:
                        s_out *= 2
                    model_bytes = 8 * V * (s_in + s_out)
                    res = {"scale": scale, "vertices": V, "width": W, "mixes": M, "k": K, "steps": a.steps,
                           "repeats": a.repeats, "host_ms": round(med(t_host), 3), "mix_ms": round(med(t_mix), 3),
                           "host_over_mix": round(med(t_host) / med(t_mix), 3),
                           "host_ms_all": [round(x, 3) for x in t_host], "mix_ms_all": [round(x, 3) for x in t_mix],
                           "separated": min(t_host) > max(t_mix),  # every host repeat above every mix_topk repeat
                           "s_in": s_in, "s_out": s_out, "mix_kernel_ms": round(info["mix_ns"] * 1e-6, 4),
                           "mix_model_bytes": model_bytes,
                           "mix_tb_per_s": round(model_bytes / max(info["mix_ns"], 1) * 1e-3, 3),
                           "matrix_passes": info["matrix_passes"], "cand_passes": info["cand_passes"],
                           "select_kernel_ms": round(info["select_ns"] * 1e-6, 3),
                           "batch_device_bytes": b.info()["device_bytes"], "lists_equal": bool(same)}
                    print(json.dumps(res), flush=True)
                    results.append(res)
                    if not same:
                        print(json.dumps({"scale": scale, "mixes": M, "k": K, "error": "mix_topk and the model disagree"}),
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
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--mixes", default="1,16")
    ap.add_argument("--ks", default="10,1000,100000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
        a.mixes = [int(s) for s in a.mixes.split(",")]
        a.ks = [int(s) for s in a.ks.split(",")]
    except ValueError:
        ap.error("--scales, --mixes and --ks take comma-separated lists of integers")
    if a.steps < 0 or a.repeats < 1 or not 1 <= a.width <= 16 or any(m < 1 or m > 16 for m in a.mixes) or any(k < 1 for k in a.ks):
        ap.error("--repeats must be at least 1, the width and every number of mixes in 1..16, every K at least 1")
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--width",
           str(a.width), "--mixes", ",".join(map(str, a.mixes)), "--ks", ",".join(map(str, a.ks)), "--steps", str(a.steps),
           "--repeats", str(a.repeats)]
    cmd += ["--out", a.out] if a.out else []
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
