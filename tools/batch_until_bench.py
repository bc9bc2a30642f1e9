"""pr_batch_step_until against the alternatives a caller has without it, on the bench's R-MAT graphs,
one GPU, one process per run.

    python tools/batch_until_bench.py [--scales 20,22] [--widths 8,16] [--tol 1e-6] [--cap 1000]
                                      [--repeats 3] [--blocks 1,4,8,16,32] [--out FILE] [--timeout SECONDS]

Per scale: builds the graph bench.py times (sparky_hip.workloads.generate: seeded R-MAT, edge factor
16, interned on the device) with its canonical CSR kept, then for every width W a PageRankBatch with
teleport vectors that stagger convergence (columns j % 3 == 0: the mass 0.15 * 10^(j // 3) on one
seed; the others dense; the last one the scalar).  All times are a host clock around a call that
ends synchronised, --repeats measurements after a warm-up, alternating between the variants, with
their median, minimum and maximum:
  (a) nothing frozen: 20 iterations of step_until(20, 0.0) against 20 of step(20), ms per iteration
      (the until-kernels with every column active, plus their read-backs, against the plain ones);
      the plain figure is also given from pr_batch_info's HIP events;
  (b) end to end at --tol: step_until(cap, tol) against the host loop a caller needs without it
      (step(1) + norms() per iteration until every L1 is <= tol) and against step(max_j iters_j), the
      run of someone who knew the count; the slowest column's ranks are compared with the latter's
      bitwise;
  (c) the block size: (b)'s step_until through _step_until_ex with every value of --blocks.
One JSON line per (scale, width) on stdout and the list of them in --out.  The measurement runs in
one child process under a time limit of its own; the first failure ends the run with a non-zero
status.
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


def vectors(V, W):
    ts = []
    for j in range(W):
        if j % 3 == 0:
            t = np.zeros(V)
            t[(7 * j + 1) % V] = 0.15 * 10.0 ** (j // 3)
        else:
            t = 0.02 * (j + 1) + 1e-7 * ((np.arange(V) * (2 * j + 1)) % 1000)
        ts.append(t)
    if W > 1:
        ts[-1] = None
    return ts


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def host_loop(b, cap, tol):
    """What a caller does today: one iteration, one read-back, until every column is within tol."""
    for n in range(1, cap + 1):
        b.step(1)
        if (b.norms()[1] <= tol).all():
            return n
    return cap


def step_sync(b, n):
    b.step(n)
    b.sync()


def measure(b, a):
    res = {}
    b.reset()
    step_sync(b, 3)  # warm-up of both sets of kernels
    b.step_until(3, 0.0)
    # (a) nothing frozen
    plain, plain_ev, until = [], [], []
    for _ in range(a.repeats):
        b.reset()
        plain.append(timed(lambda: step_sync(b, 20))[0] / 20)
        plain_ev.append(b.info()["last_step_ns"] * 1e-6 / 20)
        b.reset()
        ms, iters = timed(lambda: b.step_until(20, 0.0))
        assert (iters == 20).all()
        until.append(ms / 20)
    res["a_step_ms_per_iter"] = spread(plain)
    res["a_step_event_ms_per_iter"] = spread(plain_ev)
    res["a_until_ms_per_iter"] = spread(until)
    res["a_until_over_step"] = round(statistics.median(until) / statistics.median(plain), 4)
    # (b) end to end
    t_until, t_loop, t_fixed = [], [], []
    for _ in range(a.repeats):
        b.reset()
        ms, iters = timed(lambda: b.step_until(a.cap, a.tol))
        t_until.append(ms)
        slow = int(iters.argmax())
        mine = b.ranks(slow).copy()
        b.reset()
        ms, n_loop = timed(lambda: host_loop(b, a.cap, a.tol))
        t_loop.append(ms)
        b.reset()
        t_fixed.append(timed(lambda: step_sync(b, int(iters.max())))[0])
        same = bool(np.array_equal(mine.view(np.uint64), b.ranks(slow).view(np.uint64)))
    res.update({"b_iters": [int(x) for x in iters], "b_converged": bool((b.norms()[1] <= a.tol).all()),
                "b_host_loop_iters": int(n_loop), "b_until_ms": spread(t_until), "b_host_loop_ms": spread(t_loop),
                "b_fixed_ms": spread(t_fixed), "b_slowest_column": slow, "b_slowest_bitwise_equal_fixed": same,
                "b_host_loop_over_until": round(statistics.median(t_loop) / statistics.median(t_until), 4),
                "b_until_over_fixed": round(statistics.median(t_until) / statistics.median(t_fixed), 4)})
    # (c) the block size
    per_block = {blk: [] for blk in a.blocks}
    enq = {}
    for _ in range(a.repeats):
        for blk in a.blocks:
            b.reset()
            ms, (it2, info) = timed(lambda: b._step_until_ex(a.cap, a.tol, blk))
            assert np.array_equal(it2, iters)
            per_block[blk].append(ms)
            enq[blk] = info[0]
    res["c_block_ms"] = {str(blk): spread(v) for blk, v in per_block.items()}
    res["c_block_enqueued"] = {str(blk): int(n) for blk, n in enq.items()}
    return res, same


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
        for W in a.widths:
            with sparky_hip.PageRankBatch(g, W) as b:
                for j, t in enumerate(vectors(V, W)):
                    if t is not None:
                        b.set_teleport(j, t)
                res, same = measure(b, a)
                inf = b.info()
            res = {"scale": scale, "vertices": V, "edges": g.info()["n_edges"], "width": W, "stride": inf["stride"],
                   "tol": a.tol, "cap": a.cap, "repeats": a.repeats, **res}
            print(json.dumps(res), flush=True)
            results.append(res)
            if not same:
                print(json.dumps({"scale": scale, "width": W, "error": "step_until and step(max iters) disagree"}),
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
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--blocks", default="1,4,8,16,32")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--cap", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
        a.widths = [int(s) for s in a.widths.split(",")]
        a.blocks = [int(s) for s in a.blocks.split(",")]
    except ValueError:
        ap.error("--scales, --widths and --blocks take comma-separated lists of integers")
    if a.repeats < 1 or a.cap < 1 or any(w < 1 or w > 16 for w in a.widths) or any(x < 1 for x in a.blocks):
        ap.error("--repeats, --cap and the blocks must be at least 1, widths in 1..16")
    if not (a.tol >= 0.0 and a.tol != float("inf")):
        ap.error("--tol: not a finite number >= 0")
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--widths",
           ",".join(map(str, a.widths)), "--blocks", ",".join(map(str, a.blocks)), "--tol", repr(a.tol), "--cap",
           str(a.cap), "--repeats", str(a.repeats)]
    cmd += ["--out", a.out] if a.out else []
    try:  # this parent never touches the GPU
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
