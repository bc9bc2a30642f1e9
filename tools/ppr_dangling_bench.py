"""What the engine's teleport dangling mode costs a pass, and the scalar bench line on another build.

    python tools/ppr_dangling_bench.py [--scales 20,24,26] [--layouts fused,split] [--steps 20] [--repeats 3]
                                       [--lib PATH] [--out FILE] [--timeout SECONDS]
    python tools/ppr_dangling_bench.py --bench [--lib PATH] [--steps 20] [--warmup 3] [--out FILE]

First form.  Per (scale, layout): builds the graph bench.py times (sparky_hip.workloads.generate:
seeded R-MAT, edge factor 16, interned on the device) in the given layout, sets a dense teleport
vector of all 0.15, turns the library's timing on and measures PR_STAT_SPMV_MS_MEAN (one part: the
whole iteration, one event interval over the --steps iterations of a pr_step call) for
  U    the vector with the uniform dangling term (the kTeleOn kernels),
  D    pr_set_teleport_dangling(TELEPORT) (the kTeleDangling kernels: one more multiply per row),
  U'   the uniform mode again,
  D'   the mode again,
each as --repeats measurements after a warm-up, reported with their median.  |U - U'| is the spread
within the process against which D - U is to be read.  With t = 0.15 everywhere ts = 0.15 V, so
q * t = dc / V up to rounding: the top 64 IDs of the legs must agree and their ranks lie within 1e-9,
which guards against timing a mode that did nothing or something else.  With --lib PATH the library
at PATH is measured instead (PR_LIB_PATH); a build without the mode's symbols runs U and U' only:
two such processes around one of this build give the parent-versus-parent spread of the same cells.

Second form (--bench): runs `bench.py --gpus 1 --steps K --warmup W` in a child process, with --lib
on that library (the symbols it lacks are marked optional first, which bench.py itself cannot do),
and prints bench.py's JSON line: alternate the two builds, process by process.

Every measurement runs in one child process under a time limit of its own; this parent never touches
the GPU; the first failure ends the run with a non-zero status.
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

NEW_SYMBOLS = {"pr_set_teleport_dangling", "pr_get_teleport_dangling", "pr_get_teleport_sum"}


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
    return out, (ids.tolist(), ranks.tolist())


def worker(a) -> int:
    import sparky_hip._lib as L

    if a.lib:
        L.OPTIONAL |= NEW_SYMBOLS
    import torch

    import sparky_hip
    from sparky_hip.workloads import generate

    has_mode = hasattr(L.load(), "pr_set_teleport_dangling")
    results = []
    for scale in a.scales:
        for layout in a.layouts:
            t0 = time.perf_counter()
            wl = generate("rmat", scale=scale, edge_factor=16, device=0)
            V, E = wl.n_vertices, wl.n_edges
            g = sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True, n_edges=E,
                                         keep_canonical=False, layout=layout)
            del wl
            torch.cuda.empty_cache()
            inf = g.info()
            print(f"# scale {scale} {layout}: {V} vertices, {E} edges, layout {inf['layout']}, {inf['classes']} classes, "
                  f"{inf['n_sink']} sinks, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            g.set_timing(True)
            g.set_teleport(np.full(V, 0.15))
            legs, tops = {}, {}
            for leg in ("U", "D", "U2", "D2") if has_mode else ("U", "U2"):
                if has_mode:
                    g.set_teleport_dangling("teleport" if leg[0] == "D" else "uniform")
                legs[leg], tops[leg] = measure(g, a.steps, a.repeats)
            med = {k: round(statistics.median(v), 5) for k, v in legs.items()}
            res = {"scale": scale, "layout": layout, "vertices": V, "edges": E, "classes": inf["classes"],
                   "steps": a.steps, "repeats": a.repeats, "lib": a.lib or "this build", "has_mode": has_mode,
                   "uniform_ms": med["U"], "uniform_again_ms": med["U2"],
                   "uu_spread_pct": round(100.0 * abs(med["U2"] - med["U"]) / med["U"], 3),
                   "all": {k: [round(x, 5) for x in v] for k, v in legs.items()}}
            ok = tops["U"] == tops["U2"]
            if has_mode:
                u = 0.5 * (med["U"] + med["U2"])
                d = 0.5 * (med["D"] + med["D2"])
                res.update({"dangling_ms": med["D"], "dangling_again_ms": med["D2"],
                            "dd_spread_pct": round(100.0 * abs(med["D2"] - med["D"]) / med["D"], 3),
                            "dangling_over_uniform_pct": round(100.0 * (d - u) / u, 3), "ts": g.teleport_sum()})
                ru, rd = np.array(tops["U"][1]), np.array(tops["D"][1])
                ok = ok and tops["D"] == tops["D2"] and tops["D"][0] == tops["U"][0]
                ok = ok and bool(np.max(np.abs(rd - ru) / ru) <= 1e-9) and (inf["n_sink"] == 0 or tops["D"][1] != tops["U"][1])
            res["guard_ok"] = bool(ok)
            print(json.dumps(res), flush=True)
            results.append(res)
            g.close()
            del g
            torch.cuda.empty_cache()
            if not ok:
                print(json.dumps({"scale": scale, "layout": layout, "error": "the legs' top-64 lists disagree"}), flush=True)
                return 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


def bench_worker(a) -> int:
    """bench.py in this process, on --lib if given, with the symbols that build lacks marked optional."""
    import runpy

    import sparky_hip._lib as L

    if a.lib:
        L.OPTIONAL |= NEW_SYMBOLS
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    except SystemExit as e:
        return int(e.code or 0)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scales", default="20,24,26")
    ap.add_argument("--layouts", default="fused,split")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="--bench: bench.py's --warmup")
    ap.add_argument("--bench", action="store_true", help="run bench.py (the scalar path) instead")
    ap.add_argument("--lib", default=None, help="measure this build of libpagerank_hip.so instead (PR_LIB_PATH)")
    ap.add_argument("--out", default=None, help="also write the results to this file")
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        a.scales = [int(s) for s in a.scales.split(",")]
    except ValueError:
        ap.error("--scales takes a comma-separated list of R-MAT scales")
    a.layouts = a.layouts.split(",")
    if any(x not in ("auto", "fused", "split") for x in a.layouts):
        ap.error("--layouts takes a comma-separated list of auto, fused, split")
    if a.steps < 1 or a.repeats < 1:
        ap.error("--steps and --repeats must be at least 1")
    if a.worker:
        return bench_worker(a) if a.bench else worker(a)
    env = dict(os.environ)
    if a.lib:
        env["PR_LIB_PATH"] = os.path.abspath(a.lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scales", ",".join(map(str, a.scales)), "--layouts",
           ",".join(a.layouts), "--steps", str(a.steps), "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
    cmd += (["--lib", a.lib] if a.lib else []) + (["--bench"] if a.bench else [])
    try:  # this parent never touches the GPU
        if not a.bench:
            return subprocess.run(cmd + (["--out", a.out] if a.out else []), env=env, timeout=a.timeout).returncode
        res = subprocess.run(cmd, env=env, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        if a.out and res.returncode == 0:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(res.stdout.strip().splitlines()[-1] + "\n")
        return res.returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
