"""bench.py --dump-outputs / --full.

A plain run sets up, warms up, times its steps and prints the line; with --dump-outputs it also
writes what the last timed step computed (float64 .npy, at most 64 MB in all, a fixed seeded sample
of the ranks above bench.DUMP_MAX_RANKS vertices); the validation leg (parity, cpu_baseline) runs
only with --full.  The sampling is checked on CPU with a fake graph, the plain run itself on the
GPU at a size small enough for a second: its dumped ranks must equal, bit for bit, warmup + steps
iterations of the library on the same seeded graph."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeGraph:
    def __init__(self, V):
        self.V = V

    def ranks(self, out):
        out[: self.V] = 1.0 + np.arange(self.V) * 1e-6
        return out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_ranks_of_a_small_graph(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    V = 1000
    shapes = bench.dump_outputs(str(tmp_path / "o"), FakeGraph(V), None, 0, V, {"last_dc": 0.25, "last_l1": 3.5})
    got = _load(tmp_path / "o")
    assert sorted(got) == ["ranks", "ranks_index", "stats"] and shapes["ranks"] == [V]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["ranks_index"], np.arange(V))
    assert np.array_equal(got["ranks"], 1.0 + np.arange(V) * 1e-6)
    assert np.array_equal(got["stats"], [0.25, 3.5])


def test_dump_samples_a_large_graph_the_same_way_every_time(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    V = bench.DUMP_MAX_RANKS + 12345
    st = {"last_dc": 0.0, "last_l1": 0.0}
    bench.dump_outputs(str(tmp_path / "a"), FakeGraph(V), None, 0, V, st)
    bench.dump_outputs(str(tmp_path / "b"), FakeGraph(V), None, 0, V, st)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    idx = a["ranks_index"].astype(np.int64)
    assert idx.shape == (bench.DUMP_MAX_RANKS,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < V
    assert np.array_equal(a["ranks"], 1.0 + idx * 1e-6)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
    # a non-zero rank of an N > 1 run takes part in the reduction only: it writes nothing
    assert bench.dump_outputs(str(tmp_path / "c"), FakeGraph(V), None, 1, V, st) is None
    assert not os.path.exists(tmp_path / "c")


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    steps, warmup, scale = 3, 2, 12
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--scale", str(scale), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["iterations_timed"] == steps
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "GTEPS" and line["dtype"] == "f64"
    assert abs(line["value"] - line["config"]["n_edges_dedup"] / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * line["value"]
    # a plain run: no validation leg
    assert line["full"] is False and line["parity"] is None and line["cpu_baseline"] is None
    assert "oracle" not in p.stderr
    got = _load(out)
    assert sorted(got) == ["ranks", "ranks_index", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert line["outputs"] == {n: list(a.shape) for n, a in got.items()}

    import sparky_hip
    from sparky_hip.workloads import generate

    wl = generate("rmat", scale=scale)
    V = wl.n_vertices
    assert line["config"]["n_vertices"] == V and got["ranks"].shape == (V,)
    with sparky_hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device_input=True, n_edges=wl.n_edges,
                                  keep_canonical=False) as g:
        g.reset()
        g.step(warmup + steps)
        g.sync()
        ref = g.ranks().copy()
        st = g.stats()
    assert np.array_equal(got["ranks_index"], np.arange(V))
    assert np.array_equal(got["ranks"], ref)
    assert np.array_equal(got["stats"], [st["last_dc"], st["last_l1"]])
