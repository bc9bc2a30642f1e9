"""Personalised PageRank on the GPU: pr_set_teleport / pr_set_teleport_sparse through
PageRankGraph.set_teleport, set_teleport_sparse, PartGroup and both CLIs' --seeds.

Reference: numpy over export_csr() -- c = r / out_deg where out_deg > 0, S[v] = sum of c over the
row's columns (S[v] = r_old[v] for an empty row), dc = sum of r over the PR_VF_SINK vertices,
r' = t + 0.85 (S + dc / N).  Bound: |got - want| <= 1e-9 max(1, |want|), the project's parity
figure made relative because a single seed's term is 0.15 V.  Where two runs must agree exactly
(a vector of all 0.15 against the scalar, sparse against dense) they are compared as uint64 views.

The three places the teleport term enters are all covered: the unit epilogue of the fused layout
(every "fused" case), k_finalize's long rows (test_long_rows, fused) and the grouped epilogue of
the split layout in its class-loop, walk, one-wave, 128-class and fused-pack forms."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "build", "pagerank")
KAT = ["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"]  # tests/test_cli_gpu.py
PR_VF_SINK = 2

# fused; 8 and 64 classes with the class loop / the per-row walk in four-wave / one-wave
# workgroups; 128 classes (class loop, four waves only)
LAYOUTS = [("fused", None)] + [("split", dict(classes=c, epi_walk=w, epi_narrow=n))
                               for c in (8, 64) for w in (0, 1) for n in (0, 1)] + [("split", dict(classes=128))]
LAYOUT_IDS = ["fused"] + [f"c{c}-walk{w}-narrow{n}" for c in (8, 64) for w in (0, 1) for n in (0, 1)] + ["c128"]


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def random_edges(rng, V, E, hub_frac=0.0):
    src = rng.integers(0, V, E, dtype=np.int64)
    dst = rng.integers(0, V, E, dtype=np.int64)
    if hub_frac > 0:
        dst[rng.random(E) < hub_frac] = 0
    dst[rng.random(E) < 0.05] = -1
    seen = np.zeros(V, bool)  # every ID appears: one record per missing vertex
    seen[src] = True
    seen[dst[dst >= 0]] = True
    miss = np.nonzero(~seen)[0]
    src = np.concatenate([src, miss])
    dst = np.concatenate([dst, np.full(miss.shape, -1)])
    return src.astype(np.int32), dst.astype(np.int32)


def graph_kw(layout, opts):
    return dict(layout="fused") if layout == "fused" else dict(layout="split", options=opts)


class Reference:
    """The iteration in numpy over a canonical CSR (rows = dst, columns = src)."""

    def __init__(self, csr):
        self.V = len(csr.out_deg)
        self.deg = csr.out_deg.astype(np.float64)
        self.col = csr.col_idx.astype(np.int64)
        self.row = np.repeat(np.arange(self.V), np.diff(csr.row_ptr))
        self.empty = np.diff(csr.row_ptr) == 0
        self.sink = (csr.vflags & PR_VF_SINK) != 0

    def step(self, r, t, damping=0.85):
        c = np.zeros(self.V)
        nz = self.deg > 0
        c[nz] = r[nz] / self.deg[nz]
        S = np.bincount(self.row, weights=c[self.col], minlength=self.V)
        S[self.empty] = r[self.empty]
        dc = float(np.sum(r[self.sink]))
        return t + damping * (S + dc / self.V)

    def run(self, t, iterations, r=None):
        r = np.ones(self.V) if r is None else r
        for _ in range(iterations):
            r = self.step(r, t)
        return r


def assert_close(got, want):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-9, f"max error {err.max():.3e} at vertex {int(err.argmax())}"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.fixture(scope="module")
def small():
    """V = 3000, E = 20000 (hole rows in every split layout), its distinct teleport vector."""
    V = 3000
    src, dst = random_edges(np.random.default_rng(5), V, 20000)
    return V, src, dst, 0.05 + 1e-4 * np.arange(V)


@pytest.mark.parametrize("layout,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_vector_is_the_scalar_bitwise(hip, small, layout, opts):
    V, src, dst, _ = small
    with hip.PageRankGraph(V, src, dst, **graph_kw(layout, opts)) as g:
        g.reset()
        g.step(10)
        scalar = g.ranks().copy()
        g.set_teleport(np.full(V, 0.15))
        g.reset()
        g.step(10)
        assert np.array_equal(bits(g.ranks()), bits(scalar))
        g.set_teleport(None)
        g.reset()
        g.step(10)
        assert np.array_equal(bits(g.ranks()), bits(scalar))


@pytest.mark.parametrize("layout,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_every_row_reads_its_own_value(hip, small, layout, opts):
    """t[v] = 0.05 + 1e-4 v: a wrong ID -> row map or a leaked hole row is off by far more than
    the bound."""
    V, src, dst, t = small
    with hip.PageRankGraph(V, src, dst, **graph_kw(layout, opts)) as g:
        inf = g.info()
        if layout == "split":
            assert inf["layout"] == 1 and inf["classes"] == opts["classes"]
        ref = Reference(g.export_csr())
        g.set_teleport(t)
        g.reset()
        g.step(1)
        want = ref.run(t, 1)
        assert_close(g.ranks(), want)
        g.step(6)
        assert_close(g.ranks(), ref.run(t, 6, want))
        assert g.stats()["iters"] == 7


@pytest.mark.parametrize("layout", ["fused", "split"])
def test_long_rows(hip, layout):
    """Vertex 0 has 2049 in-links, vertex 1 has 5000: rows cut into pieces, finished by k_finalize
    (fused layout) or as long segments (split layout)."""
    V = 6000
    rng = np.random.default_rng(21)
    src, dst = random_edges(rng, V, 20000)
    s0 = rng.permutation(V)[:2049]
    s1 = rng.permutation(V)[:5000]
    src = np.concatenate([src, s0, s1]).astype(np.int32)
    dst = np.concatenate([dst, np.zeros(2049), np.ones(5000)]).astype(np.int32)
    t = 0.05 + 1e-4 * np.arange(V)
    with hip.PageRankGraph(V, src, dst, **graph_kw(layout, dict(classes=8))) as g:
        inf = g.info()
        assert inf["n_long_rows"] >= 2
        assert inf["layout"] == (1 if layout == "split" else 0)
        ref = Reference(g.export_csr())
        g.set_teleport(t)
        g.reset()
        g.step(5)
        assert_close(g.ranks(), ref.run(t, 5))


@pytest.mark.parametrize("layout", ["fused", "split"])
def test_sparse_equals_dense_bitwise(hip, small, layout):
    V, src, dst, _ = small
    rng = np.random.default_rng(33)
    seeds = rng.permutation(V)[:17].astype(np.int32)
    cases = [(seeds, rng.random(17) * 40.0 + 0.01, rest) for rest in (0.0, 0.01)]
    cases.append((np.zeros(0, np.int32), np.zeros(0), 0.3))  # n = 0: every vertex `rest`
    cases.append((rng.permutation(V).astype(np.int32), rng.random(V) + 0.01, 7.0))  # n = V: no vertex `rest`
    with hip.PageRankGraph(V, src, dst, **graph_kw(layout, dict(classes=8))) as g:
        for ids, values, rest in cases:
            dense = np.full(V, rest)
            dense[ids] = values
            g.set_teleport_sparse(ids, values, rest)
            g.reset()
            g.step(5)
            sparse_ranks = g.ranks().copy()
            g.set_teleport(dense)
            g.reset()
            g.step(5)
            assert np.array_equal(bits(g.ranks()), bits(sparse_ranks))
        ref = Reference(g.export_csr())  # and the last vector against the reference
        assert_close(g.ranks(), ref.run(dense, 5))


@pytest.mark.parametrize("layout", ["fused", "split"])
def test_seed_moves_the_top(hip, layout):
    """64 hubs in a ring, every other vertex links to hub i % 64 (test_gpu_topk.py's tie graph): the
    uniform run cannot tell the hubs apart; one seed at hub 5 carrying the whole teleport mass puts
    the top of the list at or just downstream of it."""
    V = 4160
    hubs = np.arange(64)
    rest = np.arange(64, V)
    src = np.concatenate([hubs, rest]).astype(np.int32)
    dst = np.concatenate([(hubs + 1) % 64, rest % 64]).astype(np.int32)
    t = np.zeros(V)
    t[5] = 0.15 * V
    with hip.PageRankGraph(V, src, dst, **graph_kw(layout, dict(classes=8))) as g:
        g.set_teleport_sparse(np.array([5], np.int32), np.array([0.15 * V]), 0.0)
        g.reset()
        g.step(30)
        full = g.ranks().copy()
        assert_close(full, Reference(g.export_csr()).run(t, 30))
        ids, ranks = g.topk(1)
        assert int(ids[0]) in (5, 6, 7, 8)
        everyone = np.arange(V, dtype=np.int32)
        for k in (1, 64, 1000):
            o = np.lexsort((everyone, -full))[:k]
            ids, ranks = g.topk(k)
            assert np.array_equal(ids, everyone[o]) and np.array_equal(bits(ranks), bits(full[o]))


@pytest.mark.parametrize("pack_fused", [0, 1])
def test_parts(hip, small, pack_fused):
    """Three parts on one device: every part keeps its own rows of the same vector (the fused-pack
    epilogue and the pack kernel); clearing it on all parts is the group's scalar run, bitwise."""
    V, src, dst, t = small
    P = 3
    with hip.PageRankGraph(V, src, dst, layout="fused") as g1:
        ref = Reference(g1.export_csr())
    opts = {"classes": 8, "pack_fused": pack_fused}
    parts = [hip.PageRankGraph(V, src, dst, part=p, n_parts=P, keep_canonical=False, layout="split", options=opts)
             for p in range(P)]
    try:
        grp = hip.PartGroup(parts)
        scalar = grp.run(5).copy()
        grp.set_teleport(t)
        got = grp.run(5)
        assert not np.isnan(got).any()
        assert_close(got, ref.run(t, 5))
        grp.set_teleport(None)
        assert np.array_equal(bits(grp.run(5)), bits(scalar))
        ids = np.array([7, 2999, 64], np.int32)  # the sparse form on every part
        vals = np.array([3.0, 0.5, 11.0])
        grp.set_teleport_sparse(ids, vals, 0.02)
        dense = np.full(V, 0.02)
        dense[ids] = vals
        assert_close(grp.run(5), ref.run(dense, 5))
    finally:
        for g in parts:
            g.close()


def test_state_and_lifetime(hip, small):
    V, src, dst, t = small
    t2 = 0.3 - 5e-5 * np.arange(V)
    with hip.PageRankGraph(V, src, dst) as g:
        ref = Reference(g.export_csr())
        rows = g.info()["local_rows"]
        assert rows == V
        bytes0 = g.info()["device_bytes"]
        g.set_teleport(t)  # before the first reset
        bytes1 = g.info()["device_bytes"]
        assert bytes1 >= bytes0 + 8 * rows
        g.reset()
        g.step(1)
        assert_close(g.ranks(), ref.run(t, 1))  # the first iteration already used it
        g.step(1)
        g.set_teleport(t2)  # between two steps: holds from the next iteration on
        assert g.info()["device_bytes"] == bytes1  # a second set allocates nothing more
        g.step(3)
        assert_close(g.ranks(), ref.run(t2, 3, ref.run(t, 2)))
        g.set_teleport(None)  # NULL keeps the allocation, and the scalar is back
        assert g.info()["device_bytes"] == bytes1
        g.step(2)
        assert_close(g.ranks(), ref.run(0.15, 2, ref.run(t2, 3, ref.run(t, 2))))
        assert g.stats()["iters"] == 7


def test_argument_errors_change_nothing(hip, small):
    from sparky_hip import _lib

    V, src, dst, t = small
    with hip.PageRankGraph(V, src, dst) as g:
        bytes0 = g.info()["device_bytes"]
        bad = [(np.array([1, V], np.int32), np.array([1.0, 1.0]), 0.0),   # ID out of range
               (np.array([1, -1], np.int32), np.array([1.0, 1.0]), 0.0),
               (np.array([4, 9, 4], np.int32), np.array([1.0, 1.0, 1.0]), 0.0),  # duplicate
               (np.array([1, 2], np.int32), np.array([1.0, np.inf]), 0.0),
               (np.array([1, 2], np.int32), np.array([1.0, 1.0]), np.nan)]
        for ids, values, rest in bad:
            with pytest.raises(hip.PageRankError) as ei:
                g.set_teleport_sparse(ids, values, rest)
            assert ei.value.code == _lib.PR_ERR_INVALID
        with pytest.raises(hip.PageRankError) as ei:
            g.set_teleport(np.where(np.arange(V) == 17, np.nan, 0.15))
        assert ei.value.code == _lib.PR_ERR_INVALID
        with pytest.raises(ValueError):
            g.set_teleport(np.zeros(V + 1))
        assert g.info()["device_bytes"] == bytes0  # nothing was allocated
        g.reset()
        g.step(3)
        scalar = g.ranks().copy()
    with hip.PageRankGraph(V, src, dst) as g:
        g.reset()
        g.step(3)
        assert np.array_equal(bits(g.ranks()), bits(scalar))  # and the failed calls set nothing


# ---- both CLIs ---------------------------------------------------------------------------------
def _base(runner):
    return [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("seeds")
    inp, seeds = d / "edges.txt", d / "seeds.txt"
    inp.write_text("\n".join(KAT) + "\n")
    seeds.write_text("C 2\nA\n")
    return str(inp), str(seeds)


def run_cli(runner, cli_files, *extra):
    inp, seeds = cli_files
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    res = subprocess.run(_base(runner) + [inp, "10", "--seeds", seeds, "--top", "3", *extra], capture_output=True,
                         text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[:10] == [f"Starting iter{i}" for i in range(10)] and len(lines) == 13
    return lines[10:]


@pytest.fixture(scope="module")
def one_device_lines(cli_files):
    return {runner: run_cli(runner, cli_files) for runner in ("cpp", "python")}


def test_cli_seeds(hip, cli_files, one_device_lines):
    """Both CLIs print the same lines, and those are the Python host's set_teleport_sparse + topk."""
    from sparky_hip._host import HostEdges, java_double_native, seed_teleport

    assert one_device_lines["cpp"] == one_device_lines["python"]
    edges = HostEdges.read(cli_files[0])
    ids, weights = edges.read_seeds(cli_files[1])
    assert list(ids) == [2, 0] and list(weights) == [2.0, 1.0]
    names = edges.names()
    with hip.PageRankGraph(edges.n_vertices, edges.src, edges.dst, keep_canonical=False) as g:
        g.set_teleport_sparse(ids, seed_teleport(weights, edges.n_vertices))
        g.reset()
        g.step(10)
        top_ids, top_ranks = g.topk(3)
    edges.close()
    want = [f"{names[i]} has rank: {java_double_native(r)}." for i, r in zip(top_ids.tolist(), top_ranks.tolist())]
    assert one_device_lines["cpp"] == want


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_seeds_devices_group(cli_files, one_device_lines, runner):
    lines = run_cli(runner, cli_files, "--devices", "0,0")
    for got, want in zip(lines, one_device_lines[runner]):
        gu, gr = got.rsplit(" has rank: ", 1)
        wu, wr = want.rsplit(" has rank: ", 1)
        g, w = float(gr[:-1]), float(wr[:-1])
        assert gu == wu and abs(g - w) <= 1e-9 * max(1.0, abs(w))
