"""Batched personalised PageRank on the GPU: pr_batch_* through PageRankBatch and both CLIs'
--seed-set.

Reference: numpy over export_csr(), per column (tests/test_gpu_teleport.py's Reference, re-stated) --
c = r / out_deg where out_deg > 0, S[v] = sum of c over the row's columns (S[v] = r_old[v] for an
empty row), dc = sum of r over the PR_VF_SINK vertices (0 for a PR_DANGLING_NONE graph),
r' = t + 0.85 (S + dc / N).  Bound: |got - want| <= 1e-9 max(1, |want|), the project's parity
figure in the relative form of that file.  Where two runs must agree exactly they are compared as
uint64 views."""
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
WIDTHS = [1, 2, 3, 5, 8, 16]


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


class Reference:
    """The iteration in numpy over a canonical CSR (rows = dst, columns = src)."""

    def __init__(self, csr, dangling_none=False):
        self.V = len(csr.out_deg)
        self.deg = csr.out_deg.astype(np.float64)
        self.col = csr.col_idx.astype(np.int64)
        self.row = np.repeat(np.arange(self.V), np.diff(csr.row_ptr))
        self.empty = np.diff(csr.row_ptr) == 0
        self.sink = ((csr.vflags & PR_VF_SINK) != 0) & (not dangling_none)

    def dc(self, r):
        return float(np.sum(r[self.sink]))

    def step(self, r, t, damping=0.85):
        c = np.zeros(self.V)
        nz = self.deg > 0
        c[nz] = r[nz] / self.deg[nz]
        S = np.bincount(self.row, weights=c[self.col], minlength=self.V)
        S[self.empty] = r[self.empty]
        return t + damping * (S + self.dc(r) / self.V)

    def run(self, t, iterations, r=None):
        r = np.ones(self.V) if r is None else r
        for _ in range(iterations):
            r = self.step(r, t)
        return r


def assert_close(got, want):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"max error {err.max():.3e}")
    assert err.max() <= 1e-9, f"max error {err.max():.3e} at index {int(err.argmax())}"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def vectors(V, width):
    """A distinct teleport vector per column; the last column of a batch wider than 1 stays scalar
    (None)."""
    ts = [0.02 * (j + 1) + 1e-4 * ((np.arange(V) * (2 * j + 1)) % V) for j in range(width)]
    if width > 1:
        ts[-1] = None
    return ts


def set_all(b, ts):
    for j, t in enumerate(ts):
        if t is not None:
            b.set_teleport(j, t)


def term(t, V):
    return np.full(V, 0.15) if t is None else t


def check_columns(b, ref, ts, first=1, more=6):
    """1 iteration, then 6 more: every column against the reference, and the norms of the last one."""
    V = ref.V
    b.reset()
    b.step(first)
    want = [ref.run(term(t, V), first) for t in ts]
    for j in range(len(ts)):
        assert_close(b.ranks(j), want[j])
    b.step(more - 1)
    prev = [ref.run(term(t, V), more - 1, w) for t, w in zip(ts, want)]
    b.step(1)
    last = [ref.step(p, term(t, V)) for t, p in zip(ts, prev)]
    for j in range(len(ts)):
        assert_close(b.ranks(j), last[j])
    dc, l1 = b.norms()
    assert dc.shape == l1.shape == (len(ts),)
    assert_close(dc, [ref.dc(p) for p in prev])
    assert_close(l1, [np.abs(x - p).sum() for x, p in zip(last, prev)])
    assert b.info()["iters"] == first + more
    return last


# ---- against the reference ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def kat(hip):
    from sparky_hip.driver import read_edge_list

    urls, src, dst = read_edge_list(KAT)
    with hip.PageRankGraph(len(urls), src, dst) as g:
        yield g, Reference(g.export_csr())


@pytest.mark.parametrize("width", WIDTHS)
def test_kat(hip, kat, width):
    g, ref = kat
    with hip.PageRankBatch(g, width) as b:
        inf = b.info()
        assert inf["width"] == width and inf["stride"] == 1 << (width - 1).bit_length()
        ts = vectors(ref.V, width)
        set_all(b, ts)
        check_columns(b, ref, ts)
        if width == 1:  # the one column left scalar: the plain run
            b.set_teleport(0, None)
            check_columns(b, ref, [None])


@pytest.fixture(scope="module")
def small(hip):
    """V = 3000, E = 20000, 5 % no-link records."""
    V = 3000
    src, dst = random_edges(np.random.default_rng(5), V, 20000)
    with hip.PageRankGraph(V, src, dst) as g:
        yield g, Reference(g.export_csr())


@pytest.mark.parametrize("width", WIDTHS)
def test_random_graph(hip, small, width):
    g, ref = small
    ts = vectors(ref.V, width)
    with hip.PageRankBatch(g, width) as b:
        set_all(b, ts)
        got = check_columns(b, ref, ts)
        mine = b.ranks(0).copy()
    g.set_teleport(ts[0])  # column 0 against the existing engine: other sum orders, so the bound
    try:
        g.reset()
        g.step(7)
        assert_close(mine, g.ranks())
        assert_close(got[0], g.ranks())
    finally:
        g.set_teleport(None)


@pytest.fixture(scope="module", params=["local", "none"])
def hub(hip, request):
    """V = 40000, E = 400000, 30 % of the links point at vertex 0: a row of ~38000 distinct in-links,
    cut into chunks at every stride (the capacity is at most 4096)."""
    V = 40_000
    src, dst = random_edges(np.random.default_rng(11), V, 400_000, hub_frac=0.3)
    with hip.PageRankGraph(V, src, dst, dangling=request.param) as g:
        csr = g.export_csr()
        assert csr.row_ptr[1] - csr.row_ptr[0] > 30_000
        yield g, Reference(csr, dangling_none=request.param == "none")


@pytest.mark.parametrize("width", [1, 8, 16])
def test_hub_graph(hip, hub, width):
    g, ref = hub
    ts = vectors(ref.V, width)
    with hip.PageRankBatch(g, width) as b:
        assert b.info()["n_long_rows"] >= 1  # the chunk-order path runs
        set_all(b, ts)
        check_columns(b, ref, ts)
        dc, _ = b.norms()
        if not ref.sink.any():
            assert (dc == 0.0).all()  # PR_DANGLING_NONE


# ---- bitwise properties ------------------------------------------------------------------------
def run_bits(hip, g, width, ts, steps):
    with hip.PageRankBatch(g, width) as b:
        set_all(b, ts)
        b.reset()
        for n in steps:
            b.step(n)
        return [bits(b.ranks(j)).copy() for j in range(width)]


@pytest.mark.parametrize("width", [3, 16])
def test_reproducible_and_step_split(hip, small, width):
    g, ref = small
    ts = vectors(ref.V, width)
    a = run_bits(hip, g, width, ts, [7])
    for other in (run_bits(hip, g, width, ts, [7]), run_bits(hip, g, width, ts, [3, 4])):
        for x, y in zip(a, other):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("width", [2, 5, 16])
def test_column_position_does_not_matter(hip, small, hub, width):
    for g, ref in (small, hub):
        ts = vectors(ref.V, width)
        ts[-1] = ts[0]
        out = run_bits(hip, g, width, ts, [5])
        assert np.array_equal(out[0], out[-1])


@pytest.mark.parametrize("big", [1e300, 1.7e308])
def test_neighbour_blow_up_stays_in_its_column(hip, small, big):
    g, ref = small
    width = 4
    ts = [t if t is not None else np.full(ref.V, 0.3) for t in vectors(ref.V, width)]
    benign = run_bits(hip, g, width, ts, [40])
    ts[1] = np.full(ref.V, big)
    wild = run_bits(hip, g, width, ts, [40])
    if big > 1e308:
        assert not np.isfinite(wild[1].view(np.float64)).all()  # the neighbour really left the finite range
    for j in (0, 2, 3):
        assert np.array_equal(benign[j], wild[j])


def test_sparse_equals_dense(hip, small):
    g, ref = small
    V = ref.V
    rng = np.random.default_rng(33)
    seeds = rng.permutation(V)[:17].astype(np.int32)
    cases = [(seeds, rng.random(17) * 40.0 + 0.01, 0.0), (seeds, rng.random(17) + 0.01, 0.01),
             (np.zeros(0, np.int32), np.zeros(0), 0.3)]
    with hip.PageRankBatch(g, 3) as b:
        for j, (ids, values, rest) in enumerate(cases):
            b.set_teleport_sparse(j, ids, values, rest)
        b.reset()
        b.step(5)
        sparse = [bits(b.ranks(j)).copy() for j in range(3)]
        dense = []
        for j, (ids, values, rest) in enumerate(cases):
            t = np.full(V, rest)
            t[ids] = values
            dense.append(t)
            b.set_teleport(j, t)
        b.reset()
        b.step(5)
        for j in range(3):
            assert np.array_equal(bits(b.ranks(j)), sparse[j])
        assert_close(b.ranks(0), ref.run(dense[0], 5))


# ---- top-K ---------------------------------------------------------------------------------------
def test_topk(hip):
    """64 hubs in a ring, every other vertex links to hub i % 64 (test_gpu_topk.py's tie graph): under
    the all-zero teleport vector and under the scalar the 4096 non-hub vertices share one rank."""
    V = 4160
    hubs, rest = np.arange(64), np.arange(64, V)
    src = np.concatenate([hubs, rest]).astype(np.int32)
    dst = np.concatenate([(hubs + 1) % 64, rest % 64]).astype(np.int32)
    everyone = np.arange(V, dtype=np.int32)
    with hip.PageRankGraph(V, src, dst) as g, hip.PageRankBatch(g, 3) as b:
        b.set_teleport(0, vectors(V, 1)[0])
        b.set_teleport_sparse(1, np.zeros(0, np.int32), np.zeros(0), 0.0)  # all-zero teleport: large tie classes
        b.reset()
        b.step(6)
        for j in range(3):
            full = b.ranks(j).copy()
            if j == 1:
                assert len(np.unique(full)) <= 65
            order = np.lexsort((everyone, -full))
            for k in (1, 10, V, V + 5):
                ids, ranks = b.topk(j, k)
                o = order[:k]
                assert np.array_equal(ids, everyone[o]) and np.array_equal(bits(ranks), bits(full[o]))
        ids, ranks = b.topk(0, 0)
        assert len(ids) == 0


# ---- errors and lifetime -------------------------------------------------------------------------
def test_errors(hip, small):
    from sparky_hip import _lib

    g, ref = small
    V = ref.V

    def raises(code, fn, *args, **kw):
        with pytest.raises(hip.PageRankError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, ei.value

    for width in (0, 17):
        raises(_lib.PR_ERR_INVALID, hip.PageRankBatch, g, width)
    src, dst = random_edges(np.random.default_rng(6), 200, 900)
    with hip.PageRankGraph(200, src, dst, keep_canonical=False) as g2:
        raises(_lib.PR_ERR_STATE, hip.PageRankBatch, g2, 2)
    parts = [hip.PageRankGraph(200, src, dst, part=p, n_parts=2) for p in range(2)]
    try:
        hip.PartGroup(parts).reset()
        raises(_lib.PR_ERR_STATE, hip.PageRankBatch, parts[0], 2)
    finally:
        for p in parts:
            p.close()

    bytes0 = g.info()["device_bytes"]
    t = vectors(V, 1)[0]
    with hip.PageRankBatch(g, 3) as b:
        raises(_lib.PR_ERR_STATE, b.step, 1)  # before reset
        raises(_lib.PR_ERR_STATE, b.ranks, 0)
        b.set_teleport(0, t)
        one = np.array([1.0, 1.0])
        raises(_lib.PR_ERR_INVALID, b.set_teleport, 3, t)  # bad column
        raises(_lib.PR_ERR_INVALID, b.set_teleport, -1, t)
        raises(_lib.PR_ERR_INVALID, b.set_teleport_sparse, 3, np.array([1, 2], np.int32), one)
        raises(_lib.PR_ERR_INVALID, b.set_teleport_sparse, 0, np.array([4, 4], np.int32), one)  # duplicate
        raises(_lib.PR_ERR_INVALID, b.set_teleport_sparse, 0, np.array([1, V], np.int32), one)  # out of range
        raises(_lib.PR_ERR_INVALID, b.set_teleport_sparse, 0, np.array([1, 2], np.int32), np.array([1.0, np.nan]))
        raises(_lib.PR_ERR_INVALID, b.set_teleport_sparse, 0, np.array([1, 2], np.int32), one, np.inf)
        raises(_lib.PR_ERR_INVALID, b.set_teleport, 0, np.where(np.arange(V) == 17, np.nan, 0.15))
        raises(_lib.PR_ERR_INVALID, b.ranks, 3)
        raises(_lib.PR_ERR_INVALID, b.topk, 0, -1)
        with pytest.raises(ValueError):
            b.set_teleport(0, np.zeros(V + 1))
        b.reset()
        b.step(5)
        got = bits(b.ranks(0)).copy()
        assert b.info()["device_bytes"] >= 4 * 8 * 4 * V  # R, T and two C at stride 4
        assert g.info()["device_bytes"] == bytes0  # the graph's own figure never moves
    assert g.info()["device_bytes"] == bytes0
    assert np.array_equal(got, run_bits(hip, g, 3, [t, None, None], [5])[0])  # the failed calls set nothing


# ---- both CLIs -------------------------------------------------------------------------------------
def _base(runner):
    return [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("seedsets")
    inp, a, b = d / "edges.txt", d / "a.txt", d / "b.txt"
    inp.write_text("\n".join(KAT) + "\n")
    a.write_text("C 2\nA\n")
    b.write_text("# one seed\nF\n")
    return str(inp), str(a), str(b), str(d)


def run_cli(runner, args):
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    res = subprocess.run(_base(runner) + args, capture_output=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_cli_seed_sets(cli_files):
    inp, a, b, d = cli_files
    out = {}
    for runner in ("cpp", "python"):
        out[runner] = run_cli(runner, [inp, "10", "--seed-set", a, "--seed-set", b, "--top", "3", "--out",
                                       os.path.join(d, "out_" + runner)])
    assert out["cpp"] == out["python"]  # identical bytes
    lines = out["cpp"].decode().splitlines()
    assert lines[:10] == [f"Starting iter{i}" for i in range(10)] and len(lines) == 10 + 2 * 4
    assert lines[10] == f"# seed set 0: {a}" and lines[14] == f"# seed set 1: {b}"
    for j, path in enumerate((a, b)):  # each set's lines: those of a single --seeds run of its file
        single = run_cli("cpp", [inp, "10", "--seeds", path, "--top", "3"]).decode().splitlines()[10:]
        mine = lines[11 + 4 * j:14 + 4 * j]
        assert len(single) == 3
        for got, want in zip(mine, single):
            gu, gr = got.rsplit(" has rank: ", 1)
            wu, wr = want.rsplit(" has rank: ", 1)
            x, w = float(gr[:-1]), float(wr[:-1])
            assert gu == wu and abs(x - w) <= 1e-9 * max(1.0, abs(w))
            assert gr == wr or x != w  # equal ranks print as equal text
    for runner in ("cpp", "python"):
        for j in range(2):
            part = os.path.join(d, "out_" + runner, f"seedset{j}", "PageRank9")
            assert os.path.exists(os.path.join(part, "_SUCCESS"))
            rows = open(os.path.join(part, "part-00000")).read().splitlines()
            assert len(rows) == 6 and rows[0].startswith("(A,")
    for j in range(2):
        parts = [open(os.path.join(d, "out_" + r, f"seedset{j}", "PageRank9", "part-00000"), "rb").read()
                 for r in ("cpp", "python")]
        assert parts[0] == parts[1]
