"""pr_batch_step_until on the GPU: per-column convergence decided on the device, through
PageRankBatch.step_until and both CLIs' --tol.

Reference: numpy over export_csr(), per column (tests/test_gpu_batch.py's Reference, re-stated) --
c = r / out_deg where out_deg > 0, S[v] = sum of c over the row's columns (S[v] = r_old[v] for an
empty row), dc = sum of r over the PR_VF_SINK vertices, r' = t + 0.85 (S + dc / N); a column stops
after the first iteration whose L1 delta sum_v |r'[v] - r[v]| is <= tol.  Bound on the ranks:
|got - want| <= 1e-9 max(1, |want|).  The iteration counts must match the reference exactly; so that
this is a fair demand the reference's own L1 is asserted to stay more than 1e-6 (relative) away from
tol on both sides of every crossing.  Where two runs must agree exactly they are compared as uint64
views: a column that step_until stopped after n iterations against a fresh batch after step(n).

Graphs, the smallest that reach each path: the 6-vertex KAT; V = 300 / E = 2500 (PACK units with
short and medium rows); V = 6000 / E = 60000 with 30 % of the links at vertex 0, whose ~5700 distinct
in-links exceed the unit capacity at every stride (CHUNK units and k_batch_long)."""
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
WIDTHS = [1, 3, 8, 16]
TOL = 1e-6
CAP = 400


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

    def __init__(self, csr):
        self.V = len(csr.out_deg)
        self.deg = csr.out_deg.astype(np.float64)
        self.col = csr.col_idx.astype(np.int64)
        self.row = np.repeat(np.arange(self.V), np.diff(csr.row_ptr))
        self.empty = np.diff(csr.row_ptr) == 0
        self.sink = (csr.vflags & PR_VF_SINK) != 0
        self._until = {}

    def dc(self, r):
        return float(np.sum(r[self.sink]))

    def step(self, r, t, damping=0.85):
        c = np.zeros(self.V)
        nz = self.deg > 0
        c[nz] = r[nz] / self.deg[nz]
        S = np.bincount(self.row, weights=c[self.col], minlength=self.V)
        S[self.empty] = r[self.empty]
        return t + damping * (S + self.dc(r) / self.V)

    def until(self, key, t):
        """(n, ranks after n iterations): the first n whose L1 delta is <= TOL.  Computed once per
        teleport vector (`key`) and shared, read-only, by every test of the graph.  Asserts that the
        crossing is not borderline: the L1 of iteration n and that of iteration n - 1 are more than
        1e-6 (relative) away from TOL, so an implementation within the rank bound counts the same."""
        if key not in self._until:
            r, before = np.ones(self.V), np.inf
            for n in range(1, CAP + 1):
                new = self.step(r, t)
                l1 = float(np.abs(new - r).sum())
                r = new
                if l1 <= TOL:
                    break
                before = l1
            assert l1 <= TOL, f"vector {key}: the reference needs more than {CAP} iterations"
            assert (TOL - l1) / TOL > 1e-6 and (before - TOL) / TOL > 1e-6, (key, n, l1, before)
            r.setflags(write=False)
            self._until[key] = (n, r)
        return self._until[key]


def assert_close(got, want):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"max error {err.max():.3e}")
    assert err.max() <= 1e-9, f"max error {err.max():.3e} at index {int(err.argmax())}"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def vectors(V, width):
    """Teleport vectors that stagger convergence: columns j % 3 == 0 put the mass 0.15 * 10^(j // 3)
    on the single seed (7 j + 1) % V, the others are test_gpu_batch.py's dense vectors; the last
    column of a batch wider than 1 stays scalar (None)."""
    ts = []
    for j in range(width):
        if j % 3 == 0:
            t = np.zeros(V)
            t[(7 * j + 1) % V] = 0.15 * 10.0 ** (j // 3)
        else:
            t = 0.02 * (j + 1) + 1e-4 * ((np.arange(V) * (2 * j + 1)) % V)
        ts.append(t)
    if width > 1:
        ts[-1] = None
    return ts


def term(t, V):
    return np.full(V, 0.15) if t is None else t


def new_batch(hip, g, ts):
    b = hip.PageRankBatch(g, len(ts))
    for j, t in enumerate(ts):
        if t is not None:
            b.set_teleport(j, t)
    b.reset()
    return b


def fixed_steps(hip, g, ts, counts):
    """A fresh batch stepped once through the sorted distinct `counts`: per column j the rank bits
    and the (dc, l1) bits after counts[j] iterations."""
    width = len(ts)
    rk, dc, l1 = [None] * width, np.zeros(width), np.zeros(width)
    with new_batch(hip, g, ts) as b:
        done = 0
        for n in sorted(set(int(c) for c in counts)):
            b.step(n - done)
            done = n
            d, l = b.norms()
            for j in range(width):
                if counts[j] == n:
                    rk[j], dc[j], l1[j] = bits(b.ranks(j)).copy(), d[j], l[j]
    return rk, dc, l1


class Case:
    """One graph, its reference, and per width the expected counts and the fixed-step bits (run once)."""

    def __init__(self, hip, g):
        self.hip, self.g, self.ref = hip, g, Reference(g.export_csr())
        self.V = self.ref.V
        self._fixed = {}

    def want(self, width):
        """(ts, counts, reference ranks) of the benign batch of `width`."""
        ts = vectors(self.V, width)
        res = [self.ref.until("scalar" if t is None else j, term(t, self.V)) for j, t in enumerate(ts)]
        counts = np.array([n for n, _ in res], np.int32)
        if width >= 3:
            assert len(set(counts.tolist())) >= 2, counts  # the columns really stop at different times
        return ts, counts, [r for _, r in res]

    def fixed(self, width):
        if width not in self._fixed:
            ts, counts, _ = self.want(width)
            self._fixed[width] = fixed_steps(self.hip, self.g, ts, counts)
        return self._fixed[width]

    def check_bits(self, b, width, iters):
        """Batch b, stopped by step_until, against step(counts[j]) per column: counts, ranks, norms."""
        _, counts, _ = self.want(width)
        rk, dc, l1 = self.fixed(width)
        assert np.array_equal(iters, counts), (iters, counts)
        for j in range(width):
            assert np.array_equal(bits(b.ranks(j)), rk[j]), j
        d, l = b.norms()
        assert np.array_equal(bits(d), bits(dc)) and np.array_equal(bits(l), bits(l1))
        assert (l <= TOL).all()
        assert b.info()["iters"] == counts.max()


@pytest.fixture(scope="module", params=["kat", "pack", "hub"])
def case(hip, request):
    if request.param == "kat":
        from sparky_hip.driver import read_edge_list

        urls, src, dst = read_edge_list(KAT)
        V = len(urls)
    elif request.param == "pack":
        V = 300
        src, dst = random_edges(np.random.default_rng(7), V, 2500)
    else:
        V = 6000
        src, dst = random_edges(np.random.default_rng(11), V, 60000, hub_frac=0.3)
    with hip.PageRankGraph(V, src, dst) as g:
        c = Case(hip, g)
        if request.param == "hub":
            csr = g.export_csr()
            assert csr.row_ptr[1] - csr.row_ptr[0] > 4096  # above the capacity at stride 1
            with hip.PageRankBatch(g, 1) as b:
                assert b.info()["n_long_rows"] >= 1  # CHUNK units and k_batch_long run at every stride
        yield c


# ---- 1: equals fixed steps ---------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_equals_fixed_steps(hip, case, width):
    ts, counts, want = case.want(width)
    print("reference iterations:", counts.tolist())
    with new_batch(hip, case.g, ts) as b:
        bytes0 = b.info()["device_bytes"]
        iters = b.step_until(CAP, TOL)
        print("iterations:", iters.tolist())
        assert iters.dtype == np.int32 and iters.shape == (width,)
        case.check_bits(b, width, iters)
        for j in range(width):
            assert_close(b.ranks(j), want[j])
        assert b.info()["device_bytes"] == bytes0  # the few words per column are there from create on


# ---- 2: the cap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_cap(hip, case, width):
    ts, counts, _ = case.want(width)
    assert counts.min() > 10  # no column converges within the caps used here
    rk5, dc5, l15 = fixed_steps(hip, case.g, ts, [5] * width)
    rk10, dc10, l110 = fixed_steps(hip, case.g, ts, [10] * width)
    with new_batch(hip, case.g, ts) as b:
        start = [bits(b.ranks(j)).copy() for j in range(width)]
        n0 = [bits(x).copy() for x in b.norms()]
        iters = b.step_until(0, TOL)  # a no-op
        assert (iters == 0).all() and b.info()["iters"] == 0
        assert all(np.array_equal(bits(b.ranks(j)), start[j]) for j in range(width))
        assert all(np.array_equal(bits(x), y) for x, y in zip(b.norms(), n0))
        iters = b.step_until(5, TOL)
        assert (iters == 5).all() and b.info()["iters"] == 5
        assert all(np.array_equal(bits(b.ranks(j)), rk5[j]) for j in range(width))
        d, l = b.norms()
        assert np.array_equal(bits(d), bits(dc5)) and np.array_equal(bits(l), bits(l15))
        assert (l > TOL).all()  # how a caller sees "not converged"
    with new_batch(hip, case.g, ts) as b:
        iters = b.step_until(10, 0.0)  # tol 0 needs an exact 0: nothing freezes
        assert (iters == 10).all()
        assert all(np.array_equal(bits(b.ranks(j)), rk10[j]) for j in range(width))
        d, l = b.norms()
        assert np.array_equal(bits(d), bits(dc10)) and np.array_equal(bits(l), bits(l110))


# ---- 3: the block size does not show -------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_block_independence(hip, case, width):
    ts, counts, _ = case.want(width)
    for block in (1, 3, 64):
        with new_batch(hip, case.g, ts) as b:
            iters, (enqueued, executed) = b._step_until_ex(CAP, TOL, block)
            case.check_bits(b, width, iters)
            assert executed == counts.max()
            assert executed <= enqueued <= min(CAP, -(-executed // block) * block)


# ---- 4: continuation -----------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_continuation(hip, case, width):
    ts, counts, _ = case.want(width)
    rk, dc, l1 = fixed_steps(hip, case.g, ts, counts + 3)
    with new_batch(hip, case.g, ts) as b:
        iters = b.step_until(CAP, TOL)
        assert np.array_equal(iters, counts)
        b.step(3)  # every column advances, the frozen ones included
        for j in range(width):
            assert np.array_equal(bits(b.ranks(j)), rk[j]), j
        assert b.info()["iters"] == counts.max() + 3
        d, l = b.norms()  # every column's last iteration is its own (counts[j] + 3)-th again
        assert np.array_equal(bits(d), bits(dc)) and np.array_equal(bits(l), bits(l1))
        again = b.step_until(CAP, TOL)  # a new call starts with every column active
        assert (again >= 1).all(), again
        assert b.info()["iters"] == counts.max() + 3 + again.max()


# ---- 5: isolation --------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 8, 16])
def test_isolation(hip, case, width):
    ts, counts, _ = case.want(width)
    wild = 1
    ts = list(ts)
    ts[wild] = np.full(case.V, 1.7e308)  # leaves the finite range: its L1 becomes NaN
    rk, dc, l1 = case.fixed(width)
    with new_batch(hip, case.g, ts) as b:
        iters = b.step_until(CAP, TOL)
        assert iters[wild] == CAP
        d, l = b.norms()
        assert np.isnan(l[wild]) and not np.isfinite(b.ranks(wild)).all()
        for j in range(width):
            if j == wild:
                continue
            assert iters[j] == counts[j]
            assert np.array_equal(bits(b.ranks(j)), rk[j]), j
            assert bits(d)[j] == bits(dc)[j] and bits(l)[j] == bits(l1)[j]
        assert b.info()["iters"] == CAP


# ---- 6: errors -----------------------------------------------------------------------------------
def test_errors(hip, case):
    import ctypes

    from sparky_hip import _lib

    def raises(code, fn, *args):
        with pytest.raises(hip.PageRankError) as ei:
            fn(*args)
        assert ei.value.code == code, ei.value

    g = case.g
    bytes0 = g.info()["device_bytes"]
    ts, counts, _ = case.want(3)
    with hip.PageRankBatch(g, 3) as b:
        raises(_lib.PR_ERR_STATE, b.step_until, 10, TOL)  # before reset
        for bad in (np.nan, -1.0, np.inf, -np.inf):
            raises(_lib.PR_ERR_INVALID, b.step_until, 10, bad)  # argument errors win over the state error
        raises(_lib.PR_ERR_INVALID, b.step_until, -1, TOL)
        for j, t in enumerate(ts):
            if t is not None:
                b.set_teleport(j, t)
        b.reset()
        for bad in (np.nan, -1.0, np.inf):
            raises(_lib.PR_ERR_INVALID, b.step_until, 10, bad)
        raises(_lib.PR_ERR_INVALID, b.step_until, -1, TOL)
        raises(_lib.PR_ERR_INVALID, b._step_until_ex, 10, TOL, 0)
        assert b.info()["iters"] == 0  # the failed calls ran nothing
        L = _lib.load()
        assert L.pr_batch_step_until(b._h, CAP, ctypes.c_double(TOL), None) == _lib.PR_OK  # iters_out = NULL
        case.check_bits(b, 3, counts)
        assert g.info()["device_bytes"] == bytes0  # the graph's own figure never moves
    assert g.info()["device_bytes"] == bytes0


# ---- 7: both CLIs --------------------------------------------------------------------------------
def _base(runner):
    return [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]


def run_cli(runner, args):
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    res = subprocess.run(_base(runner) + args, capture_output=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_cli_tol(tmp_path):
    inp, a, b = tmp_path / "edges.txt", tmp_path / "a.txt", tmp_path / "b.txt"
    inp.write_text("\n".join(KAT) + "\n")
    a.write_text("C 2\nA\n")
    b.write_text("# one seed\nF\n")
    inp, a, b, d = str(inp), str(a), str(b), str(tmp_path)
    out = {}
    for runner in ("cpp", "python"):
        out[runner] = run_cli(runner, [inp, str(CAP), "--seed-set", a, "--seed-set", b, "--top", "3", "--tol", "1e-3",
                                       "--out", os.path.join(d, "out_" + runner)])
    assert out["cpp"] == out["python"]  # identical bytes
    lines = out["cpp"].decode().splitlines()
    heads = [i for i, ln in enumerate(lines) if ln.startswith("# seed set ")]
    assert len(heads) == 2 and lines[heads[0]] == f"# seed set 0: {a}" and lines[heads[1]] == f"# seed set 1: {b}"
    n = []
    for h in heads:
        words = lines[h + 1].split()
        assert words[:2] == ["#", "iterations:"] and words[3:] == ["(converged)"], lines[h + 1]
        n.append(int(words[2]))
    assert all(1 <= x < CAP for x in n)
    assert lines[:heads[0]] == [f"Starting iter{i}" for i in range(max(n))]
    assert len(lines) == max(n) + 2 * 5
    fixed = {}
    for j, h in enumerate(heads):  # each set's listing: that of the same command run for exactly n_j iterations
        if n[j] not in fixed:
            fixed[n[j]] = run_cli("cpp", [inp, str(n[j]), "--seed-set", a, "--seed-set", b, "--top", "3"]).decode().splitlines()
        plain = fixed[n[j]]
        at = plain.index(lines[h])
        assert lines[h + 2:h + 5] == plain[at + 1:at + 4]
    for runner in ("cpp", "python"):
        for j in range(2):
            root = os.path.join(d, "out_" + runner, f"seedset{j}")
            assert os.listdir(root) == [f"PageRank{n[j] - 1}"]
            assert os.path.exists(os.path.join(root, f"PageRank{n[j] - 1}", "_SUCCESS"))
    for j in range(2):
        parts = [open(os.path.join(d, "out_" + r, f"seedset{j}", f"PageRank{n[j] - 1}", "part-00000"), "rb").read()
                 for r in ("cpp", "python")]
        assert parts[0] == parts[1] and parts[0].startswith(b"(A,")
