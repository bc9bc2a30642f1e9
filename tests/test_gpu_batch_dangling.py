"""PR_BATCH_DANGLING_TELEPORT on the GPU (csrc/pr_batch.hip: k_batch_units_td, k_batch_long_td,
k_batch_tsum_col, k_batch_tsum_finalize), bitwise.

Reference: tests/batch_dangling_model.py -- the order-exact row sums of tests/batch_order_model.py,
then q = dc / ts and t + damping * (S + q * t), one separately rounded float64 operation at a time,
with the fallback to the uniform dc / N for a column whose ts is 0 or not finite.  Ranks are compared
as uint64 views: no tolerance.  The model takes the device's own previous ranks, the dc that norms()
reports as used and the ts that teleport_sums() reports; ts itself is a sum whose order spans the
grid, so it is held to

  ts   |ts - fsum(t)| <= V 2^-52 fsum(|t|): twice the first-order worst case (V - 1) 2^-53 sum|t| of
       any order of V additions -- the argument of the dc bound in tests/test_gpu_batch_boundaries.py

Graphs: batch_order_model's boundary_graph() and many_units_graph(), a ten-vertex graph with two
components for the locality statement, and a V = 300 / E = 2500 graph like
tests/test_gpu_batch_queue.py's, with 100 sink-only vertices, for the queue.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_dangling_model as bdm
import batch_order_model as bom
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
PR_ERR_STATE = -5  # include/pagerank_hip.h
CLI = os.path.join(PKG_DIR, "build", "pagerank")


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Case:
    """A graph on the device, its exported CSR, random initial ranks and one model per stride."""

    def __init__(self, hip, made, seed, dangling="local"):
        self.V, self.src, self.dst, self.plan = made
        self.dangling_none = dangling == "none"
        self.g = hip.PageRankGraph(self.V, self.src, self.dst, dangling=dangling)
        self.csr = self.g.export_csr()
        assert np.array_equal(np.diff(self.csr.row_ptr), self.plan["indeg"])
        rng = np.random.default_rng(seed)
        self.init = rng.uniform(0.5, 1.5, self.V)
        self.init.setflags(write=False)
        self.seed = seed
        self._models = {}

    def model(self, stride):
        if stride not in self._models:
            self._models[stride] = bdm.DanglingModel(self.csr, stride, self.dangling_none)
        return self._models[stride]

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def boundary(hip):
    c = Case(hip, bom.boundary_graph(), 31)
    yield c
    c.close()


@pytest.fixture(scope="module")
def many(hip):
    c = Case(hip, bom.many_units_graph(), 32)
    yield c
    c.close()


def set_columns(b, specs):
    for j, s in enumerate(specs):
        if s[0] == "dense":
            b.set_teleport(j, s[1])
        elif s[0] == "sparse":
            b.set_teleport_sparse(j, s[1], s[2], 0.0)


def open_batch(hip, case, width, mode="teleport"):
    """A batch with teleport_columns()'s vectors set; returns (batch, model, specs, terms)."""
    b = hip.PageRankBatch(case.g, width)
    specs, terms = bom.teleport_columns(case.V, width, case.seed + 100)
    set_columns(b, specs)
    if mode is not None:
        b.set_dangling(mode)
    assert b.info()["stride"] == bom.stride_of(width)
    return b, case.model(bom.stride_of(width)), specs, terms


def check_sums(b, specs, terms, cols=None):
    """teleport_sums() against math.fsum (in the columns `cols`; default: all), and exactly 0.0 for the
    scalar columns.  Returns ts."""
    ts = b.teleport_sums()
    assert ts.shape == (len(specs),)
    for j, s in enumerate(specs):
        if s[0] == "scalar":
            assert bits(ts[j])[0] == 0, (j, ts[j])
            continue
        if cols is not None and j not in cols:
            continue
        t = terms[j]
        exact, mag = math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())
        print(f"column {j}: ts {ts[j]!r} fsum {exact!r} bound {t.size * EPS * mag:.3e}")
        assert abs(ts[j] - exact) <= t.size * EPS * mag, (j, ts[j], exact)
        assert bdm.uses_teleport(ts[j])
    return ts


def check_iteration(b, model, terms, ts, cols, advance=None, frozen=()):
    """One iteration (step(1), or `advance`) of the columns `cols` against step_teleport, from the
    device's previous ranks, the dc norms() reports as used and `ts`; `frozen` columns keep their bits."""
    prev = {j: b.ranks(j) for j in list(cols) + list(frozen)}
    if advance is None:
        b.step(1)
    else:
        advance()
    new = {j: b.ranks(j) for j in list(cols) + list(frozen)}
    dc, _ = b.norms()
    for j in cols:
        want = model.step_teleport(prev[j], terms[j], dc[j], ts[j])
        bad = np.nonzero(bits(new[j]) != bits(want))[0]
        assert bad.size == 0, (f"column {j} (ts {ts[j]!r}, dc {dc[j]!r}): {bad.size} of {want.size} ranks differ, first rows "
                               f"{bad[:8].tolist()} with in-degrees {model.indeg[bad[:8]].tolist()}")
        x = prev[j][model.sink]
        assert abs(dc[j] - math.fsum(x.tolist())) <= x.size * EPS * math.fsum(np.abs(x).tolist())
    for j in frozen:
        assert np.array_equal(bits(new[j]), bits(prev[j])), f"frozen column {j} moved"
    return new


def all_bits(b, cols):
    return {j: bits(b.ranks(j)).copy() for j in cols}


def assert_same(a, b, what):
    for j in a:
        diff = np.nonzero(a[j] != b[j])[0]
        assert diff.size == 0, (what, j, diff.size, diff[:8].tolist())


def padding_is_zero(b, width):
    """The columns width .. stride - 1 of the layout hold +0.0 everywhere."""
    for j in range(width, b.info()["stride"]):
        assert not bits(b._ranks_ex(j)).any(), f"padding column {j} is not zero"


# ---- 1. bitwise against the model ----------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 5, 16])
def test_boundary_rows_teleport(hip, boundary, width):
    case, cols = boundary, list(range(width))
    b, model, specs, terms = open_batch(hip, case, width)
    try:
        assert b.dangling == "teleport"
        ts = check_sums(b, specs, terms)
        b.reset(init_ranks=case.init)
        dc0, _ = b.norms()
        assert (dc0 > 0).all()  # the mode has something to move
        for _ in range(3):
            check_iteration(b, model, terms, ts, cols)
            padding_is_zero(b, width)
        single = all_bits(b, cols)
        b.reset(init_ranks=case.init)
        assert b.dangling == "teleport"
        b.step(3)
        assert_same(single, all_bits(b, cols), "step(3) against three single steps")
        assert np.array_equal(bits(b.teleport_sums()), bits(ts))
    finally:
        b.close()


# ---- 2. the until siblings -----------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 5, 16])
def test_until_siblings_teleport(hip, boundary, width):
    case, cols = boundary, list(range(width))
    b, model, specs, terms = open_batch(hip, case, width)
    try:
        ts = check_sums(b, specs, terms)
        b.reset(init_ranks=case.init)
        b.step(3)
        want = all_bits(b, cols)
        b.reset(init_ranks=case.init)
        assert b.step_until(3, 0.0).tolist() == [3] * width
        assert_same(want, all_bits(b, cols), "step_until(3, 0.0) against step(3)")
        # the odd columns advance, the even ones are frozen; at width 1 the single column advances
        active = [j for j in cols if j % 2 == 1] if width > 1 else [0]
        still = [j for j in cols if j not in active]
        mask = sum(1 << j for j in active)

        def advance():
            assert b.step_until_any(mask, 1, 0.0) == (1, 0)

        for _ in range(3):
            check_iteration(b, model, terms, ts, active, advance=advance, frozen=still)
        check_iteration(b, model, terms, ts, cols)
    finally:
        b.close()


# ---- 3. grid trips -------------------------------------------------------------------------------
def test_many_units_teleport(hip, many):
    case, width = many, 16
    cols = [0, 8, 15]
    assert case.V * width > 2 * bom.GRID_MAX * 256  # several trips of k_batch_tsum_col's grid
    b, model, specs, terms = open_batch(hip, case, width)
    try:
        assert b.info()["n_units"] > bom.GRID_MAX
        ts = check_sums(b, specs, terms, cols + [1])
        b.reset(init_ranks=case.init)
        for _ in range(2):
            check_iteration(b, model, terms, ts, cols)
        # the same dense vector in columns 0 and 15; the sparse form of a vector in column 8, its dense
        # form in column 9
        b.set_teleport(15, terms[0])
        sparse = specs[1]
        b.set_teleport_sparse(8, sparse[1], sparse[2], 0.0)
        b.set_teleport(9, terms[1])
        ts2 = b.teleport_sums()
        assert bits(ts2[15])[0] == bits(ts2[0])[0] == bits(ts[0])[0]
        assert bits(ts2[8])[0] == bits(ts2[9])[0] == bits(ts[1])[0]
        untouched = [j for j in range(width) if j not in (8, 9, 15)]
        assert np.array_equal(bits(ts2[untouched]), bits(ts[untouched]))
    finally:
        b.close()


# ---- 4. fallback bits ----------------------------------------------------------------------------
def test_fallback_columns_keep_uniform_bits(hip, boundary):
    case, width = boundary, 16
    zero_col, none_col, real_col = 4, 2, 3  # teleport_columns(): 4 dense, 2 scalar, 3 dense positive
    got = {}
    for mode in ("teleport", "uniform"):
        b, model, specs, terms = open_batch(hip, case, width, mode)
        try:
            assert specs[none_col][0] == "scalar" and specs[real_col][0] == "dense"
            b.set_teleport(zero_col, np.zeros(case.V))
            ts = b.teleport_sums()
            assert bits(ts[zero_col])[0] == 0 and bits(ts[none_col])[0] == 0 and ts[real_col] > 0
            b.reset(init_ranks=case.init)
            b.step(3)
            got[mode] = all_bits(b, (zero_col, none_col, real_col))
        finally:
            b.close()
    for j in (zero_col, none_col):
        assert np.array_equal(got["teleport"][j], got["uniform"][j]), j
    assert not np.array_equal(got["teleport"][real_col], got["uniform"][real_col])


# ---- 5. locality ---------------------------------------------------------------------------------
def test_unreachable_vertices_keep_rank_zero(hip):
    edges = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 4), (5, 6), (6, 7), (7, 5), (6, 8), (9, 5)]
    src = np.array([e[0] for e in edges], np.int32)
    dst = np.array([e[1] for e in edges], np.int32)
    init = np.array([1.0] * 5 + [0.0] * 5)
    far = np.arange(5, 10)
    with hip.PageRankGraph(10, src, dst) as g:
        for mode in ("teleport", "uniform"):
            with hip.PageRankBatch(g, 1) as b:
                b.set_teleport_sparse(0, [0], [1.5], 0.0)
                b.set_dangling(mode)
                assert bits(b.teleport_sums())[0] == bits(1.5)[0]
                b.reset(init_ranks=init)
                for it in range(5):
                    b.step(1)
                    r = b.ranks(0)
                    dc, _ = b.norms()
                    assert dc[0] > 0  # the sinks 3 and 4 hold mass
                    if mode == "teleport":
                        assert np.array_equal(bits(r[far]), np.zeros(5, np.uint64)), (it, r[far])
                        assert (r[:5] > 0).all()
                    else:  # the test can tell the modes apart: the uniform term reaches every vertex
                        assert (r[far] > 0).all(), (it, r[far])


# ---- 6. mode plumbing ----------------------------------------------------------------------------
def test_mode_plumbing(hip, boundary):
    case, width = boundary, 16
    cols = list(range(width))
    a, model, specs, terms = open_batch(hip, case, width, mode=None)   # never touched
    u, _, _, _ = open_batch(hip, case, width, mode="uniform")
    t, _, _, _ = open_batch(hip, case, width, mode="teleport")
    x, _, _, _ = open_batch(hip, case, width, mode=None)
    try:
        assert a.dangling == "uniform" and u.dangling == "uniform" and t.dangling == "teleport"
        bytes_before = a.info()["device_bytes"]
        with pytest.raises(ValueError):
            a.set_dangling("seeds")
        import sparky_hip._lib as L

        for bad in (-1, 2, 7):  # any other mode value: PR_ERR_INVALID, nothing changed
            assert L.load().pr_batch_set_dangling(t._h, bad) == L.PR_ERR_INVALID
        assert t.dangling == "teleport" and a.dangling == "uniform"
        for b in (a, u, t, x):
            b.reset(init_ranks=case.init)
        assert t.dangling == "teleport"  # survives reset
        # the default: the bits of uniform mode, which check_iteration of the boundaries test holds to the
        # uniform model; and no new allocation
        a.step(2)
        u.step(2)
        assert_same(all_bits(a, cols), all_bits(u, cols), "untouched against explicit uniform")
        assert a.info()["device_bytes"] == bytes_before
        prev = a.ranks(1)
        a.step(1)
        dc, _ = a.norms()  # the dc that iteration used
        assert np.array_equal(bits(a.ranks(1)), bits(model.step(prev, terms[1], dc[1])))
        # x switches per iteration: teleport, uniform, uniform, teleport; every iteration is the model's in
        # the mode it ran in, from x's own state
        ts = t.teleport_sums()
        for mode in ("teleport", "uniform", "uniform", "teleport"):
            x.set_dangling(mode)
            assert x.dangling == mode
            prev = {j: x.ranks(j) for j in cols}
            x.step(1)
            dc, _ = x.norms()
            for j in cols:
                want = (model.step_teleport(prev[j], terms[j], dc[j], ts[j]) if mode == "teleport"
                        else model.step(prev[j], terms[j], dc[j]))
                assert np.array_equal(bits(x.ranks(j)), bits(want)), (mode, j)
        assert x.info()["device_bytes"] == bytes_before + 8 * 16
        # switched off and on again without a step in between: an uninterrupted teleport run
        t.step(2)
        t.set_dangling("uniform")
        t.set_dangling("teleport")
        t.step(2)
        y, _, _, _ = open_batch(hip, case, width, mode="teleport")
        try:
            y.reset(init_ranks=case.init)
            y.step(4)
            assert_same(all_bits(y, cols), all_bits(t, cols), "off and on again against an uninterrupted run")
        finally:
            y.close()
    finally:
        for b in (a, u, t, x):
            b.close()


def test_dangling_none_graph_ignores_the_mode(hip):
    case = Case(hip, bom.boundary_graph(), 33, dangling="none")
    try:
        width, cols, got = 16, list(range(16)), {}
        for mode in ("teleport", "uniform"):
            b, model, specs, terms = open_batch(hip, case, width, mode)
            try:
                b.reset(init_ranks=case.init)
                b.step(3)
                dc, _ = b.norms()
                assert (dc == 0.0).all()
                got[mode] = all_bits(b, cols)
                if mode == "teleport":
                    check_sums(b, specs, terms)  # the getter still works
            finally:
                b.close()
        assert_same(got["teleport"], got["uniform"], "PR_DANGLING_NONE: teleport against uniform")
    finally:
        case.close()


# ---- 7. the queue --------------------------------------------------------------------------------
def queue_graph():
    """Like tests/test_gpu_batch_queue.py's 'pack' graph -- V = 300, E = 2500, 5 % records without a
    link -- but with the sources drawn from the first 200 vertices only, so that the other 100 are
    sink-only and a third of the mass is dangling: the two modes then rank differently."""
    rng, V, E = np.random.default_rng(7), 300, 2500
    src = rng.integers(0, 200, E, dtype=np.int64)
    dst = rng.integers(0, V, E, dtype=np.int64)
    dst[rng.random(E) < 0.05] = -1
    seen = np.zeros(V, bool)
    seen[src] = True
    seen[dst[dst >= 0]] = True
    miss = np.nonzero(~seen)[0]
    src = np.concatenate([src, miss])
    dst = np.concatenate([dst, np.full(miss.shape, -1)])
    return V, src.astype(np.int32), dst.astype(np.int32)


def test_run_queue_teleport(hip):
    V, src, dst = queue_graph()
    rng = np.random.default_rng(41)
    queries = []
    for q in range(10):
        k = int(rng.integers(1, 4))
        ids = rng.choice(V, k, replace=False).astype(np.int32)
        mass = 0.15 * V * 10.0 ** rng.uniform(-1.0, 1.5)  # the iteration counts spread with it
        queries.append((ids, mass * (1.0 + np.arange(k)) / k, 0.0))
    width, cap, tol, K = 4, 200, 1e-6, 10
    with hip.PageRankGraph(V, src, dst) as g:
        lists = {}
        for mode in ("teleport", "uniform"):
            got = {}
            with hip.PageRankBatch(g, width) as b:
                b.set_dangling(mode)
                b.reset()

                def on_done(i, column, rec):
                    got[i] = bits(b.ranks(column)).copy()
                    for call in (lambda: b.set_dangling("uniform"), lambda: b.dangling, b.teleport_sums):
                        with pytest.raises(hip.PageRankError) as e:  # like the other entry points
                            call()
                        assert e.value.code == PR_ERR_STATE

                recs = b.run_queue(queries, cap, tol, k=K, on_done=on_done)
                assert b.dangling == mode
                assert b.norms()[0].min() > 0  # there is dangling mass to move
            lists[mode] = [r["topk"][0].tolist() for r in recs]
            assert len({r["iterations"] for r in recs}) >= 2  # the columns were refilled at different times
            for q, (ids, values, rest) in enumerate(queries):
                with hip.PageRankBatch(g, width) as f:  # a fresh batch in the same mode, the vector in column 0
                    f.set_dangling(mode)
                    f.set_teleport_sparse(0, ids, values, rest)
                    f.reset()
                    f.step(recs[q]["iterations"])
                    assert np.array_equal(bits(f.ranks(0)), got[q]), (mode, q, recs[q])
                    if recs[q]["converged"]:
                        _, l1 = f.norms()
                        assert l1[0] <= tol
                        if recs[q]["iterations"] > 1:
                            with hip.PageRankBatch(g, width) as e:  # and not an iteration earlier
                                e.set_dangling(mode)
                                e.set_teleport_sparse(0, ids, values, rest)
                                e.reset()
                                e.step(recs[q]["iterations"] - 1)
                                assert e.norms()[1][0] > tol, (mode, q)
        assert lists["teleport"] != lists["uniform"]  # the queue does not ignore the mode


# ---- 8. both CLIs --------------------------------------------------------------------------------
def test_cli_dangling_to_seeds(hip, tmp_path):
    from sparky_hip import read_edge_list
    from sparky_hip._host import seed_teleport
    from sparky_hip.driver import java_double_to_string

    rng = np.random.default_rng(51)
    lines = [f"u{int(s)} u{int(d)}" for s, d in zip(rng.integers(0, 40, 300), rng.integers(0, 60, 300))]  # u40.. are sinks
    inp, fa, fb = tmp_path / "edges.txt", tmp_path / "a.txt", tmp_path / "b.txt"
    inp.write_text("\n".join(lines) + "\n")
    fa.write_text("u3 2\nu7\n")
    fb.write_text("u11\n")
    urls, src, dst = read_edge_list(lines)
    index = {u: i for i, u in enumerate(urls)}
    sets = [(np.array([index["u3"], index["u7"]], np.int32), seed_teleport([2.0, 1.0], len(urls))),
            (np.array([index["u11"]], np.int32), seed_teleport([1.0], len(urls)))]
    want = {}
    with hip.PageRankGraph(len(urls), src, dst) as g:
        for mode in ("teleport", "uniform"):
            with hip.PageRankBatch(g, 2) as b:
                b.set_dangling(mode)
                for j, (ids, values) in enumerate(sets):
                    b.set_teleport_sparse(j, ids, values)
                b.reset()
                b.step(8)
                assert (b.norms()[0] > 0).all()
                text = "".join(f"Starting iter{i}\n" for i in range(8))
                for j, f in enumerate((fa, fb)):
                    ids, ranks = b.topk(j, 5)
                    text += f"# seed set {j}: {f}\n"
                    text += "".join(f"{urls[i]} has rank: {java_double_to_string(float(r))}.\n" for i, r in zip(ids, ranks))
                want[mode] = text
    assert want["teleport"] != want["uniform"]
    args = [str(inp), "8", "--seed-set", str(fa), "--seed-set", str(fb), "--top", "5"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    out = {}
    for runner, base in (("cpp", [CLI]), ("python", [sys.executable, "-m", "sparky_hip"])):
        res = subprocess.run(base + args + ["--dangling-to-seeds"], capture_output=True, env=env, timeout=120)
        assert res.returncode == 0, res.stderr
        out[runner] = res.stdout
    assert out["cpp"] == out["python"]  # identical bytes
    assert out["cpp"].decode() == want["teleport"]
    res = subprocess.run([CLI] + args, capture_output=True, env=env, timeout=120)
    assert res.returncode == 0 and res.stdout.decode() == want["uniform"]  # without the option: as before
