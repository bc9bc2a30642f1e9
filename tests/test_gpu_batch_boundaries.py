"""The batch iteration (csrc/pr_batch.hip: k_batch_units, k_batch_long, k_batch_finalize, their
_until siblings, k_batch_reset and k_batch_reset_col) at its unit, chunk and grid boundaries,
bitwise.

Reference: tests/batch_order_model.py, the iteration with every row sum in the order that
csrc/pr_batch.h documents, one separately rounded float64 operation at a time.  The ranks are
compared as uint64 views: no tolerance.  The two per-column norms are sums whose order spans the
whole grid, so they are held to a derived bound against math.fsum instead:

  dc   |dc - fsum(x)| <= n_sink 2^-52 sum|x| over x = the previous ranks of the PR_VF_SINK vertices:
       twice the first-order worst case (n - 1) 2^-53 sum|x| of any order of n additions
  l1   the terms |new - prev| in float64 are the device's own terms bit for bit once the ranks are,
       so |l1 - fsum(terms)| <= V 2^-52 sum(terms), by the same argument

Inputs (batch_order_model, proven on the CPU by tests/test_batch_order_model_cpu.py):
boundary_graph() puts rows on both sides of every switch -- the 8 / 9 in-link switch between the
one-group path and row_sum, G - 1 / G / G + 1 and the unroll-by-4 edge for every G, cap - 1 / cap /
cap + 1 / 2 cap / 2 cap + 1 for every stride's cap, a 64-row unit with empty first and last rows, a
unit of empty rows only, a unit closed at exactly cap, long rows at row 0, at row V - 1 and side by
side; many_units_graph() has more units than k_batch_units has waves and more elements than
k_batch_reset has threads, so their grid-stride loops take further trips.

Every batch starts from per-vertex random ranks and has a distinct teleport vector per column (dense
with negative entries, sparse with rest = 0.0, scalar, dense positive), so that a misrouted or
misordered value changes bits.
"""
import math

import numpy as np
import pytest

import batch_order_model as bom

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Case:
    """A graph on the device, its exported CSR, the random initial ranks and one model per stride."""

    def __init__(self, hip, oracle_c, made, seed, dangling="local"):
        self.V, self.src, self.dst, self.plan = made
        self.dangling_none = dangling == "none"
        self.g = hip.PageRankGraph(self.V, self.src, self.dst, dangling=dangling)
        self.csr = self.g.export_csr()
        ref = oracle_c.build_csr(self.V, self.src, self.dst)  # the CSR the CPU tests prove the rows from
        assert np.array_equal(self.csr.row_ptr, ref.row_ptr) and np.array_equal(self.csr.col_idx, ref.col_idx)
        assert np.array_equal(self.csr.out_deg, ref.out_deg) and np.array_equal(self.csr.vflags, ref.vflags)
        assert np.array_equal(np.diff(self.csr.row_ptr), self.plan["indeg"])
        rng = np.random.default_rng(seed)
        self.init = rng.uniform(0.5, 1.5, self.V)
        self.init2 = rng.uniform(0.5, 1.5, self.V)
        self.init.setflags(write=False)
        self.init2.setflags(write=False)
        self.seed = seed
        self._models = {}

    def model(self, stride):
        if stride not in self._models:
            self._models[stride] = bom.BatchModel(self.csr, stride, self.dangling_none)
        return self._models[stride]

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def boundary(hip, oracle_c):
    c = Case(hip, oracle_c, bom.boundary_graph(), 21)
    yield c
    c.close()


@pytest.fixture(scope="module")
def many(hip, oracle_c):
    c = Case(hip, oracle_c, bom.many_units_graph(), 22)
    yield c
    c.close()


def open_batch(hip, case, width):
    """A batch with its teleport vectors set; returns (batch, model, terms)."""
    b = hip.PageRankBatch(case.g, width)
    specs, terms = bom.teleport_columns(case.V, width, case.seed + 100)
    for j, s in enumerate(specs):
        if s[0] == "dense":
            b.set_teleport(j, s[1])
        elif s[0] == "sparse":
            b.set_teleport_sparse(j, s[1], s[2], 0.0)
    assert b.info()["stride"] == bom.stride_of(width)
    return b, case.model(bom.stride_of(width)), terms


def explain(model, prev, t, dc, got, want):
    """Where device and model differ, and how far each is from the iteration with math.fsum row sums:
    both close means another order of the same sum, one far means a wrong value."""
    bad = np.nonzero(bits(got) != bits(want))[0]
    rows = bad[:8].tolist()
    err_dev = err_model = 0.0
    for v in bad[:200].tolist():
        exact = t[v] + 0.85 * (model.exact_row_sum(prev, v) + dc / model.V)
        scale = model.abs_row_sum(prev, v) + abs(t[v]) + abs(dc / model.V)
        err_dev = max(err_dev, abs(got[v] - exact) / scale)
        err_model = max(err_model, abs(want[v] - exact) / scale)
    return (f"{bad.size} of {got.size} ranks differ; first rows {rows} with in-degrees "
            f"{model.indeg[rows].tolist()}; largest error against fsum row sums, relative to the sum of "
            f"magnitudes: device {err_dev:.3e}, model {err_model:.3e}")


def check_iteration(b, case, model, terms, cols, advance=None, frozen=()):
    """One iteration (step(1), or `advance`) checked in the columns `cols` against the model, from the
    device's own previous ranks and the dc that norms() reports as used; `frozen` columns must keep
    their bits.  Returns the new ranks per column."""
    prev = {j: b.ranks(j) for j in list(cols) + list(frozen)}
    if advance is None:
        b.step(1)
    else:
        advance()
    new = {j: b.ranks(j) for j in list(cols) + list(frozen)}
    dc, l1 = b.norms()
    sink = model.sink
    for j in cols:
        want = model.step(prev[j], terms[j], dc[j])
        same = np.array_equal(bits(new[j]), bits(want))
        assert same, f"column {j}: " + explain(model, prev[j], terms[j], float(dc[j]), new[j], want)
        x = prev[j][sink]
        dc_exact, dc_abs = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist())
        print(f"column {j}: dc {dc[j]!r} fsum {dc_exact!r} bound {x.size * EPS * dc_abs:.3e}")
        assert abs(dc[j] - dc_exact) <= x.size * EPS * dc_abs, (j, dc[j], dc_exact)
        if case.dangling_none:
            assert dc[j] == 0.0
        moved = np.abs(new[j] - prev[j])
        l1_exact = math.fsum(moved.tolist())
        print(f"column {j}: l1 {l1[j]!r} fsum {l1_exact!r} bound {model.V * EPS * l1_exact:.3e}")
        assert abs(l1[j] - l1_exact) <= model.V * EPS * l1_exact, (j, l1[j], l1_exact)
    for j in frozen:
        assert np.array_equal(bits(new[j]), bits(prev[j])), f"frozen column {j} moved"
    return new


def all_bits(b, cols):
    return {j: bits(b.ranks(j)).copy() for j in cols}


def assert_same(a, b, what):
    for j in a:
        diff = np.nonzero(a[j] != b[j])[0]
        assert diff.size == 0, (what, j, diff.size, diff[:8].tolist())


# ---- the boundary graph --------------------------------------------------------------------------
def boundary_rows(hip, case, width):
    cols = list(range(width))
    b, model, terms = open_batch(hip, case, width)
    try:
        assert b.info()["n_long_rows"] == int((case.plan["indeg"] > bom.unit_cap(bom.stride_of(width))).sum())
        assert b.info()["n_long_rows"] == len(model.long_rows) >= 10
        b.reset(init_ranks=case.init)
        for _ in range(3):  # the first one also checks k_batch_reset's dangling sums
            check_iteration(b, case, model, terms, cols)
        single = all_bits(b, cols)
        b.reset(init_ranks=case.init)
        b.step(3)
        assert_same(single, all_bits(b, cols), "step(3) against three single steps")
        assert b.info()["iters"] == 3
    finally:
        b.close()


@pytest.mark.parametrize("width", [1, 2, 3, 5, 9, 16])
def test_boundary_rows(hip, boundary, width):
    """Every stride, with padding columns at widths 3, 5 and 9; dangling 'local'."""
    boundary_rows(hip, boundary, width)


def test_boundary_rows_dangling_none(hip, oracle_c):
    """PR_DANGLING_NONE at width 16: no dangling mass anywhere, dc is exactly 0."""
    case = Case(hip, oracle_c, bom.boundary_graph(), 23, dangling="none")
    try:
        assert not case.model(16).sink.any()
        boundary_rows(hip, case, 16)
    finally:
        case.close()


@pytest.mark.parametrize("width", [1, 2, 3, 5, 16])
def test_until_siblings_at_boundaries(hip, boundary, width):
    case, cols = boundary, list(range(width))
    b, model, terms = open_batch(hip, case, width)
    try:
        b.reset(init_ranks=case.init)
        b.step(3)
        want = all_bits(b, cols)
        b.reset(init_ranks=case.init)
        iters = b.step_until(3, 0.0)
        assert iters.tolist() == [3] * width
        assert_same(want, all_bits(b, cols), "step_until(3, 0.0) against step(3)")
        # the odd columns advance, the even ones are frozen (at width 1 the single column advances and
        # nothing is frozen): one iteration per call, so that norms() describes it
        active = [j for j in cols if j % 2 == 1] if width > 1 else [0]
        still = [j for j in cols if j not in active]
        mask = sum(1 << j for j in active)

        def advance():
            executed, converged = b.step_until_any(mask, 1, 0.0)
            assert (executed, converged) == (1, 0)

        for _ in range(3):
            check_iteration(b, case, model, terms, active, advance=advance, frozen=still)
        # every column again: the frozen ones from contributions and dangling sums that were carried
        # cin -> cout three times, on CHUNK rows and 64-row units too
        check_iteration(b, case, model, terms, cols)
    finally:
        b.close()


# ---- the many-units graph ------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 16])
def test_many_units(hip, many, width):
    """More units than waves: a wave's second unit reuses the LDS row sums after the trailing barrier
    and adds to the dangling / L1 partials of its first; k_batch_long's partials follow a full grid."""
    case = many
    cols = sorted({0, width // 2, width - 1})
    b, model, terms = open_batch(hip, case, width)
    try:
        inf = b.info()
        assert 1.2 * bom.GRID_MAX <= inf["n_units"] <= 1.5 * bom.GRID_MAX, inf
        assert inf["n_long_rows"] == len(model.long_rows) >= 1
        b.reset(init_ranks=case.init)
        for _ in range(2):
            check_iteration(b, case, model, terms, cols)
        single = all_bits(b, cols)
        b.reset(init_ranks=case.init)
        assert b.step_until(2, 0.0).tolist() == [2] * width
        assert_same(single, all_bits(b, cols), "step_until(2, 0.0) against two single steps")
    finally:
        b.close()


def test_reset_column_many_trips(hip, many):
    """V * 16 elements are five trips of k_batch_reset's grid: reset_column is bitwise reset there too."""
    case, width = many, 16
    cols = list(range(width))
    assert case.V * width > 2 * bom.GRID_MAX * 256
    b, model, terms = open_batch(hip, case, width)
    fresh, _, _ = open_batch(hip, case, width)
    try:
        fresh.reset(init_ranks=case.init2)
        fresh_dc, fresh_l1 = fresh.norms()
        sink = case.init2[model.sink]
        assert (np.abs(fresh_dc - math.fsum(sink.tolist())) <= sink.size * EPS * math.fsum(np.abs(sink).tolist())).all()
        b.reset(init_ranks=case.init)
        b.step(3)
        picked = (0, 7, 15)
        for j in picked:
            others = [k for k in cols if k != j]
            before = all_bits(b, others)
            dc0, l10 = b.norms()
            b.reset_column(j, case.init2)
            dc, l1 = b.norms()
            assert bits(dc[j])[0] == bits(fresh_dc[j])[0], (j, dc[j], fresh_dc[j])
            assert l1[j] == 0.0
            assert np.array_equal(bits(dc[others]), bits(dc0[others])) and np.array_equal(bits(l1[others]), bits(l10[others]))
            assert_same(before, all_bits(b, others), f"reset_column({j}) touched another column")
            assert np.array_equal(bits(b.ranks(j)), bits(case.init2))
        b.step(2)
        fresh.step(2)
        assert_same(all_bits(fresh, picked), all_bits(b, picked), "a restarted column against the fresh batch")
    finally:
        fresh.close()
        b.close()
