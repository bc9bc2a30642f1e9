"""tests/batch_order_model.py proven without a GPU: the vectorised row sum against the lane-level
emulation, bit for bit; the boundary graph's prescribed rows in the oracle's canonical CSR and in
the planner's own output (csrc/pr_batch.h through build/libpr_batch_shim.so) at every stride; the
unit counts of the many-units graph; and the model's iteration on the KAT graph, whose exact ranks
tests/test_gpu_parity.py::test_kat_exact_values lists."""
import ctypes
import os

import numpy as np
import pytest

import batch_order_model as bom
from conftest import PKG_DIR

STRIDES = list(bom.STRIDES)


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_shim.so"))
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.prb_unit_cap.argtypes = [ctypes.c_int]
    lib.prb_plan.argtypes = [P, i64, ctypes.c_int, i64, P, P, P, P, P, P, P]
    lib.prb_plan.restype = i64
    return lib


def shim_plan(shim, row_ptr, stride):
    """prb_plan's units as a list of (e0, row0, rows, n, slot), and n_long."""
    rp = np.ascontiguousarray(row_ptr, np.int64)
    V = len(rp) - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    n_long, n_slots = np.zeros(1, np.int64), np.zeros(1, np.int64)
    cap_units = V + int(rp[-1]) // shim.prb_unit_cap(stride) + 8
    e0 = np.zeros(cap_units, np.int64)
    row0, rows, n, slot = (np.zeros(cap_units, np.int32) for _ in range(4))
    nu = shim.prb_plan(p(rp), V, stride, cap_units, p(e0), p(row0), p(rows), p(n), p(slot), p(n_long), p(n_slots))
    assert 0 <= nu <= cap_units
    units = list(zip(e0[:nu].tolist(), row0[:nu].tolist(), rows[:nu].tolist(), n[:nu].tolist(), slot[:nu].tolist()))
    return units, int(n_long[0])


@pytest.fixture(scope="module")
def boundary(oracle_c):
    V, src, dst, plan = bom.boundary_graph()
    return V, src, dst, plan, oracle_c.build_csr(V, src, dst)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- the row sum ---------------------------------------------------------------------------------
def boundary_lengths(stride):
    """Every row length of (a)-(c) that row_sum takes at this stride, and the chunk lengths of the
    longer ones."""
    G, cap = bom.groups(stride), bom.unit_cap(stride)
    lens = {9, 10}
    for s in STRIDES:
        g = bom.groups(s)
        lens |= {m * g + d for m in (1, 4, 8) for d in (-1, 0, 1)}
    for c in bom.CAPS:
        lens |= {c - 1, c, c + 1, 2 * c, 2 * c + 1}
    out = set()
    for n in lens:
        if n <= cap:
            out.add(n)
        else:
            out |= {cn for _, cn in bom.chunk_ranges(n, cap)}
    # chunks run through row_sum whatever their length; short PACK rows do not, but the order of a
    # chunk of 1..8 in-links is row_sum's too
    return sorted(out | set(range(1, 9)) | {G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1})


@pytest.mark.parametrize("stride", STRIDES)
def test_vectorised_row_sum_is_the_lane_emulation(stride):
    rng = np.random.default_rng(100 + stride)
    G = bom.groups(stride)
    lens = boundary_lengths(stride)
    assert {1, 8, 9, G, G + 1, 4 * G, 4 * G + 1, bom.unit_cap(stride)} <= set(lens)
    for n in lens:
        # signed values spread over 16 decades: any other order of addition changes the bits
        x = rng.choice([-1.0, 1.0], (n, stride)) * 10.0 ** rng.uniform(-8, 8, (n, stride))
        lanes = bom.row_sum_lanes(x, stride)
        for j in range(stride):
            col = lanes[j::stride]
            assert (bits(col) == bits(col)[0]).all(), (n, j)  # every lane group ends with the same bits
            assert bits(bom.row_sum_vec(x[:, j], stride))[0] == bits(col)[0], (n, j)


def test_row_sum_order_matters_for_these_values():
    """The inputs above tell orders apart: the in-order sum of the same values has other bits for most
    rows, so the agreement above is no accident of tame values."""
    rng = np.random.default_rng(7)
    differ = 0
    for _ in range(50):
        x = rng.choice([-1.0, 1.0], 300) * 10.0 ** rng.uniform(-8, 8, 300)
        differ += bits(bom.row_sum_vec(x, 4))[0] != bits(bom._sum_in_order(x[None, :]))[0]
    assert differ >= 25


# ---- the boundary graph --------------------------------------------------------------------------
def test_boundary_graph_rows(boundary):
    V, src, dst, plan, csr = boundary
    assert 13_000 <= V <= 15_000
    indeg = np.diff(csr.row_ptr)
    assert np.array_equal(indeg, plan["indeg"])  # exactly the prescribed in-degrees ...
    assert csr.n_edges == int((dst >= 0).sum()) < 300_000  # ... and no duplicate edge: distinct sources
    for v in (0, V - 1, plan["long_rows"][3]):
        cols = csr.col_idx[csr.row_ptr[v]:csr.row_ptr[v + 1]]
        assert len(np.unique(cols)) == len(cols) == bom.LONG
    # (a), (b), (c)
    assert [d for _, d in plan["rows_a"]] == [0, 1, 2, 7, 8, 9, 10]
    have = {d for _, d in plan["rows_b"]}
    for G in (4, 8, 16, 32, 64):
        assert {m * G + k for m in (1, 4, 8) for k in (-1, 0, 1)} <= have
    have = {d for _, d in plan["rows_c"]}
    for cap in (256, 512, 1024, 2048, 4096):
        assert {cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1} <= have
    for r, d in plan["rows_a"] + plan["rows_b"] + plan["rows_c"]:
        assert indeg[r] == d
    # (g)
    assert indeg[0] == indeg[V - 1] == indeg[V - 2] == bom.LONG
    # (h) and the flag the kernel takes an empty row's sum by
    f = csr.vflags
    assert np.array_equal((f & bom.VF_INDEG0) != 0, indeg == 0)
    assert np.nonzero(f & bom.VF_SINK)[0].tolist() == plan["sinks"] and len(plan["sinks"]) > 100
    assert (indeg[plan["sinks"]] > 0).all() and (csr.out_deg[plan["sinks"]] == 0).all()
    assert indeg[plan["sinks"]].max() == bom.LONG and 4097 in indeg[plan["sinks"]] and 257 in indeg[plan["sinks"]]
    assert np.nonzero(f & bom.VF_NOLINK)[0].tolist() == plan["nolinks"] and len(plan["nolinks"]) > 100
    assert (csr.out_deg[plan["nolinks"]] == 0).all() and (f[plan["nolinks"]] & bom.VF_KEY).all()
    assert (indeg[plan["nolinks"]] > 0).any() and (indeg[plan["nolinks"]] == 0).any()
    keys0 = plan["indeg0_keys"]
    assert len(keys0) > 100 and (indeg[keys0] == 0).all() and (csr.out_deg[keys0] > 0).all()
    assert (csr.out_deg[(f & (bom.VF_SINK | bom.VF_NOLINK)) == 0] > 0).all()


@pytest.mark.parametrize("stride", STRIDES)
def test_boundary_graph_in_the_planner(shim, boundary, stride):
    V, src, dst, plan, csr = boundary
    cap = shim.prb_unit_cap(stride)
    assert cap == bom.unit_cap(stride)
    units, n_long = shim_plan(shim, csr.row_ptr, stride)
    indeg = plan["indeg"]
    assert units == bom.plan_units(csr.row_ptr, stride)  # the restated planner is the planner
    pack = {row0: (rows, n) for _, row0, rows, n, _ in units if rows > 0}
    chunks = {}
    for e0, row0, rows, n, slot in units:
        if rows < 0:
            chunks.setdefault(row0, []).append((e0, n))
    # the model's classification and chunk ranges are the planner's
    m = bom.BatchModel(csr, stride)
    assert m.long_rows.tolist() == sorted(chunks) == np.nonzero(indeg > cap)[0].tolist()
    assert n_long == len(chunks) and [chunks[v] for v in m.long_rows.tolist()] == m.chunks
    kinds = m.kinds()
    in_pack = np.zeros(V, bool)
    for row0, (rows, n) in pack.items():
        in_pack[row0:row0 + rows] = True
    assert np.array_equal(in_pack, kinds != 3)
    assert np.array_equal(kinds == 1, (indeg >= 1) & (indeg <= 8)) and np.array_equal(kinds == 0, indeg == 0)
    # (c) at this stride: one unit of exactly cap, last chunks of 1 in-link and of cap in-links
    by_deg = {d: r for r, d in plan["rows_c"]}
    assert kinds[by_deg[cap - 1]] == 2 and kinds[by_deg[cap]] == 2
    assert [n for _, n in chunks[by_deg[cap + 1]]] == [cap, 1]
    assert [n for _, n in chunks[by_deg[2 * cap]]] == [cap, cap]
    assert [n for _, n in chunks[by_deg[2 * cap + 1]]] == [cap, cap, 1]
    # (d) a unit of 64 rows whose first and last rows are empty
    u = plan["unit64_row0"]
    assert pack[u] == (64, 62) and indeg[u] == 0 and indeg[u + 63] == 0 and (indeg[u + 1:u + 63] == 1).all()
    assert indeg[u - 1] == indeg[u + 64] == bom.LONG
    # (e) a unit of empty rows only
    e = plan["empty_unit_row0"]
    assert pack[e] == (2, 0) and indeg[e - 1] == indeg[e + 2] == bom.LONG
    # (f) a unit closed at exactly n == cap, with 2 rows
    fr = plan["full_unit_row0"][cap]
    assert pack[fr] == (2, cap) and indeg[fr - 1] == bom.LONG and indeg[fr + 2] == 1
    # (g) long rows at both ends and side by side
    assert units[0][1:3] == (0, -1) and units[-1][1] == V - 1 and units[-1][2] < 0
    assert {V - 2, V - 1} <= set(chunks)
    # units of the row limit, and units the capacity closed, both occur
    assert sum(rows == 64 for rows, _ in pack.values()) > 50
    assert any(rows < 64 and n + int(indeg[row0 + rows]) > cap for row0, (rows, n) in pack.items()
               if row0 + rows < V and indeg[row0 + rows] <= cap)


# ---- the many-units graph ------------------------------------------------------------------------
def test_many_units_graph(shim, oracle_c):
    V, src, dst, plan = bom.many_units_graph()
    csr = oracle_c.build_csr(V, src, dst)
    indeg = np.diff(csr.row_ptr)
    assert np.array_equal(indeg, plan["indeg"]) and csr.n_edges == len(src)
    assert 1_900_000 <= csr.n_edges <= 2_100_000
    assert (indeg[0], indeg[V // 2], indeg[V - 1]) == (4097, 9000, 300)
    assert indeg[4:12].tolist() == [1, 0, 9, 2, 1, 0, 9, 2]
    assert np.nonzero(csr.vflags & bom.VF_SINK)[0].tolist() == plan["sinks"] and len(plan["sinks"]) > 1000
    assert np.array_equal((csr.vflags & bom.VF_INDEG0) != 0, indeg == 0)
    for stride in (1, 16):  # more than one trip of k_batch_units' grid-stride loop, for ~2000 waves
        units, n_long = shim_plan(shim, csr.row_ptr, stride)
        assert 1.2 * bom.GRID_MAX <= len(units) <= 1.5 * bom.GRID_MAX, (stride, len(units))
        assert n_long >= 1
        rows = np.array([u[2] for u in units])
        assert (rows[rows > 0] == 64).mean() > 0.99  # the row limit closes the units
    for stride in (4, 8, 16):  # more than one trip of k_batch_reset's grid
        assert V * stride > bom.GRID_MAX * 256


# ---- the iteration -------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_model_on_the_kat(oracle_c, stride):
    from sparky_hip.driver import read_edge_list

    urls, src, dst = read_edge_list(["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"])
    csr = oracle_c.build_csr(len(urls), src, dst)
    m = bom.BatchModel(csr, stride)
    r = np.ones(len(urls))
    dc = float(np.sum(r[m.sink]))
    got = m.step(r, np.full(len(urls), 0.15), dc)
    want = dict(A=1.1416666666666666, B=0.7166666666666667, C=1.9916666666666665,
                D=1.1416666666666666, E=1.1416666666666666, F=0.7166666666666667)
    assert {u: float(x) for u, x in zip(urls, got)} == want


def test_model_tells_strides_apart(boundary):
    """On the GPU tests' own data (random ranks in [0.5, 1.5)) the bits depend on the order: the models
    of two strides agree on every row of at most 8 in-links, whose order is the same at every stride,
    and disagree on a large share of the longer rows (two roundings of one sum coincide often, so not
    on all: about a third of the rows of 9..17 in-links and half of the longer ones; the assertion asks
    for a tenth, hundreds of rows).  A kernel that summed a class of rows in another order, let alone
    lost or doubled an in-link, would not pass a bitwise comparison over this graph."""
    V, src, dst, plan, csr = boundary
    rng = np.random.default_rng(21)
    r = rng.uniform(0.5, 1.5, V)
    a, b = (bom.BatchModel(csr, s).row_sums(r) for s in (1, 16))
    indeg = plan["indeg"]
    same = bits(a) == bits(b)
    assert same[indeg <= 8].all()
    assert (~same[indeg > 8]).mean() > 0.1 and (~same[indeg > 8]).sum() > 200
    assert (~same[indeg > 64]).mean() > 0.1
    # one in-link less in a row of 4G + 1 changes its bits too
    m = bom.BatchModel(csr, 4)
    v = {d: row for row, d in plan["rows_b"]}[4 * 16 + 1]
    x = m.contributions(r)[m.col[csr.row_ptr[v]:csr.row_ptr[v + 1]]]
    assert bits(bom.row_sum_vec(x, 4))[0] != bits(bom.row_sum_vec(x[:-1], 4))[0]


def test_model_against_plain_sums(boundary):
    """The model is the plain iteration up to rounding: every rank within the first-order bound of its
    row's length against math.fsum row sums, at the widest and the narrowest stride."""
    V, src, dst, plan, csr = boundary
    rng = np.random.default_rng(3)
    r, t = rng.uniform(0.5, 1.5, V), rng.uniform(-2.0, 2.0, V)
    eps = 2.0 ** -52
    for stride in (1, 16):
        m = bom.BatchModel(csr, stride)
        got = m.step(r, t, 12.5)
        rows = [v for v, _ in plan["rows_a"] + plan["rows_b"] + plan["rows_c"]] + [0, V - 1, plan["unit64_row0"]]
        for v in rows:
            want = t[v] + 0.85 * (m.exact_row_sum(r, v) + 12.5 / V)
            n = max(int(plan["indeg"][v]), 1)
            assert abs(got[v] - want) <= (n + 4) * eps * (m.abs_row_sum(r, v) + abs(t[v]) + 1.0), (stride, v)
