"""k_spmv_hot's dense cold gathers (pr_spmv.h wave_unit_gather_compact) at small shapes, bitwise.

The size rule (pr_iter.hip kDenseUnitsPerCU) picks the dense path only for passes of ~134 M
in-links, so every small test runs the per-position gathers; PR_OPT_HOT_GATHER forces either path.
Every case here runs one handle twice, per-position then dense, from per-vertex random initial
ranks (every contribution distinct from iteration 1 on, so a misrouted value shows), and asserts:

* info()["hot_gather"] follows the setting;
* ranks after every iteration, and every iteration's dangling sum and L1 delta: bit-identical
  between the two paths (pr_spmv.h: the dense v[j] "is bitwise the per-position a + b");
* the dense run against the oracle: 1e-9 relative for ranks, dc and L1 (RANK_TOL, as
  test_gpu_parity.py test_random_graphs).

Forced dense at a few units per CU also reaches what a full-size pass meets only at class tails:
classes with fewer units than waves (the wave returns before it touches a unit) and the empty
sentinel unit (all padding codes: no cold entry, no round).
"""
import ctypes

import numpy as np
import pytest

import hot_gather_inputs as hgi

pytestmark = pytest.mark.gpu

RANK_TOL = 1e-9  # north_star: "ranks within 1e-9 max relative error"


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def bits(x):
    return np.float64(x).tobytes()


class Case:
    """A graph, its random initial ranks and the oracle's run from them (computed once, shared)."""

    def __init__(self, oracle_c, V, src, dst, iters, seed):
        self.V, self.src, self.dst, self.iters = V, src, dst, iters
        self.init = np.random.default_rng(seed).uniform(0.5, 1.5, V)
        self.csr = oracle_c.build_csr(V, src, dst)
        self.ref = oracle_c.run(self.csr, iters, init=self.init, keep_history=True)
        for a in (self.src, self.dst, self.init, self.ref["history"]):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def boundary(oracle_c):
    V, src, dst, plan = hgi.boundary_graph()
    c = Case(oracle_c, V, src, dst, 6, 11)
    c.plan = plan
    return c


@pytest.fixture(scope="module")
def mixed(oracle_c):
    V = 60000
    src, dst = hgi.random_edges(np.random.default_rng(811), V, 700000, hub_frac=0.03)
    return Case(oracle_c, V, src, dst, 8, 12)


@pytest.fixture(scope="module")
def parts_case(oracle_c):
    V = 50003
    src, dst = hgi.random_edges(np.random.default_rng(812), V, 600000, hub_frac=0.03)
    return Case(oracle_c, V, src, dst, 7, 13)


def run_mode(g, case, mode):
    """One run of `g` on gather path `mode`: (per-iteration ranks, per-iteration stats, final ranks)."""
    g.set_hot_gather(mode)
    assert g.info()["hot_gather"] == mode
    hist = []
    ranks, stats = g.run(case.iters, init_ranks=case.init, want_ranks_in_callback=True,
                         callback=lambda it, r, st: hist.append(r))
    assert g.info()["hot_gather"] == mode
    assert len(hist) == case.iters and np.array_equal(ranks, hist[-1])
    return hist, [(s.dangling_sum, s.l1_delta) for s in stats]


def assert_bitwise(a, b):
    (hist_a, norms_a), (hist_b, norms_b) = a, b
    assert len(hist_a) == len(hist_b) == len(norms_a) == len(norms_b)
    for it in range(len(hist_a)):
        diff = np.nonzero(hist_a[it] != hist_b[it])[0]
        assert np.array_equal(hist_a[it], hist_b[it]), ("ranks", it, diff.size, diff[:8].tolist())
        assert bits(norms_a[it][0]) == bits(norms_b[it][0]), ("dangling_sum", it)
        assert bits(norms_a[it][1]) == bits(norms_b[it][1]), ("l1_delta", it)


def assert_oracle(run, case):
    hist, norms = run
    ref = case.ref
    for it in range(case.iters):
        assert max_rel(hist[it], ref["history"][it]) <= RANK_TOL, it
        assert abs(norms[it][0] - ref["dc"][it]) <= RANK_TOL * max(ref["dc"][it], 1.0), it
        assert abs(norms[it][1] - ref["l1"][it]) <= 1e-9 * max(ref["l1"][it], 1.0), it


def both_paths(g, case):
    per_pos = run_mode(g, case, 0)
    dense = run_mode(g, case, 1)
    assert_bitwise(per_pos, dense)
    assert_oracle(dense, case)
    return dense


@pytest.mark.parametrize("codes,code_bits", [(-1, 20), (0, 32)])
def test_boundary_units(hip, boundary, codes, code_bits):
    """hot_gather_inputs.boundary_graph: hubs whose single (row, class) segment has 512 + m in-links,
    all cold (no hot set), so the last PIECE unit of each has exactly m cold entries, m on both sides
    of every 64-entry load, of the 128-value half and of the 256-entry round of the dense gathers,
    1 and 512; a segment of exactly 512 (a full STREAM unit: two full rounds) and of 1024 / 1025.
    With the 2.5-byte codes and with the 32-bit codes (k_spmv_hot<kCodeU32, true>, which no other
    test runs).  The exported CSR is the oracle's, which test_hot_gather_inputs_cpu.py proves these
    segment lengths from."""
    case, plan = boundary, boundary.plan
    opts = {"classes": plan["C"], "hot_slots": 0, "codes": codes}
    with hip.PageRankGraph(case.V, case.src, case.dst, layout="split", options=opts) as g:
        info = g.info()
        assert info["classes"] == plan["C"] and info["layout"] == 1 and info["hot_slots"] == 0
        assert info["code_bits"] == code_bits
        # every listed hub but the one of exactly 512 in-links (one STREAM unit) is cut into pieces
        assert info["n_long_rows"] >= sum(L > hgi.WAVE_UNIT for L in plan["hub_len"]) == plan["n_listed"] - 1
        ex = g.export_csr()
        assert np.array_equal(ex.row_ptr, case.csr.row_ptr) and np.array_equal(ex.col_idx, case.csr.col_idx)
        assert np.array_equal(ex.out_deg, case.csr.out_deg) and np.array_equal(ex.vflags, case.csr.vflags)
        dense = both_paths(g, case)
    # the hubs' own ranks: every one a sum over pieces whose last has the listed cold count
    hubs = np.arange(plan["n_listed"])
    assert max_rel(dense[0][-1][hubs], case.ref["history"][-1][hubs]) <= RANK_TOL


@pytest.mark.parametrize("slots", [0, 37, 300, 1000, -1])
@pytest.mark.parametrize("classes", [8, 16, 64])
def test_mixed_hot_and_cold_units(hip, mixed, classes, slots):
    """STREAM units that mix hot and cold entries: the hot set sweeps the cold share per unit from all
    (0 slots) over nearly all and nearly none to none (-1: every class region is hot at this size, so
    a unit has zero rounds and the LDS reads alone stand), with 1 to 4 loads per round and second
    rounds across thousands of units, plus the hub's pieces."""
    case = mixed
    opts = {"classes": classes, "hot_slots": slots}
    with hip.PageRankGraph(case.V, case.src, case.dst, keep_canonical=False, layout="split", options=opts) as g:
        info = g.info()
        assert info["classes"] == classes and info["code_bits"] == 20
        if slots >= 0:
            assert info["hot_slots"] == slots
        both_paths(g, case)


def group_run(hip, parts, case, mode):
    """The parts on gather path `mode` (set before the group is made): the final ranks of 7
    iterations split over two step calls (with chunked runs the second starts with chunks pending
    and the hot kernel runs phase by phase), then the same iterations one by one with every
    iteration's ranks, dc and L1 (part 0's view: every part sums all parts' slots in part order)."""
    for p in parts:
        p.set_hot_gather(mode)
        assert p.info()["hot_gather"] == mode
    grp = hip.PartGroup(parts)
    grp.reset(init_ranks=case.init)
    grp.step(case.iters // 2)
    grp.step(case.iters - case.iters // 2)
    grp.sync()
    final = grp.ranks()
    grp.reset(init_ranks=case.init)
    hist, norms = [], []
    for _ in range(case.iters):
        grp.step(1)
        grp.sync()
        hist.append(grp.ranks())
        st = parts[0].stats()
        norms.append((st["last_dc"], st["last_l1"]))
    assert not np.isnan(final).any() and np.array_equal(final, hist[-1])
    return hist, norms


@pytest.mark.parametrize("P,classes,slots,chunks", [(2, 16, -1, 0), (3, 32, 300, 1), (8, 64, 0, 1)])
def test_piece_codes(hip, parts_case, P, classes, slots, chunks):
    """The parts of a row partition (piece codes, kCodeC20P: a cold code maps back to a gather
    offset through the class's LDS table before it is compacted), in one process on one GPU; with
    whole runs and with chunked runs, where k_spmv_hot is launched phase by phase."""
    case = parts_case
    opts = {"classes": classes, "hot_slots": slots, "xchg_chunks": chunks}
    parts = [hip.PageRankGraph(case.V, case.src, case.dst, part=p, n_parts=P, keep_canonical=False,
                               layout="split", options=opts) for p in range(P)]
    try:
        assert all(p.info()["code_bits"] == 20 and p.info()["classes"] == classes for p in parts)
        per_pos = group_run(hip, parts, case, 0)
        dense = group_run(hip, parts, case, 1)
    finally:
        for p in parts:
            p.close()
    assert_bitwise(per_pos, dense)
    assert_oracle(dense, case)


def test_dense_with_reserved_cus(hip, mixed):
    """The size rule is keyed on the full grid; the forced path must not depend on the grid: dense
    gathers with one CU per XCD left free (PR_OPT_HOT_RESERVE) against per-position gathers on every
    CU, bitwise."""
    case = mixed
    with hip.PageRankGraph(case.V, case.src, case.dst, keep_canonical=False, layout="split",
                           options={"classes": 32, "hot_slots": 300}) as g:
        g.set_hot_reserve(0)
        per_pos = run_mode(g, case, 0)
        g.set_hot_reserve(1)
        dense = run_mode(g, case, 1)
    assert_bitwise(per_pos, dense)
    assert_oracle(dense, case)


def test_policy_and_argument_checks(hip):
    """The default is the size rule (a small split graph: per-position gathers) and -1 returns to it;
    a fused-layout handle accepts the option without effect; values other than -1, 0, 1 are
    PR_ERR_INVALID and change nothing."""
    from sparky_hip import _lib

    L = _lib.load()
    V = 4000
    src, dst = hgi.random_edges(np.random.default_rng(5), V, 40000, hub_frac=0.02)
    with hip.PageRankGraph(V, src, dst, keep_canonical=False, layout="split", options={"classes": 8}) as g:
        assert g.info()["classes"] == 8 and g.info()["hot_gather"] == 0
        g.set_hot_gather(1)
        assert g.info()["hot_gather"] == 1
        for bad in (2, -2):
            assert L.pr_set_option(g._h, _lib.PR_OPT_HOT_GATHER, bad) == _lib.PR_ERR_INVALID
            assert g.info()["hot_gather"] == 1
        g.set_hot_gather(-1)
        assert g.info()["hot_gather"] == 0
        old = np.zeros(24, np.int64)  # a caller built against 24 info entries keeps working
        assert L.pr_graph_info(g._h, ctypes.c_void_p(old.ctypes.data), 24) == _lib.PR_OK
        assert old[13] == 8 and old[23] == g.info()["code_bits"]
    with hip.PageRankGraph(V, src, dst, keep_canonical=False, layout="fused") as g:
        assert g.info()["classes"] == 1 and g.info()["hot_gather"] == 0
        for mode in (1, 0, -1):
            g.set_hot_gather(mode)
            assert g.info()["hot_gather"] == 0
        for bad in (2, -2):
            assert L.pr_set_option(g._h, _lib.PR_OPT_HOT_GATHER, bad) == _lib.PR_ERR_INVALID
        g.set_hot_gather(1)
        r, _ = g.run(3)
        assert np.isfinite(r).all()
