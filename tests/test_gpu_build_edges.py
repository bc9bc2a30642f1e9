"""The device-side graph build at the boundaries of its own loops, against tests/build_model.py.

pr_build.hip packs, sorts (pr_sort.hip), dedupes (pr_compact.h) and lays the graph out; every other
GPU test feeds it graphs sized for the iteration.  The cases here (build_model.CASES) sit on the build's
edges instead: the sort's partial last tile at tile, wave-slice and ballot-row counts; key widths 2b
from 2 to 34 bits (one to five passes, last digits of 2, 4, 6 and 8 bits, the largest real key next
to the all-ones sentinel); exactly 2048 x 2048 keys and one more (the second tile of a workgroup);
duplicate runs across a compaction tile, a thread's 8-item slice and position 0; m = 0, m = 1 and m on
a tile edge; inputs that are 90 % records without links.  tests/test_build_model_cpu.py asserts that
each case reaches its boundary and that the model equals the C oracle bit for bit.

Bars: export_csr() and the counters of info() equal the model exactly.  The degree-order sort, the
per-part compaction, the local-key sort and the plan are not exported, so every case with V >= 2
also iterates twice against oracle_c.run on the model's CSR at the project's bars (RANK_TOL, dc and
L1 to 1e-9, as tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

import build_model as bm
from sparky_hip import _lib

pytestmark = pytest.mark.gpu

RANK_TOL = 1e-9  # north_star: "ranks within 1e-9 max relative error"
ITERS = 2
COUNTERS = ("n_vertices", "n_edges", "n_sink", "n_nolink", "n_indeg0", "max_indeg")
LAYOUTS = {"fused": dict(layout="fused"), "split": dict(layout="split", options={"classes": 8})}


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.abs(b)))


_REF = {}


def reference(oracle_c, name):
    """oracle_c.run on the model's CSR, once per case."""
    if name not in _REF:
        m = bm.case_inputs(name)[2]
        csr = oracle_c.CSR(m.n_vertices, m.row_ptr, m.col_idx, m.out_deg, m.vflags)
        _REF[name] = oracle_c.run(csr, ITERS, keep_history=True)
    return _REF[name]


def assert_build_equals_model(g, m):
    ex = g.export_csr()
    for a in ("row_ptr", "col_idx", "out_deg", "vflags"):
        got, want = getattr(ex, a), getattr(m, a)
        assert got.shape == want.shape, a
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (a, "first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size)
    inf = g.info()
    assert {k: inf[k] for k in COUNTERS} == m.counters
    return inf


def assert_layout(inf, layout):
    assert inf["layout"] == {"fused": 0, "split": 1}[layout]
    assert inf["classes"] == (8 if layout == "split" else 1)


def check_case(hip, oracle_c, name, layout):
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    with hip.PageRankGraph(c.V, src, dst, **LAYOUTS[layout]) as g:
        inf = assert_build_equals_model(g, m)
        assert_layout(inf, layout)
        assert inf["local_rows"] == c.V and inf["local_edges"] == m.n_edges
        if c.V < 2:
            return
        ref = reference(oracle_c, name)
        hist = []
        ranks, stats = g.run(ITERS, want_ranks_in_callback=True, callback=lambda it, r, st: hist.append(r))
    for it in range(ITERS):
        assert max_rel(hist[it], ref["history"][it]) <= RANK_TOL, it
        assert abs(stats[it].dangling_sum - ref["dc"][it]) <= 1e-9 * max(ref["dc"][it], 1.0), it
        assert abs(stats[it].l1_delta - ref["l1"][it]) <= 1e-9 * max(ref["l1"][it], 1.0), it
    assert np.array_equal(ranks, hist[-1])


@pytest.mark.parametrize("layout", ["fused", "split"])
@pytest.mark.parametrize("name", [c.name for c in bm.CASES if not c.big])
def test_build_case(hip, oracle_c, name, layout):
    check_case(hip, oracle_c, name, layout)


# above 1 M edges: one layout each, alternating
@pytest.mark.parametrize("name,layout", [(c.name, ("fused", "split")[i % 2])
                                         for i, c in enumerate(c for c in bm.CASES if c.big)])
def test_build_case_past_one_tile_per_workgroup(hip, oracle_c, name, layout):
    m = bm.case_inputs(name)[2]
    if name == "tpw2_dedup":  # the dedupe output, the per-part compaction and the local-key sort too
        assert m.n_edges > 4_194_304
    check_case(hip, oracle_c, name, layout)


@pytest.mark.parametrize("name,P", bm.PART_CASES)
def test_build_case_as_parts(hip, oracle_c, name, P):
    """The same inputs as parts of a row partition: the per-part filter (PartPred / PartXform through
    compact_index) and the local-key sort at other counts and widths."""
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    layout = ("fused", "split")[P % 2]
    parts = []
    try:
        for p in range(P):
            parts.append(hip.PageRankGraph(c.V, src, dst, part=p, n_parts=P, keep_canonical=False, **LAYOUTS[layout]))
        infos = [g.info() for g in parts]
        for p, inf in enumerate(infos):
            assert {k: inf[k] for k in COUNTERS} == m.counters
            assert (inf["part"], inf["n_parts"]) == (p, P)
            assert_layout(inf, layout)
        assert sum(i["local_edges"] for i in infos) == m.n_edges
        assert sum(i["local_rows"] for i in infos) == c.V
        # parts own every P-th vertex of the degree order (out-degree descending, ID ascending)
        rank_of = np.empty(c.V, np.int64)
        rank_of[np.lexsort((np.arange(c.V), -m.out_deg.astype(np.int64)))] = np.arange(c.V)
        owner = rank_of % P
        rows = np.repeat(np.arange(c.V), np.diff(m.row_ptr))
        assert [i["local_edges"] for i in infos] == np.bincount(owner[rows], minlength=P).tolist()
        assert [i["local_rows"] for i in infos] == np.bincount(owner, minlength=P).tolist()
        r = hip.PartGroup(parts).run(ITERS)
    finally:
        for g in parts:
            g.close()
    assert not np.isnan(r).any()
    assert max_rel(r, reference(oracle_c, name)["ranks"]) <= RANK_TOL


# ---- validation ------------------------------------------------------------------------------------
VALID = "tail_E4097"  # 4097 edges over V = 300: three sort tiles, the last of one key
MSG_RANGE, MSG_APPEAR = "outside [0, n_vertices)", "never appears"


def expect_invalid_then_valid(hip, V, src, dst, msg, other):
    with pytest.raises(hip.PageRankError) as e:
        hip.PageRankGraph(V, src, dst)
    assert e.value.code == _lib.PR_ERR_INVALID == -1
    assert msg in str(e.value) and other not in str(e.value)
    # the next build of the same process is unharmed
    vs, vd, m = bm.case_inputs(VALID)
    with hip.PageRankGraph(V, vs, vd) as g:
        assert_build_equals_model(g, m)


@pytest.mark.parametrize("index", [0, 2048, 4096])
@pytest.mark.parametrize("field,value", [("src", -1), ("src", "V"), ("dst", -2), ("dst", "V")])
def test_one_bad_id_is_refused(hip, field, value, index):
    c = bm.CASE_BY_NAME[VALID]
    vs, vd, _ = bm.case_inputs(VALID)
    assert vs.shape == (4097,) and c.V == 300
    src, dst = vs.copy(), vd.copy()
    (src if field == "src" else dst)[index] = c.V if value == "V" else value
    expect_invalid_then_valid(hip, c.V, src, dst, MSG_RANGE, MSG_APPEAR)


@pytest.mark.parametrize("which", ["first", "last"])
def test_a_missing_id_is_refused(hip, which):
    c = bm.CASE_BY_NAME[VALID]
    vs, vd, _ = bm.case_inputs(VALID)
    v = 0 if which == "first" else c.V - 1
    keep = (vs != v) & (vd != v)
    assert 0 < keep.sum() < keep.size
    # every other ID still appears: only v is missing
    seen = np.zeros(c.V, bool)
    seen[vs[keep]] = True
    seen[vd[keep]] = True
    assert (~seen).nonzero()[0].tolist() == [v]
    expect_invalid_then_valid(hip, c.V, vs[keep], vd[keep], MSG_APPEAR, MSG_RANGE)
