"""tests/build_model.py on the CPU: the numpy model of the canonical build against the C oracle (and, at
V <= 17, against the structure oracle/sparky_rdd.py derives), the edge-list builder against the counts
it was asked for, and every case of the table against the boundary it is in the table for.

The last part is the guard against drift: tests/test_gpu_build_edges.py runs build_model.CASES on the
GPU and relies on each one reaching a particular loop boundary of pr_sort.hip / pr_compact.h.  Here
that is asserted from sort_shape / compact_shape and the sorted keys, not claimed in a comment.
"""
import numpy as np
import pytest

import build_model as bm
import sparky_rdd

CASE_NAMES = [c.name for c in bm.CASES]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_model_equals_oracle_bitwise(oracle_c, name):
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    o = oracle_c.build_csr(c.V, src, dst)
    for a in ("row_ptr", "col_idx", "out_deg", "vflags"):
        got, want = getattr(m, a), getattr(o, a)
        assert got.dtype == want.dtype and got.shape == want.shape, a
        assert np.array_equal(got, want), a
    assert m.counters["n_edges"] == o.n_edges


@pytest.mark.parametrize("name", [c.name for c in bm.CASES if c.V <= 17])
def test_model_equals_rdd_structure(name):
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    g = sparky_rdd.SparkyRDD([(int(s), None if d < 0 else int(d)) for s, d in zip(src, dst)])
    assert g.total_url_count == c.V == m.counters["n_vertices"]
    inl = {v: set() for v in range(c.V)}
    for u, lst in g.all_urls.items():
        for t in lst or ():
            if t is not None:
                inl[t].add(u)
    for v in range(c.V):
        assert sorted(inl[v]) == m.col_idx[m.row_ptr[v]:m.row_ptr[v + 1]].tolist(), v
        lst = g.all_urls[v]
        deg = 0 if lst is None else sum(t is not None for t in lst)
        assert deg == m.out_deg[v]
        want = bm.PR_VF_SINK if lst is None else bm.PR_VF_KEY
        if lst is not None and deg == 0:
            want |= bm.PR_VF_NOLINK
        if not inl[v]:
            want |= bm.PR_VF_INDEG0
        assert m.vflags[v] == want, v
    sinks = {v for v in range(c.V) if m.vflags[v] & bm.PR_VF_SINK}
    assert g.dang_urls == sinks and m.counters["n_sink"] == len(sinks)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_builder_delivers_the_counts(name):
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    assert src.dtype == dst.dtype == np.int32 and src.shape == dst.shape == (c.E,)
    assert int((dst < 0).sum()) == c.n_nolink
    assert m.n_edges == c.m
    seen = np.zeros(c.V, bool)
    seen[src] = True
    seen[dst[dst >= 0]] = True
    assert seen.all()
    # the counters follow from the arrays
    k = m.counters
    indeg = np.diff(m.row_ptr)
    assert k["n_sink"] == int(((m.vflags & bm.PR_VF_SINK) != 0).sum())
    assert k["n_nolink"] == int(((m.vflags & bm.PR_VF_NOLINK) != 0).sum())
    assert k["n_indeg0"] == int((indeg == 0).sum()) and k["max_indeg"] == int(indeg.max())
    assert int(m.out_deg.sum()) == c.m == int(m.row_ptr[-1])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_boundary(name):
    c = bm.CASE_BY_NAME[name]
    src, dst, m = bm.case_inputs(name)
    f = bm.facts(c, src, dst, m)
    assert c.expect, "a case without a stated boundary"
    assert {k: f[k] for k in c.expect} == c.expect


def test_table_covers_the_boundaries():
    """The table as a whole: every digit width and pass count, both sides of the two-tile threshold,
    partial tiles at wave-slice and ballot-row edges, and the dedupe extremes."""
    fs = {}
    for c in bm.CASES:
        src, dst, m = bm.case_inputs(c.name)
        fs[c.name] = bm.facts(c, src, dst, m)
    assert {f["passes"] for f in fs.values()} >= {1, 2, 3, 4, 5}
    assert {f["last_nbits"] for f in fs.values()} >= {2, 4, 6, 8}
    assert {f["two_b"] for n, f in fs.items() if n.startswith("width")} >= {2, 4, 8, 10, 16, 18, 24, 26, 32, 34}
    assert {f["tiles_per_wg"] for f in fs.values()} >= {1, 2}
    assert {f["compact_tpw"] for f in fs.values()} >= {1, 2}
    tails = {f["tail"] for n, f in fs.items() if n.startswith("tail")}
    assert tails >= {2, 63, 64, 65, 511, 512, 513, 2047, 0, 1}
    assert {0, 1} <= {f["m"] for f in fs.values()} and any(f["m_tail"] == 0 and f["m"] > 0 for f in fs.values())
    assert any(f["scan_per"] > 1 for f in fs.values()) and any(f["scan_per"] == 1 for f in fs.values())
    for name, P in bm.PART_CASES:
        assert name in bm.CASE_BY_NAME and P in (2, 3)


def test_sort_and_compact_shape_known_values():
    full = 2048 * 2048
    assert bm.sort_shape(1, 18)["passes"] == 0 and bm.sort_shape(5, 0)["passes"] == 0  # early return
    s = bm.sort_shape(2049, 18)
    assert (s["ntiles"], s["nwg"], s["tiles_per_wg"], s["passes"], s["last_nbits"], s["tail"]) == (2, 2, 1, 3, 2, 1)
    s = bm.sort_shape(full, 24)
    assert (s["ntiles"], s["nwg"], s["tiles_per_wg"], s["passes"], s["last_nbits"], s["tail"]) == (2048, 2048, 1, 3, 8, 0)
    assert s["scan_per"] == 512
    s = bm.sort_shape(full + 1, 24)
    assert (s["ntiles"], s["nwg"], s["tiles_per_wg"]) == (2049, 1025, 2)
    s = bm.sort_shape(3 * full, 6)
    assert (s["ntiles"], s["nwg"], s["tiles_per_wg"], s["passes"], s["last_nbits"]) == (6144, 2048, 3, 1, 6)
    assert bm.compact_shape(0)["nwg"] == 0
    assert bm.compact_shape(2048) == dict(ntiles=1, nwg=1, tiles_per_wg=1, tail=0)
    assert bm.compact_shape(full + 1) == dict(ntiles=2049, nwg=1025, tiles_per_wg=2, tail=1)
    assert [bm.bits_for(v) for v in (0, 1, 2, 3, 4, 255, 256, 65535, 65536)] == [1, 1, 2, 2, 3, 8, 9, 16, 17]


def test_run_copies_places_the_runs():
    rng = np.random.default_rng(0)
    cp = bm.run_copies(50, 120, ((0, 3), (10, 4), (40, 9)), rng)
    keys = np.repeat(np.arange(50), cp)
    assert keys.shape == (120,) and (cp >= 1).all()
    for start, n in ((0, 3), (10, 4), (40, 9)):
        assert len(set(keys[start:start + n])) == 1
        assert start == 0 or keys[start - 1] != keys[start]
        assert keys[start + n] != keys[start]
    with pytest.raises(ValueError):
        bm.run_copies(5, 10, ((0, 3), (2, 2)), rng)  # overlap
    with pytest.raises(ValueError):
        bm.run_copies(3, 10, ((7, 2),), rng)  # beyond the last key
    with pytest.raises(ValueError):
        bm.run_copies(3, 4, ((0, 3),), rng)  # no room for the other keys


def test_builder_fails_rather_than_append():
    with pytest.raises(ValueError, match="never appear"):
        bm.edge_list(300, 10, 10)  # 10 edges cannot mention 300 IDs
    with pytest.raises(ValueError, match="never appear"):
        bm.edge_list(3000, 2000, 1000, n_nolink=5, seed=1)
    with pytest.raises(ValueError):
        bm.edge_list(3, 20, 10)  # m > V * V
    with pytest.raises(ValueError):
        bm.edge_list(3, 5, 0, n_nolink=3)  # duplicates of nothing
    with pytest.raises(ValueError):
        bm.build(3, [0, 1], [1, 0])  # ID 2 never appears
    with pytest.raises(ValueError):
        bm.build(3, [0, 1, 2], [1, 3, 0])


def test_builder_orders_and_determinism():
    a = bm.edge_list(3000, 20000, 1500, n_nolink=18000, seed=7, order="real_first")
    b = bm.edge_list(3000, 20000, 1500, n_nolink=18000, seed=7, order="real_first")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[1][:2000] >= 0).all() and (a[1][2000:] == -1).all()
    c = bm.edge_list(3000, 20000, 1500, n_nolink=18000, seed=7, order="real_last")
    assert (c[1][:18000] == -1).all() and (c[1][18000:] >= 0).all()
    # the forced corner pairs are in
    for V in (2, 3, 300):
        s, d = bm.edge_list(V, 4 * V + 200, min(V * V, 2 * V), n_nolink=100, seed=V)
        have = set(zip(s.tolist(), d.tolist()))
        assert {(0, 0), (V - 1, V - 1), (0, V - 1), (V - 1, 0)} <= have
