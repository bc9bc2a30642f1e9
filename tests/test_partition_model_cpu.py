"""tests/partition_model.py without a GPU: the model against the protocol model of
tests/test_dist_cpu.py, the builders' construction claims, and -- for every case that
tests/test_gpu_partition_edges.py runs -- that the input really reaches the edge it is there for,
so that a later change of a shape cannot silently turn an edge case into an ordinary one."""
import numpy as np
import pytest

import partition_model as pm


def build(oracle_c, V, src, dst):
    return oracle_c.build_csr(V, src, dst)


# ---- the model itself ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 9, 16])
def test_pair_counts_are_the_exchange_lists(oracle_c, P):
    """pair[p, q] + 2 is the length of the p -> q list of the protocol model, from either end."""
    rng = np.random.default_rng(P)
    V = 601
    src, dst = pm.random_edges(rng, V, 4000, hub_frac=0.05)
    csr = build(oracle_c, V, src, dst)
    pair = pm.pair_counts(csr, P)
    assert np.all(np.diag(pair) == 0)
    order, rank_of, S_pad, gpos = pm.layout(csr, P)
    for p in range(P):
        send, recv = pm.exchange_lists(p, P, csr, rank_of, S_pad, gpos)
        for q in range(P):
            if q != p:
                assert len(send[q]) == pair[p, q] + 2
                assert len(recv[q]) == pair[q, p] + 2
    xs, xr = pm.sparse_volumes(pair)
    assert xs.sum() == xr.sum() == pair.sum() + 2 * P * (P - 1)
    # each part receives the sources of its cross-part in-links, once each (test_gpu_parity.py's rule)
    own = pm.owners(csr, P)
    rows = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    for q in range(P):
        need = np.unique(csr.col_idx[(own[rows] == q) & (own[csr.col_idx] != q)])
        assert xr[q] == len(need) + 2 * (P - 1)


@pytest.mark.parametrize("V,P", [(0, 3), (1, 2), (5, 8), (64, 64), (65, 64), (20011, 33)])
def test_part_rows(V, P):
    rows = pm.part_rows(V, P)
    assert rows.sum() == V and rows.max() - rows.min() <= 1
    assert np.all(np.diff(rows) <= 0)  # the first V % P parts hold the extra row
    assert np.count_nonzero(rows == 0) == max(0, P - V)


def test_owners_rows_and_edges(oracle_c):
    rng = np.random.default_rng(3)
    V = 777
    src, dst = pm.random_edges(rng, V, 5000)
    csr = build(oracle_c, V, src, dst)
    for P in (1, 2, 9, 64):
        own = pm.owners(csr, P)
        order = np.lexsort((np.arange(V), -csr.out_deg.astype(np.int64)))
        assert np.array_equal(own[order], np.arange(V) % P)
        assert np.array_equal(pm.local_rows(csr, P), pm.part_rows(V, P))
        assert pm.local_edges(csr, P).sum() == csr.n_edges
        indeg = np.diff(csr.row_ptr)
        assert all(pm.local_edges(csr, P)[p] == indeg[own == p].sum() for p in range(P))


def test_geometry_helpers():
    assert [pm.n_chunks(C) for C in (1, 8, 16, 64, 128)] == [1, 1, 2, 8, 16]
    assert pm.classes_with_rows(3, 8) == 3 and pm.classes_with_rows(100, 64) == 64
    assert pm.chunks_with_rows(32, 64) == [0, 1, 2, 3] and pm.chunks_with_rows(9, 64) == [0, 1]
    assert pm.chunks_with_rows(0, 64) == [] and pm.chunks_with_rows(70, 64) == list(range(8))
    assert pm.chunks_with_rows(5, 1) == [0]
    assert [pm.hot_kp(s, 64) for s in (-1, 100, 40)] == [287, 1, 0]  # the figures of the issue


# ---- the builders --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", pm.SILENT_P)
@pytest.mark.parametrize("name", sorted(pm.SILENT_BUILDERS))
def test_silent_builders(oracle_c, name, P):
    V, src, dst = pm.SILENT_BUILDERS[name](P, pm.SILENT_ROWS, pm.SILENT_SINKS)
    assert V == P * (pm.SILENT_ROWS + pm.SILENT_SINKS)
    csr = build(oracle_c, V, src, dst)
    assert csr.n_edges == len(src)  # no duplicate edge
    n_src = P * pm.SILENT_ROWS
    assert np.all(csr.out_deg[:n_src] == 2) and np.all(csr.out_deg[n_src:] == 0)
    assert np.array_equal(pm.owners(csr, P), np.arange(V) % P)
    assert np.all(pm.local_rows(csr, P) == pm.SILENT_ROWS + pm.SILENT_SINKS)
    # the sinks: sink-only vertices (PR_VF_SINK), each read from a source of its own owner, so every
    # part's dangling partial is non-zero and dc has to cross through the slots
    sink = (csr.vflags & oracle_c.VF_SINK) != 0
    assert np.array_equal(np.nonzero(sink)[0], np.arange(n_src, V))
    for v in range(n_src, V):
        cols = csr.col_idx[csr.row_ptr[v]:csr.row_ptr[v + 1]]
        assert len(cols) == 1 and cols[0] % P == v % P
    assert oracle_c.run(csr, 1)["dc"][0] == pm.SILENT_SINKS * P  # every rank starts at 1
    pair = pm.pair_counts(csr, P)
    want = np.zeros((P, P), np.int64)
    if name == "one_way":
        want[0, 1] = pm.SILENT_ROWS - pm.SILENT_SINKS
    assert np.array_equal(pair, want)
    xs, xr = pm.sparse_volumes(pair)
    assert np.array_equal(xs - 2 * (P - 1), want.sum(axis=1)) and np.array_equal(xr - 2 * (P - 1), want.sum(axis=0))


# ---- the GPU file's inputs reach their edges -----------------------------------------------------
@pytest.fixture(scope="module")
def many_csr(oracle_c):
    src, dst = pm.many_edges()
    return build(oracle_c, pm.MANY_V, src, dst)


def test_many_parts_inputs(oracle_c, many_csr):
    csr = many_csr
    V = pm.MANY_V
    assert all(V % d for d in range(2, int(V ** 0.5) + 1))  # prime: no P divides it
    assert np.diff(csr.row_ptr).max() > 2 * 2048  # the hub row is cut into pieces
    Ps = sorted({c[0] for c in pm.MANY_CASES})
    assert Ps == [9, 16, 33, 64] and all(pm.K_MAX_PACK_PARTS < P <= pm.K_MAX_PARTS for P in Ps)
    assert pm.QUERY_P in Ps
    sink = (csr.vflags & oracle_c.VF_SINK) != 0
    assert 240000 <= len(pm.many_edges()[0]) <= 260000
    assert np.array_equal(np.nonzero(sink)[0] % pm.MANY_SINK_EVERY,
                          np.full(np.count_nonzero(sink), pm.MANY_SINK_EVERY - 1))
    assert np.count_nonzero(sink) == len(range(pm.MANY_SINK_EVERY - 1, V, pm.MANY_SINK_EVERY))
    assert oracle_c.run(csr, 3)["dc"].min() > 100  # a dangling sum that matters to every rank
    for P in Ps:
        rows = pm.part_rows(V, P)
        assert rows.max() - rows.min() == 1
        assert np.all(np.bincount(pm.owners(csr, P)[sink], minlength=P) > 0)  # every part's slot counts
        pair = pm.pair_counts(csr, P)
        assert np.all(pair[~np.eye(P, dtype=bool)] > 0)  # every peer pair has traffic here
    # every layout and every hot_slots value at P = 64, and the three hot-set regimes there
    at64 = [(lay, hs) for P, lay, hs in pm.MANY_CASES if P == 64]
    assert {lay for lay, _ in at64} == {pm.FUSED, pm.SPLIT16, pm.SPLIT64}
    assert {hs for lay, hs in at64 if lay[2]} == {-1, 100, 40}
    assert sorted({pm.hot_kp(hs, 64) for lay, hs in at64 if lay[2]}) == [0, 1, 287]
    for P, lay, hs in pm.MANY_CASES:
        assert (hs is None) == (lay[2] is None)
    # Kp = 0 (no hot set, k_hot_tables not launched) is reached at P = 64 only, Kp = 1 at 33 and 64
    kps = {(P, pm.hot_kp(hs, P)) for P, lay, hs in pm.MANY_CASES if lay[2]}
    assert {P for P, kp in kps if kp == 0} == {64} and {P for P, kp in kps if kp == 1} == {33, 64}


@pytest.mark.parametrize("case", pm.TINY_CASES, ids=lambda c: f"V{c.V}-P{c.P}")
def test_tiny_inputs(oracle_c, case):
    V, P = case.V, case.P
    src, dst = pm.tiny_edges(case)
    csr = build(oracle_c, V, src, dst)
    rows = pm.local_rows(csr, P)
    assert np.array_equal(rows, pm.part_rows(V, P))
    if V >= 5:  # no-link records and sinks present (a graph of one or two vertices may have neither)
        assert np.any(csr.vflags & oracle_c.VF_SINK) and np.any(csr.vflags & oracle_c.VF_NOLINK)
        assert np.any(dst == -1)
    if V < P:
        assert np.count_nonzero(rows == 0) == P - V > 0  # parts that own no row
    else:
        assert rows.min() >= 1
    pair = pm.pair_counts(csr, P)
    if P > 2 and V <= 100:
        assert np.any((pair == 0) & ~np.eye(P, dtype=bool))  # pairs that exchange the two slots only
    for name, _, C in pm.TINY_LAYOUTS:
        if C is None:
            continue
        if rows.max() < C:  # whole classes empty on every part
            assert all(pm.classes_with_rows(int(n), C) < C for n in rows)
        if C == 64:
            nc = pm.n_chunks(C)
            assert nc == 8
            if rows.max() <= C - pm.K_XCDS:  # the last chunk of every run holds the slots alone
                assert all(nc - 1 not in pm.chunks_with_rows(int(n), C) for n in rows)
    # which (V, P) reach which edge: pinned, so that a changed shape fails here
    reached = {"zero": V < P, "classes8": rows.max() < 8, "classes64": rows.max() < 64,
               "chunks64": rows.max() <= 56}
    want = {(1, 2): "zero classes8 classes64 chunks64", (2, 2): "classes8 classes64 chunks64",
            (5, 8): "zero classes8 classes64 chunks64", (16, 16): "classes8 classes64 chunks64",
            (65, 64): "classes8 classes64 chunks64", (100, 64): "classes8 classes64 chunks64",
            (2000, 64): "classes64 chunks64"}[(V, P)]
    assert sorted(k for k, v in reached.items() if v) == sorted(want.split())


def test_tiny_special_cases():
    case, lay = pm.TINY_CHUNKED
    assert case in pm.TINY_CASES and lay == pm.SPLIT64 and (case.V, case.P) == (2000, 64)
    rows = pm.part_rows(case.V, case.P)
    assert sorted(set(rows.tolist())) == [31, 32]
    # rows fill classes 0 .. 31 = chunks 0 .. 3; chunks 4 .. 7 of every run are empty but for the slots
    assert all(pm.chunks_with_rows(int(n), 64) == [0, 1, 2, 3] for n in rows)
    case, lay = pm.TINY_NONE
    assert case in pm.TINY_CASES and lay in pm.TINY_LAYOUTS
    assert {(c.V, c.P) for c in pm.TINY_CASES} == {(1, 2), (2, 2), (5, 8), (16, 16), (65, 64), (100, 64), (2000, 64)}
