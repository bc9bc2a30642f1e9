"""The row partition (pr_graph_create_part + pr_group_*) where the other GPU tests do not go: 9 to 64
parts, and parts that are tiny, empty or silent.

P > 8 (kMaxPackParts) switches off the fused pack (every iteration packs with k_pack), the piece
codes (a split part keeps 32-bit codes) and, once hot_slots < P, the hot set itself (Kp = 0).  Small
parts leave column classes and exchange chunks empty, parts of V < P own no row, and a pair of parts
may exchange nothing but its two slots {dangling partial, L1 partial}.  tests/partition_model.py
holds the cases and the model of what each part owns and exchanges; tests/
test_partition_model_cpu.py asserts that every input below reaches the edge it is named for.

Every test runs all parts in one process on device 0 through PartGroup: reset, step(3), step(4),
sync, ranks.  References: the oracle on its own CSR at the project's bar (RANK_TOL, BASELINE.json
north_star); the whole-slice all-gather of the same parts, bitwise; whole runs against chunked
runs, bitwise; PR_INFO_* counts against the model, exactly.
"""
import numpy as np
import pytest

import partition_model as pm
from test_gpu_teleport import Reference  # the iteration with a teleport vector, in numpy

pytestmark = pytest.mark.gpu

RANK_TOL = 1e-9  # north_star: "ranks within 1e-9 max relative error"
ITERS = 7  # step(3) + step(4)


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


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def layout_kw(lay, **opts):
    """PageRankGraph's layout and options for a partition_model layout; None values are left out."""
    _, layout, classes = lay
    o = {k: v for k, v in opts.items() if v is not None}
    if classes is not None:
        o["classes"] = classes
    return dict(layout=layout, options=o)


def open_parts(hip, V, src, dst, P, kw, dangling="local"):
    parts = []
    try:
        for p in range(P):
            parts.append(hip.PageRankGraph(V, src, dst, part=p, n_parts=P, keep_canonical=False, dangling=dangling,
                                           **kw))
    except BaseException:
        for g in parts:
            g.close()
        raise
    return parts


def iterate(grp, init=None):
    grp.reset(init_ranks=init)
    grp.step(3)
    grp.step(4)
    grp.sync()
    return grp.ranks()


def run_group(hip, V, src, dst, P, kw, dangling="local", init=None):
    """(ranks, every part's info, every part's dc of the last iteration)"""
    parts = open_parts(hip, V, src, dst, P, kw, dangling)
    try:
        infos = [g.info() for g in parts]
        r = iterate(hip.PartGroup(parts), init)
        dcs = [g.stats()["last_dc"] for g in parts]
        return r, infos, dcs
    finally:
        for g in parts:
            g.close()


class Model:
    """What the model says of one graph at one P."""

    def __init__(self, csr, P):
        self.csr, self.P = csr, P
        self.rows = pm.local_rows(csr, P)
        self.edges = pm.local_edges(csr, P)
        self.pair = pm.pair_counts(csr, P)
        self.send, self.recv = pm.sparse_volumes(self.pair)


def check_infos(infos, m, lay, xmode):
    """PR_INFO_* of every part against the model."""
    P, csr = m.P, m.csr
    assert [i["part"] for i in infos] == list(range(P)) and all(i["n_parts"] == P for i in infos)
    assert sum(i["local_rows"] for i in infos) == csr.n_vertices
    assert sum(i["local_edges"] for i in infos) == csr.n_edges
    assert [i["local_rows"] for i in infos] == m.rows.tolist()
    assert [i["local_edges"] for i in infos] == m.edges.tolist()
    if xmode == "sparse":
        assert [i["xchg_send"] for i in infos] == m.send.tolist()
        assert [i["xchg_recv"] for i in infos] == m.recv.tolist()
        assert sum(i["xchg_send"] for i in infos) == sum(i["xchg_recv"] for i in infos)
        for i in infos:
            if i["local_rows"] == 0:  # nothing to send or to read but the slots
                assert i["xchg_send"] == i["xchg_recv"] == 2 * (P - 1)
    else:
        assert all(i["xchg_recv"] == (P - 1) * i["xchg_send"] and i["xchg_send"] > 0 for i in infos)
    if lay[2] is None:
        assert all(i["layout"] == 0 and i["classes"] == 1 for i in infos)
    else:  # piece codes up to kMaxPackParts parts, 32-bit codes beyond
        bits_want = 20 if P <= pm.K_MAX_PACK_PARTS else 32
        assert all(i["layout"] == 1 and i["classes"] == lay[2] and i["code_bits"] == bits_want for i in infos)


def check_dc(dcs, ref, dangling="local"):
    """Every part sums all parts' dangling slots in part order: one value, the oracle's."""
    assert len(set(dcs)) == 1
    want = 0.0 if dangling == "none" else ref["dc"][ITERS - 1]
    assert abs(dcs[0] - want) <= RANK_TOL * max(abs(want), 1.0)


def both_exchanges(hip, oracle_c, V, src, dst, csr, ref, P, lay, dangling="local", init=None, **opts):
    """Sparse runs and whole slices: counts against the model, ranks and dc against the oracle, and
    the two bitwise equal.  Returns the sparse ranks."""
    m = Model(csr, P)
    out = {}
    for xmode in ("sparse", "allgather"):
        kw = layout_kw(lay, exchange_allgather=int(xmode == "allgather"), **opts)
        r, infos, dcs = run_group(hip, V, src, dst, P, kw, dangling, init)
        check_infos(infos, m, lay, xmode)
        assert not np.isnan(r).any()
        check_dc(dcs, ref, dangling)
        out[xmode] = (r, infos)
    assert np.array_equal(bits(out["sparse"][0]), bits(out["allgather"][0]))
    assert max_rel(out["sparse"][0], ref["ranks"]) <= RANK_TOL
    return out["sparse"]


# ---- 1. many parts ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(oracle_c):
    src, dst = pm.many_edges()
    csr = oracle_c.build_csr(pm.MANY_V, src, dst)
    ref = oracle_c.run(csr, ITERS)
    assert ref["dc"][ITERS - 1] > 0  # sinks on every part: the slots of all peers carry mass
    return pm.MANY_V, src, dst, csr, ref


def many_id(c):
    return f"P{c[0]}-{c[1][0]}" + ("" if c[2] is None else f"-hot{c[2]}")


@pytest.mark.parametrize("case", pm.MANY_CASES, ids=many_id)
def test_many_parts(hip, oracle_c, many, case):
    """P = 9 .. 64 on a graph of 20011 vertices with a hub row in pieces: k_pack every iteration,
    32-bit codes, the exchange lists and slots of up to 63 peers, and hot sets of Kp = hot_slots / P
    slots per part and class down to 1 and 0 (no hot set: k_hot_tables is not launched)."""
    P, lay, hot = case
    V, src, dst, csr, ref = many
    r, infos = both_exchanges(hip, oracle_c, V, src, dst, csr, ref, P, lay, hot_slots=hot)
    if hot is not None:
        assert all(i["hot_slots"] == P * pm.hot_kp(hot, P) for i in infos)


# ---- 2. the switch at 8 -> 9 parts -------------------------------------------------------------
def test_switch_between_8_and_9_parts(hip, oracle_c, many):
    """kMaxPackParts: 8 parts take the piece codes and the fused pack, 9 parts 32-bit codes and
    k_pack.  Both meet the oracle; at 8 the ranks are bitwise those of k_pack with 32-bit codes, and
    at 9 those two options change nothing."""
    V, src, dst, csr, ref = many
    plain = dict(pack_fused=0, codes=0)
    for P, want_bits in ((8, 20), (9, 32)):
        r, infos, dcs = run_group(hip, V, src, dst, P, layout_kw(pm.SPLIT16))
        assert all(i["code_bits"] == want_bits and i["classes"] == 16 for i in infos), P
        assert max_rel(r, ref["ranks"]) <= RANK_TOL, P
        check_dc(dcs, ref)
        r0, infos0, dcs0 = run_group(hip, V, src, dst, P, layout_kw(pm.SPLIT16, **plain))
        assert all(i["code_bits"] == 32 for i in infos0), P
        assert np.array_equal(bits(r), bits(r0)), P
        assert dcs == dcs0, P


# ---- 3. tiny and lopsided ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(oracle_c):
    out = {}
    for case in pm.TINY_CASES:
        src, dst = pm.tiny_edges(case)
        csr = oracle_c.build_csr(case.V, src, dst)
        out[case] = (src, dst, csr, oracle_c.run(csr, ITERS), oracle_c.run(csr, ITERS, dangling_none=True))
    return out


@pytest.mark.parametrize("lay", pm.TINY_LAYOUTS, ids=lambda lay: lay[0])
@pytest.mark.parametrize("case", pm.TINY_CASES, ids=lambda c: f"V{c.V}-P{c.P}")
def test_tiny_parts(hip, oracle_c, tiny, case, lay):
    """Parts of 0, 1, 2 or ~31 rows: parts that own no row (V < P), column classes and exchange
    chunks without a row, peer pairs whose run is the two slots alone."""
    src, dst, csr, ref, _ = tiny[case]
    both_exchanges(hip, oracle_c, case.V, src, dst, csr, ref, case.P, lay)


def test_tiny_parts_dangling_none(hip, oracle_c, tiny):
    case, lay = pm.TINY_NONE
    src, dst, csr, _, ref_none = tiny[case]
    both_exchanges(hip, oracle_c, case.V, src, dst, csr, ref_none, case.P, lay, dangling="none")


def test_tiny_parts_chunked_runs(hip, oracle_c, tiny):
    """64 parts of 31 or 32 rows with 64 classes, the overlapped exchange forced: the rows fill
    classes 0 .. 31, so chunks 4 .. 7 of every run are empty and the last one carries the slots
    alone.  Bitwise the whole runs, and the oracle's."""
    case, lay = pm.TINY_CHUNKED
    src, dst, csr, ref, _ = tiny[case]
    out = {}
    for chunks in (1, 0):
        r, infos, dcs = run_group(hip, case.V, src, dst, case.P, layout_kw(lay, xchg_chunks=chunks))
        check_infos(infos, Model(csr, case.P), lay, "sparse")
        check_dc(dcs, ref)
        out[chunks] = (r, dcs)
    assert np.array_equal(bits(out[1][0]), bits(out[0][0])) and out[1][1] == out[0][1]
    assert max_rel(out[1][0], ref["ranks"]) <= RANK_TOL


# ---- 4. silent peers -----------------------------------------------------------------------------
@pytest.mark.parametrize("lay", pm.SILENT_LAYOUTS, ids=lambda lay: lay[0])
@pytest.mark.parametrize("P", pm.SILENT_P)
@pytest.mark.parametrize("name", sorted(pm.SILENT_BUILDERS))
def test_silent_peers(hip, oracle_c, name, P, lay):
    """Graphs whose edges stay inside their owner (but for the 0 -> 1 run of one_way): every run is
    the two slots, k_pmask is skipped, k_sbase searches empty ranges, and the dangling sum -- one
    sink per part -- reaches every part through the slots alone."""
    V, src, dst = pm.SILENT_BUILDERS[name](P, pm.SILENT_ROWS, pm.SILENT_SINKS)
    csr = oracle_c.build_csr(V, src, dst)
    # distinct starting ranks: the parts are alike by construction, and with all ranks 1 their
    # dangling partials would be equal, so that one part's slots could pass for another's
    init = 0.5 + (0.37 * np.arange(V)) % 1.0
    ref = oracle_c.run(csr, ITERS, init=init)
    assert ref["dc"][ITERS - 1] > 0
    m = Model(csr, P)
    want = np.zeros((P, P), np.int64)
    if name == "one_way":
        want[0, 1] = pm.SILENT_ROWS - pm.SILENT_SINKS
    assert np.array_equal(m.pair, want)
    r, infos = both_exchanges(hip, oracle_c, V, src, dst, csr, ref, P, lay, init=init)
    for p, i in enumerate(infos):  # check_infos held them to the model; spelt out: the slots alone
        assert i["xchg_send"] == 2 * (P - 1) + (want[0, 1] if p == 0 else 0)
        assert i["xchg_recv"] == 2 * (P - 1) + (want[0, 1] if p == 1 else 0)
    if P <= pm.K_MAX_PACK_PARTS and lay[2] is not None:  # the fused pack against k_pack
        r0, infos0, dcs0 = run_group(hip, V, src, dst, P, layout_kw(lay, pack_fused=0), init=init)
        check_infos(infos0, m, lay, "sparse")
        check_dc(dcs0, ref)
        assert np.array_equal(bits(r), bits(r0))


# ---- 5. queries on many parts --------------------------------------------------------------------
def test_queries_on_16_parts(hip, oracle_c, many):
    """PartGroup.topk merges 16 lists; the sparse teleport form reaches every part's rows."""
    V, src, dst, csr, ref = many
    P = pm.QUERY_P
    rng = np.random.default_rng(5)
    seeds = rng.permutation(V)[:17].astype(np.int32)
    values = rng.random(17) * 40.0 + 0.01
    rest = 0.05
    dense = np.full(V, rest)
    dense[seeds] = values
    everyone = np.arange(V, dtype=np.int32)

    def check_topk(grp, full):
        for k in (1, 10, V + 5):
            o = np.lexsort((everyone, -full))[:k]
            ids, rk = grp.topk(k)
            assert len(ids) == len(rk) == min(k, V)
            assert np.array_equal(ids, everyone[o]) and np.array_equal(bits(rk), bits(full[o]))

    parts = open_parts(hip, V, src, dst, P, layout_kw(pm.SPLIT16))
    try:
        grp = hip.PartGroup(parts)
        r = iterate(grp).copy()
        assert max_rel(r, ref["ranks"]) <= RANK_TOL
        check_topk(grp, r)
        grp.set_teleport_sparse(seeds, values, rest)
        rs = iterate(grp).copy()
        check_topk(grp, rs)
        grp.set_teleport(dense)
        rd = iterate(grp).copy()
        assert np.array_equal(bits(rs), bits(rd))
        assert not np.isnan(rs).any()
        assert max_rel(rs, Reference(csr).run(dense, ITERS)) <= RANK_TOL
        grp.set_teleport(None)
        assert np.array_equal(bits(iterate(grp)), bits(r))
    finally:
        for g in parts:
            g.close()
