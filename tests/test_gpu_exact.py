"""Every iteration path against exact, order-free expected bits (tests/exact_model.py).

The inputs are chosen so that every sum of an iteration is exact in any order (Family D, several
iterations) or so that the first iteration is exact on every row and the second on the rows with at
most one in-link (Family S, the product's 0.15 / 0.85 on an arbitrary graph).  The expected bits
follow from the specification alone -- c = r / d a true division, t + damping * (S + dc / N) in four
separately rounded operations, S = r_old for rows without in-links -- and tests/
test_exact_model_cpu.py holds the model to the oracle bit for bit.  So every path must produce the
same bits: every layout, class count, code width, gather path, epilogue form, partition, exchange
mode, and the batch.  Ranks are compared after every iteration, and the dangling sum and the L1
delta of every iteration for which the model marks them exact.  Nothing here is compared within a
bound: every comparison is of uint64 views.
"""
import numpy as np
import pytest

import exact_model as em
import partition_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def assert_bits(got, want, what):
    """got == want as bits; on failure the message carries the number of differing entries."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.nonzero(bits(got) != bits(want))[0]
    assert diff.size == 0, (what, "differing entries", diff.size, "of", got.size, "first", diff[:6].tolist(),
                            got[diff[:3]].tolist(), want[diff[:3]].tolist())


# ---- inputs and their models, computed once -----------------------------------------------------------
class Dyadic:
    """One Family D input: the graph, and the model's runs by (teleport, init, dangling), cached."""

    def __init__(self, name):
        self.inp = em.DYADIC_BUILDERS[name]()
        self.name, self.V, self.src, self.dst = name, self.inp.V, self.inp.src, self.inp.dst
        self.g = em.Graph(self.V, self.src, self.dst)
        self.iters = em.MIN_ITERS_SINK_FREE if name in em.SINK_FREE else em.MIN_ITERS_SINKS
        self.init = {"ones": None, "grid": em.grid_init(self.V, 7)}
        self._runs = {}
        for a in (self.src, self.dst, self.init["grid"]):
            a.setflags(write=False)

    def vector(self, j):
        """Grid teleport vector number j (the hub's term is large, so its long row shows a lost term)."""
        t = em.grid_vector(self.V, 1000 + j, hot=[self.inp.hub])
        t.setflags(write=False)
        return t

    def model(self, teleport="scalar", init="ones", dangling="local", iters=None):
        """The model's run, never shorter than the iterations this input is there for: a test that
        silently ran fewer would hide failures."""
        n = self.iters if iters is None else iters
        key = (teleport, init, dangling, n)
        if key not in self._runs:
            t = 0.25 if teleport == "scalar" else self.vector(teleport)
            run = em.dyadic_run(self.g, n, teleport=t, damping=0.5, init=self.init[init], dangling=dangling)
            assert run.exact_iters["ranks"] >= n and run.exact_iters["dc"] >= n and run.exact_iters["l1"] >= n, (
                self.name, key, run.exact_iters)
            self._runs[key] = run
        return self._runs[key]


_dyadic = {}


def dyadic(name):
    if name not in _dyadic:
        _dyadic[name] = Dyadic(name)
    return _dyadic[name]


class OneStep:
    def __init__(self):
        self.inp = em.one_step_graph()
        self.V, self.src, self.dst = self.inp.V, self.inp.src, self.inp.dst
        self.g = em.Graph(self.V, self.src, self.dst)
        self.r0, self.k = em.one_step_init(self.g, 5)
        self.tvec = np.random.default_rng(6).uniform(0.0, 0.4, self.V)  # any float64 will do in Family S
        self._m = {}
        for a in (self.src, self.dst, self.r0, self.tvec):
            a.setflags(write=False)

    def model(self, dangling="local", vector=False):
        key = (dangling, vector)
        if key not in self._m:
            m = em.one_step(self.g, self.k, teleport=self.tvec if vector else 0.15, dangling=dangling)
            assert m.mask.sum() >= 2500
            self._m[key] = m
        return self._m[key]


_one = []


def one_step():
    if not _one:
        _one.append(OneStep())
    return _one[0]


# ---- running the engine ---------------------------------------------------------------------------
def engine_history(g, n, **kw):
    """n iterations through pr_run: (ranks after every iteration, dc of every iteration, L1 of every
    iteration)."""
    hist = []
    ranks, stats = g.run(n, want_ranks_in_callback=True, callback=lambda it, r, st: hist.append(r), **kw)
    assert len(hist) == len(stats) == n and np.array_equal(bits(ranks), bits(hist[-1]))
    return hist, np.array([s.dangling_sum for s in stats]), np.array([s.l1_delta for s in stats])


def check_dyadic(got, run, n, what):
    hist, dc, l1 = got
    for it in range(n):
        assert_bits(hist[it], run.ranks[it], (what, "ranks after iteration", it + 1))
    assert_bits(dc, run.dc[:n], (what, "dangling_sum"))
    assert_bits(l1, run.l1[:n], (what, "l1_delta"))


def check_one_step(hist, dc, m, what):
    assert_bits(hist[0], m.r1, (what, "ranks after iteration 1"))
    assert_bits(hist[1][m.mask], m.r2[m.mask], (what, "rows with at most one in-link after iteration 2"))
    assert_bits(dc, m.dc, (what, "dangling_sum"))


# One part: (id, layout, build options, hot_gather or None, hot_reserve or None).  Every value the
# engine's options take occurs: classes 8 / 16 / 32 / 64 / 128, hot_slots 0 / 37 / default, codes
# default / 32-bit, both gather paths, epi_walk 0 / 1, epi_narrow 0 / 1, epi_order 0 / 1 / 2, reserved CUs.
ENGINE = [
    ("fused", "fused", {}, None, None),
    ("c8", "split", dict(classes=8), None, None),
    ("c8-narrow0-walk1-order0-dense-reserve1", "split", dict(classes=8, epi_narrow=0, epi_walk=1, epi_order=0), 1, 1),
    ("c16-slots0-codes32-dense", "split", dict(classes=16, hot_slots=0, codes=0), 1, None),
    ("c16-slots37-codes32-narrow1-walk0", "split", dict(classes=16, hot_slots=37, codes=0, epi_narrow=1, epi_walk=0),
     0, None),
    ("c32-slots37-walk0-perpos", "split", dict(classes=32, hot_slots=37, epi_walk=0), 0, None),
    ("c64-narrow1-order1", "split", dict(classes=64, epi_narrow=1, epi_order=1), None, None),
    ("c64-slots0-narrow0-order2-dense", "split", dict(classes=64, hot_slots=0, epi_narrow=0, epi_order=2), 1, None),
    ("c128-order2", "split", dict(classes=128, epi_order=2), None, None),
]
ENGINE_IDS = [c[0] for c in ENGINE]


def open_engine(hip, inp, cfg, dangling="local", keep_canonical=False):
    """The graph of one ENGINE configuration, with info() asserting that the named path is taken."""
    _, layout, opts, gather, reserve = cfg
    g = hip.PageRankGraph(inp.V, inp.src, inp.dst, layout=layout, options=opts or None, dangling=dangling,
                          keep_canonical=keep_canonical)
    try:
        info = g.info()
        assert info["n_parts"] == 1 and info["n_vertices"] == inp.V
        if layout == "fused":
            assert info["layout"] == 0 and info["classes"] == 1 and info["epilogue"] == 0
        else:
            C = opts["classes"]
            assert info["layout"] == 1 and info["classes"] == C and info["epilogue"] == 3
            slots = opts.get("hot_slots", -1)
            assert info["hot_slots"] == slots if slots >= 0 else info["hot_slots"] > 37
            assert info["code_bits"] == (32 if opts.get("codes", -1) == 0 else 20)
            if opts.get("epi_walk", 1) == 0 or C > 64:
                assert info["walk_groups"] == 0
            else:
                assert info["walk_groups"] > 0
            if gather is not None:
                g.set_hot_gather(gather)
                assert g.info()["hot_gather"] == gather
            else:
                assert info["hot_gather"] == 0  # the size rule: per-position gathers at these sizes
        if reserve is not None:
            g.set_hot_reserve(reserve)
    except BaseException:
        g.close()
        raise
    return g


@pytest.mark.parametrize("cfg", ENGINE, ids=ENGINE_IDS)
@pytest.mark.parametrize("name,init", [("small", "ones"), ("hub9k", "grid"), ("sinks5", "ones")])
def test_engine_dyadic(hip, name, init, cfg):
    """Family D through pr_run with teleport = 0.25 and damping = 0.5: 8 iterations without sinks, 3
    with five sinks (dc / N a shift), ranks of every iteration, dc and L1 as bits."""
    d = dyadic(name)
    run = d.model(init=init)
    with open_engine(hip, d, cfg) as g:
        info = g.info()
        assert info["n_sink"] == d.inp.n_sinks and info["max_indeg"] >= d.inp.hub_in
        if name == "hub9k":  # the hub: one long row (fused), a long segment in every class (8 classes)
            if cfg[1] == "fused":
                assert info["n_long_rows"] == 1
            elif cfg[2]["classes"] == 8:
                assert info["n_long_rows"] >= 8
        got = engine_history(g, d.iters, teleport=0.25, damping=0.5, init_ranks=d.init[init])
    check_dyadic(got, run, d.iters, (name, cfg[0]))


@pytest.mark.parametrize("cfg", ENGINE, ids=ENGINE_IDS)
def test_engine_one_step(hip, cfg):
    """Family S with the product's 0.15 / 0.85: iteration 1 on every row of a ragged graph with
    duplicates, self-loops, records without links and two sinks; iteration 2 on the rows that read a
    single c' (the true division of whichever site wrote it) or their own old rank."""
    s = one_step()
    m = s.model()
    with open_engine(hip, s, cfg) as g:
        info = g.info()
        assert info["n_sink"] == 2 and info["n_nolink"] > 0 and info["n_indeg0"] > 0
        hist, dc, _ = engine_history(g, 2, init_ranks=s.r0)
    check_one_step(hist, dc, m, cfg[0])


@pytest.mark.parametrize("cfg", [ENGINE[0], ENGINE[1], ENGINE[6]], ids=[ENGINE_IDS[i] for i in (0, 1, 6)])
def test_engine_dangling_none(hip, cfg):
    """dangling = "none": dc is exactly 0 in both families, and Family D's grid grows as without sinks."""
    d = dyadic("sinks5")
    run = d.model(dangling="none", iters=em.MIN_ITERS_SINK_FREE)
    with open_engine(hip, d, cfg, dangling="none") as g:
        got = engine_history(g, em.MIN_ITERS_SINK_FREE, teleport=0.25, damping=0.5)
    assert not got[1].any()
    check_dyadic(got, run, em.MIN_ITERS_SINK_FREE, ("sinks5-none", cfg[0]))
    s = one_step()
    with open_engine(hip, s, cfg, dangling="none") as g:
        hist, dc, _ = engine_history(g, 2, init_ranks=s.r0)
    check_one_step(hist, dc, s.model(dangling="none"), ("none", cfg[0]))


def test_finalize_second_lap_fused(hip):
    """hub_fused_65: a row of more than 64 * 2048 in-links is 65 or more pieces in the fused layout, so
    k_finalize's piece loop takes a second lap."""
    d = dyadic("hub_fused_65")
    with open_engine(hip, d, ENGINE[0]) as g:
        info = g.info()
        assert info["n_long_rows"] == 1 and info["max_indeg"] > em.LAP * em.FUSED_UNIT
        got = engine_history(g, d.iters, teleport=0.25, damping=0.5)
    check_dyadic(got, d.model(), d.iters, "hub_fused_65")


def test_seg_reduce_second_lap_split8(hip):
    """hub_split_65: at 8 classes every class segment of the hub has more than 64 * 512 entries, so
    k_seg_reduce's piece loop takes a second lap in all eight."""
    d = dyadic("hub_split_65")
    with open_engine(hip, d, ENGINE[1]) as g:
        info = g.info()
        assert info["n_long_rows"] >= 8 and info["max_indeg"] > 8 * em.LAP * em.WAVE_UNIT
        got = engine_history(g, d.iters, teleport=0.25, damping=0.5)
    check_dyadic(got, d.model(), d.iters, "hub_split_65")


# ---- teleport vector ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["dense", "sparse"])
@pytest.mark.parametrize("cfg", [ENGINE[0], ENGINE[1], ENGINE[6], ENGINE[8]], ids=[ENGINE_IDS[i] for i in (0, 1, 6, 8)])
def test_teleport_vector(hip, cfg, how):
    """A per-vertex teleport vector on the grid through pr_set_teleport and pr_set_teleport_sparse, on
    hub9k: in the fused layout the hub is a long row, updated by k_finalize<TELE>; the scalar passed
    beside the vector is ignored."""
    d = dyadic("hub9k")
    if how == "dense":
        tkey = 1
        t = d.vector(tkey)
    else:  # 2000 seeds with grid terms, every other vertex 0.25
        tkey = "sparse"
        ids = np.sort(np.random.default_rng(31).permutation(d.V)[:2000]).astype(np.int32)
        if d.inp.hub not in ids:
            ids[0] = d.inp.hub
            ids = np.sort(ids)
        t = np.full(d.V, 0.25)
        t[ids] = d.vector(2)[ids]
    run = em.dyadic_run(d.g, d.iters, teleport=t, damping=0.5, init=d.init["grid"])
    assert min(run.exact_iters.values()) >= d.iters
    with open_engine(hip, d, cfg) as g:
        if cfg[1] == "fused":
            assert g.info()["n_long_rows"] == 1
        if how == "dense":
            g.set_teleport(t)
        else:
            g.set_teleport_sparse(ids, t[ids], rest=0.25)
        got = engine_history(g, d.iters, teleport=0.75, damping=0.5, init_ranks=d.init["grid"])
        check_dyadic(got, run, d.iters, (cfg[0], how))
        g.set_teleport(None)  # back to the scalar
        got = engine_history(g, d.iters, teleport=0.25, damping=0.5, init_ranks=d.init["grid"])
        check_dyadic(got, d.model(init="grid"), d.iters, (cfg[0], how, "scalar again"))
    s = one_step()
    with open_engine(hip, s, cfg) as g:
        g.set_teleport(s.tvec)
        hist, dc, _ = engine_history(g, 2, init_ranks=s.r0)
    check_one_step(hist, dc, s.model(vector=True), (cfg[0], "one step, vector"))


# ---- scalars through every entry point, resume ----------------------------------------------------------
@pytest.mark.parametrize("cfg", [ENGINE[0], ENGINE[2], ENGINE[8]], ids=[ENGINE_IDS[i] for i in (0, 2, 8)])
@pytest.mark.parametrize("name", ["hub9k", "sinks5"])
def test_reset_and_step_take_the_scalars(hip, name, cfg):
    """teleport = 0.25 and damping = 0.5 through pr_reset + pr_step (3 then 5 iterations; 1 then 2 with
    sinks): the ranks and the statistics of the last iteration."""
    d = dyadic(name)
    run = d.model()
    a = 3 if d.iters == 8 else 1
    with open_engine(hip, d, cfg) as g:
        g.reset(teleport=0.25, damping=0.5)
        g.step(a)
        g.sync()
        assert_bits(g.ranks(), run.ranks[a - 1], (name, cfg[0], "after the first step call"))
        g.step(d.iters - a)
        g.sync()
        assert_bits(g.ranks(), run.ranks[d.iters - 1], (name, cfg[0], "after the second step call"))
        st = g.stats()
        assert st["iters"] == d.iters
        assert_bits(st["last_dc"], run.dc[d.iters - 1], (name, cfg[0], "last_dc"))
        assert_bits(st["last_l1"], run.l1[d.iters - 1], (name, cfg[0], "last_l1"))


@pytest.mark.parametrize("cfg", [ENGINE[0], ENGINE[1]], ids=[ENGINE_IDS[i] for i in (0, 1)])
def test_resume(hip, cfg):
    """run(4), then run(4, init_ranks = those ranks): the model's iteration 8."""
    d = dyadic("hub9k")
    run = d.model(init="grid")
    with open_engine(hip, d, cfg) as g:
        r4, _ = g.run(4, teleport=0.25, damping=0.5, init_ranks=d.init["grid"])
        assert_bits(r4, run.ranks[3], (cfg[0], "iteration 4"))
        got = engine_history(g, 4, teleport=0.25, damping=0.5, init_ranks=r4)
    for it in range(4):
        assert_bits(got[0][it], run.ranks[4 + it], (cfg[0], "resumed, iteration", 5 + it))
    assert_bits(got[1], run.dc[4:8], "dc")
    assert_bits(got[2], run.l1[4:8], "l1")


# ---- row partition, group path on one GPU -----------------------------------------------------------------
# (P, layout, classes, exchange_allgather, pack_fused, xchg_chunks)
PARTS = [
    (2, "split", 16, 0, 1, 0),
    (2, "split", 64, 1, 1, 0),
    (2, "fused", None, 0, 1, 0),
    (3, "split", 64, 0, 1, 1),
    (3, "split", 8, 0, 0, 0),
    (8, "split", 64, 0, 0, 1),
    (8, "split", 8, 0, 1, 0),
    (8, "split", 64, 1, 1, 0),
    (8, "split", 64, 0, 1, 0),
    (9, "split", 16, 0, 1, 0),  # more than kMaxPackParts parts: 32-bit codes and k_pack
]


def parts_id(c):
    P, layout, C, ag, pack, chunks = c
    return f"P{P}-{'fused' if C is None else 'c%d' % C}-{'allgather' if ag else 'runs'}-pack{pack}-chunks{chunks}"


def open_parts(hip, inp, case, dangling="local"):
    P, layout, C, ag, pack, chunks = case
    opts = dict(exchange_allgather=ag, pack_fused=pack, xchg_chunks=chunks)
    if C is not None:
        opts["classes"] = C
    parts = []
    try:
        for p in range(P):
            parts.append(hip.PageRankGraph(inp.V, inp.src, inp.dst, part=p, n_parts=P, keep_canonical=False,
                                           layout=layout, options=opts, dangling=dangling))
        infos = [g.info() for g in parts]
        assert [i["part"] for i in infos] == list(range(P)) and all(i["n_parts"] == P for i in infos)
        assert sum(i["local_rows"] for i in infos) == inp.V
        if C is None:
            assert all(i["layout"] == 0 and i["classes"] == 1 for i in infos)
        else:  # piece codes up to kMaxPackParts parts, 32-bit codes beyond
            want = 20 if P <= pm.K_MAX_PACK_PARTS else 32
            assert all(i["layout"] == 1 and i["classes"] == C and i["code_bits"] == want for i in infos)
        if ag:
            assert all(i["xchg_recv"] == (P - 1) * i["xchg_send"] and i["xchg_send"] > 0 for i in infos)
        else:
            assert sum(i["xchg_send"] for i in infos) == sum(i["xchg_recv"] for i in infos)
            assert all(i["xchg_send"] > 2 * (P - 1) for i in infos)  # contributions cross, not only the slots
    except BaseException:
        for g in parts:
            g.close()
        raise
    return parts


def group_history(hip, parts, n, **kw):
    """n iterations of a group, one pr_group_step each: ranks, and every part's dc and L1."""
    grp = hip.PartGroup(parts)
    grp.reset(**kw)
    hist, dcs, l1s = [], [], []
    for _ in range(n):
        grp.step(1)
        grp.sync()
        hist.append(grp.ranks())
        st = [p.stats() for p in parts]
        dcs.append([s["last_dc"] for s in st])
        l1s.append([s["last_l1"] for s in st])
    return grp, hist, np.array(dcs), np.array(l1s)


@pytest.mark.parametrize("case", PARTS, ids=parts_id)
def test_parts_dyadic(hip, case):
    """Family D through pr_group_reset(teleport = 0.25, damping = 0.5) + pr_group_step: 8 iterations on
    hub9k from grid ranks, 3 on the five-sink graph (every part adds all parts' dangling slots).
    Every part reports the model's dc and L1; two step calls (3 + 5) reach the same bits."""
    P = case[0]
    for name, init in (("hub9k", "grid"), ("sinks5", "ones")):
        d = dyadic(name)
        run = d.model(init=init)
        parts = open_parts(hip, d, case)
        try:
            grp, hist, dcs, l1s = group_history(hip, parts, d.iters, teleport=0.25, damping=0.5,
                                                init_ranks=d.init[init])
            for it in range(d.iters):
                assert_bits(hist[it], run.ranks[it], (name, "ranks after iteration", it + 1))
                assert_bits(dcs[it], np.full(P, run.dc[it]), (name, "dc of iteration", it + 1))
                assert_bits(l1s[it], np.full(P, run.l1[it]), (name, "l1 of iteration", it + 1))
            a = 3 if d.iters == 8 else 1
            grp.reset(teleport=0.25, damping=0.5, init_ranks=d.init[init])
            grp.step(a)
            grp.step(d.iters - a)
            grp.sync()
            assert_bits(grp.ranks(), run.ranks[d.iters - 1], (name, "two step calls"))
        finally:
            for g in parts:
                g.close()


@pytest.mark.parametrize("case", PARTS, ids=parts_id)
def test_parts_one_step(hip, case):
    """Family S for two iterations: the masked rows of iteration 2 read c' values that crossed the
    exchange (tests/test_exact_model_cpu.py counts those whose single source another part owns)."""
    s = one_step()
    m = s.model()
    parts = open_parts(hip, s, case)
    try:
        _, hist, dcs, _ = group_history(hip, parts, 2, init_ranks=s.r0)
    finally:
        for g in parts:
            g.close()
    assert_bits(hist[0], m.r1, "ranks after iteration 1")
    assert_bits(hist[1][m.mask], m.r2[m.mask], "rows with at most one in-link after iteration 2")
    for it in range(2):
        assert_bits(dcs[it], np.full(case[0], m.dc[it]), ("dc of iteration", it + 1))


# ---- the batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 16])
@pytest.mark.parametrize("name", ["small", "hub9k", "sinks5"])
def test_batch(hip, name, width):
    """PageRankBatch, uniform dangling mode, reset(teleport = 0.25, damping = 0.5): every column has a
    grid teleport vector of its own (dense or sparse), column 1 keeps the scalar; ranks(j) after every
    iteration and norms() equal the model's run with that vector.  Then the engine with one column's
    vector equals that column bit for bit -- a statement no ordinary input allows."""
    from sparky_hip.batch import PageRankBatch

    d = dyadic(name)
    keys = ["scalar" if j == 1 else 100 + j for j in range(width)]
    init = "grid" if name in em.SINK_FREE else "ones"  # with sinks the grid grows 13 bits an iteration
    runs = [d.model(teleport=k, init=init) for k in keys]
    with hip.PageRankGraph(d.V, d.src, d.dst) as g:
        with PageRankBatch(g, width) as b:
            assert b.dangling == "uniform" and b.info()["width"] == width
            assert b.info()["n_long_rows"] >= 1  # the hub, in chunks
            for j, k in enumerate(keys):
                if k == "scalar":
                    continue
                t = d.vector(k)
                if j % 2 == 0:
                    b.set_teleport(j, t)
                else:  # sparse: the non-zero terms as seeds, the rest 0
                    ids = np.nonzero(t)[0].astype(np.int32)
                    b.set_teleport_sparse(j, ids, t[ids], rest=0.0)
            b.reset(teleport=0.25, damping=0.5, init_ranks=d.init[init])
            last = None
            for it in range(d.iters):
                b.step(1)
                b.sync()
                dc, l1 = b.norms()
                assert_bits(dc, [r.dc[it] for r in runs], (name, "dc of iteration", it + 1))
                assert_bits(l1, [r.l1[it] for r in runs], (name, "l1 of iteration", it + 1))
                last = [b.ranks(j) for j in range(width)]
                for j in range(width):
                    assert_bits(last[j], runs[j].ranks[it], (name, "column", j, "iteration", it + 1))
        j = width - 1
        g.set_teleport(d.vector(keys[j]))
        ranks, _ = g.run(d.iters, teleport=0.25, damping=0.5, init_ranks=d.init[init])
        assert_bits(ranks, last[j], (name, "the engine against column", j))
