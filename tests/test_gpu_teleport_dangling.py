"""The engine's teleport dangling mode (pr_set_teleport_dangling) on the GPU.

a. Exact bits on every path: tests/exact_dangling_model.py gives the one correct bit pattern of
   r' = t + damping * (S + (dc / ts) * t) on the three inputs with sinks of tests/exact_model.py, with
   8 seeds whose terms sum to ts = 8 (the hub -- a long row of the fused layout --, a sink and a source
   without in-links among them).  Ranks, dc and L1 after every iteration, dense and sparse setter,
   over fused, split, walk, narrow and class-loop epilogues and over row partitions.
b. The uniform bits are kept wherever the mode falls back.
c. Against the width-1 batch in PR_BATCH_DANGLING_TELEPORT, within the project's parity bound.
d. Plumbing: what the mode survives, ts, device bytes, split step calls, unreachable vertices.
e. Both CLIs: --seeds F --dangling=seeds.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_dangling_model as edm
import exact_model as em
from conftest import PKG_DIR
from test_gpu_exact import (ENGINE, ENGINE_IDS, PARTS, assert_bits, bits, check_dyadic, dyadic, engine_history,
                            group_history, open_engine, open_parts, parts_id)

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG_DIR, "build", "pagerank")
PARITY = 1e-9  # the project's parity bound (relative)
MODEL_ITERS = 5
MIN_EXACT = 3


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


# ---- inputs and their models, computed once --------------------------------------------------------
class Case:
    def __init__(self, name):
        self.d = dyadic(name)
        self.name, self.V, self.src, self.dst, self.inp = name, self.d.V, self.d.src, self.d.dst, self.d.inp
        self.ids, self.values, self.t = edm.seed_vector(self.d.g, self.inp.hub)
        self.init = self.d.init["grid"]
        self.run = edm.dangling_run(self.d.g, MODEL_ITERS, self.t, damping=0.5, init=self.init)
        self.n = min(self.run.exact_iters.values())
        # never shorter than this: a test that silently ran fewer iterations would hide failures
        assert self.n >= MIN_EXACT, (name, self.run.exact_iters)
        for a in (self.ids, self.values, self.t):
            a.setflags(write=False)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def open_one(hip, c, cfg, **kw):
    """One part of configuration cfg.  sinks5 goes through open_engine, which asserts that the named
    path is taken; the other two inputs (denser, or 1024 vertices) only have to build that way."""
    if c.name == "sinks5":
        return open_engine(hip, c, cfg, **kw)
    _, layout, opts, gather, reserve = cfg
    g = hip.PageRankGraph(c.V, c.src, c.dst, layout=layout, options=opts or None,
                          dangling=kw.get("dangling", "local"), keep_canonical=kw.get("keep_canonical", False))
    try:
        info = g.info()
        assert info["classes"] == (opts["classes"] if layout == "split" else 1)
        if layout == "split" and gather is not None:
            g.set_hot_gather(gather)
        if reserve is not None:
            g.set_hot_reserve(reserve)
    except BaseException:
        g.close()
        raise
    return g


def open_group(hip, c, pcase):
    if c.name == "sinks5":
        return open_parts(hip, c, pcase)
    P, layout, C, ag, pack, chunks = pcase
    opts = dict(exchange_allgather=ag, pack_fused=pack, xchg_chunks=chunks)
    if C is not None:
        opts["classes"] = C
    parts = []
    try:
        for p in range(P):
            parts.append(hip.PageRankGraph(c.V, c.src, c.dst, part=p, n_parts=P, keep_canonical=False, layout=layout,
                                           options=opts))
        assert sum(g.info()["local_rows"] for g in parts) == c.V
    except BaseException:
        for g in parts:
            g.close()
        raise
    return parts


def set_vector(target, c, how):
    if how == "dense":
        target.set_teleport(c.t)
    else:
        perm = np.random.default_rng(3).permutation(c.ids.size)  # the library sorts the seeds itself
        target.set_teleport_sparse(c.ids[perm], c.values[perm], rest=0.0)


# ---- a. exact bits on every path -------------------------------------------------------------------
A_ENGINE = [0, 1, 2, 4, 5, 6, 8]  # fused; split 8..128 classes; walk, narrow, class-loop (epi_walk = 0) epilogues


@pytest.mark.parametrize("cfg", [ENGINE[i] for i in A_ENGINE], ids=[ENGINE_IDS[i] for i in A_ENGINE])
@pytest.mark.parametrize("name", em.WITH_SINKS)
def test_engine_exact(hip, name, cfg):
    c = case(name)
    with open_one(hip, c, cfg) as g:
        info = g.info()
        assert info["n_sink"] == c.inp.n_sinks
        if cfg[1] == "fused" and c.inp.hub_in > em.FUSED_UNIT:
            assert info["n_long_rows"] == 1  # the hub, a seed: k_finalize's update carries q * t too
        g.set_teleport_dangling("teleport")
        for how in ("dense", "sparse"):
            set_vector(g, c, how)
            assert_bits(g.teleport_sum(), 8.0, (name, cfg[0], how, "ts"))
            got = engine_history(g, c.n, teleport=0.75, damping=0.5, init_ranks=c.init)
            check_dyadic(got, c.run, c.n, (name, cfg[0], how))
            assert (got[1] > 0).all()  # there is dangling mass to return
        # and the test can tell the modes apart
        g.set_teleport_dangling("uniform")
        r, _ = g.run(1, teleport=0.75, damping=0.5, init_ranks=c.init)
        assert r[c.inp.hub] != c.run.ranks[0][c.inp.hub]


A_PARTS = [0, 2, 4, 5, 9]  # P2-c16, P2-fused, P3-c8, P8-c64-chunks1, P9-c16


@pytest.mark.parametrize("pcase", [PARTS[i] for i in A_PARTS], ids=[parts_id(PARTS[i]) for i in A_PARTS])
@pytest.mark.parametrize("name", em.WITH_SINKS)
def test_parts_exact(hip, name, pcase):
    """Every part forms ts itself from the whole vector; every part reports the model's dc and L1."""
    c = case(name)
    P = pcase[0]
    parts = open_group(hip, c, pcase)
    try:
        grp = hip.PartGroup(parts)
        grp.set_teleport_dangling("teleport")
        for how in ("dense", "sparse"):
            set_vector(grp, c, how)
            for g in parts:
                assert g.teleport_dangling == "teleport"
                assert_bits(g.teleport_sum(), 8.0, (name, how, "ts of a part"))
            _, hist, dcs, l1s = group_history(hip, parts, c.n, teleport=0.75, damping=0.5, init_ranks=c.init)
            for it in range(c.n):
                assert_bits(hist[it], c.run.ranks[it], (name, how, "ranks after iteration", it + 1))
                assert_bits(dcs[it], np.full(P, c.run.dc[it]), (name, how, "dc of iteration", it + 1))
                assert_bits(l1s[it], np.full(P, c.run.l1[it]), (name, how, "l1 of iteration", it + 1))
    finally:
        for g in parts:
            g.close()


# ---- b. uniform bits kept --------------------------------------------------------------------------
B_ENGINE = [0, 1, 6]


def plain_run(g, n=4, **kw):
    hist, dc, l1 = engine_history(g, n, **kw)
    return np.concatenate([np.concatenate(hist), dc, l1])


@pytest.mark.parametrize("cfg", [ENGINE[i] for i in B_ENGINE], ids=[ENGINE_IDS[i] for i in B_ENGINE])
def test_fallbacks_keep_the_uniform_bits(hip, cfg):
    c = case("sinks5")
    rng = np.random.default_rng(17)
    init = rng.uniform(0.5, 1.5, c.V)
    t = rng.uniform(0.0, 0.3, c.V)
    a, b = int(c.ids[0]), int(c.ids[3])
    zero = np.zeros(c.V)
    zero[a], zero[b] = 1.0, -1.0
    huge = np.zeros(c.V)
    huge[a], huge[b] = 1e308, 1e308
    with open_one(hip, c, cfg) as g:
        scalar = plain_run(g, init_ranks=init)
        g.set_teleport(t)
        uniform = plain_run(g, init_ranks=init)
        assert not np.array_equal(bits(scalar), bits(uniform))
        # mode on, no vector: the scalar run
        g.set_teleport(None)
        g.set_teleport_dangling("teleport")
        assert g.teleport_sum() == 0.0
        assert_bits(plain_run(g, init_ranks=init), scalar, (cfg[0], "mode on, no vector"))
        # mode on, a vector: not the uniform run (the mode is live on this handle)
        g.set_teleport(t)
        assert not np.array_equal(bits(plain_run(g, init_ranks=init)), bits(uniform))
        # mode off after on: never on
        g.set_teleport_dangling("uniform")
        assert_bits(plain_run(g, init_ranks=init), uniform, (cfg[0], "mode off after on"))
        # ts exactly 0, ts = inf: the TELE uniform kernels
        for vec, what in ((zero, "ts = 0"), (huge, "ts = inf")):
            g.set_teleport_dangling("uniform")
            g.set_teleport(vec)
            want = plain_run(g, 2, init_ranks=init)
            g.set_teleport_dangling("teleport")
            ts = g.teleport_sum()
            assert ts == 0.0 if what == "ts = 0" else np.isinf(ts)
            assert_bits(plain_run(g, 2, init_ranks=init), want, (cfg[0], what))
    # a PR_DANGLING_NONE graph: dc is 0 and the mode changes nothing
    with open_one(hip, c, cfg, dangling="none") as g:
        g.set_teleport(t)
        want = plain_run(g, init_ranks=init)
        g.set_teleport_dangling("teleport")
        assert g.teleport_sum() > 0
        assert_bits(plain_run(g, init_ranks=init), want, (cfg[0], "dangling none"))


# ---- c. against the batch --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_graph():
    rng = np.random.default_rng(23)
    V, E = 3001, 24000
    src = rng.integers(0, 2600, E).astype(np.int32)  # vertices 2600.. are sinks
    dst = rng.integers(0, V, E).astype(np.int32)
    dst[:2500] = 11  # a hub: a long row of the fused layout
    src = np.concatenate([src, np.arange(2600, dtype=np.int32)])  # every source has a record
    dst = np.concatenate([dst, rng.integers(0, V, 2600).astype(np.int32)])
    ids = np.sort(rng.permutation(V)[:40]).astype(np.int32)
    ids[0] = 11
    ids = np.unique(ids)
    values = rng.uniform(0.01, 30.0, ids.size)
    return V, src, dst, ids, values


@pytest.mark.parametrize("layout,opts", [("fused", None), ("split", dict(classes=8))], ids=["fused", "c8"])
def test_engine_against_the_batch(hip, random_graph, layout, opts):
    from sparky_hip.batch import PageRankBatch

    V, src, dst, ids, values = random_graph
    with hip.PageRankGraph(V, src, dst, layout=layout, options=opts, keep_canonical=True) as g:
        assert g.info()["n_sink"] > 100
        with PageRankBatch(g, 1) as b:
            b.set_dangling("teleport")
            b.set_teleport_sparse(0, ids, values, rest=0.0)
            b.reset()
            b.step(10)
            want = b.ranks(0)
            want_ts = float(b.teleport_sums()[0])
        g.set_teleport_sparse(ids, values, rest=0.0)
        g.reset()
        g.step(10)
        uniform = g.ranks().copy()
        g.set_teleport_dangling("teleport")
        g.reset()
        g.step(10)
        got = g.ranks()
        ts = g.teleport_sum()
    err = np.max(np.abs(got - want) / np.abs(want))
    print(f"engine vs batch, {layout}: max relative error {err:.3e}, ts error {abs(ts - want_ts) / abs(want_ts):.3e}")
    assert (want > 0).all() and err <= PARITY
    assert abs(ts - want_ts) <= PARITY * abs(want_ts)
    assert np.max(np.abs(uniform - want) / np.abs(want)) > 1e-3  # the bound tells the modes apart


def test_engine_and_batch_agree_bitwise_on_the_exact_input(hip):
    """On the exact input every order gives the same bits, so the two routes agree bit for bit."""
    from sparky_hip.batch import PageRankBatch

    c = case("sinks5")
    with hip.PageRankGraph(c.V, c.src, c.dst) as g:
        with PageRankBatch(g, 1) as b:
            b.set_dangling("teleport")
            b.set_teleport(0, c.t)
            b.reset(teleport=0.75, damping=0.5, init_ranks=c.init)
            b.step(c.n)
            assert_bits(b.teleport_sums()[0], 8.0, "the batch's ts")
            assert_bits(b.ranks(0), c.run.ranks[c.n - 1], "the batch against the model")


# ---- d. plumbing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [ENGINE[0], ENGINE[1]], ids=[ENGINE_IDS[0], ENGINE_IDS[1]])
def test_mode_plumbing(hip, cfg):
    import sparky_hip._lib as L

    c = case("sinks5")
    last = c.run.ranks[c.n - 1]
    with open_one(hip, c, cfg) as g:
        assert g.teleport_dangling == "uniform" and g.teleport_sum() == 0.0
        bytes0 = g.info()["device_bytes"]
        g.set_teleport_dangling("teleport")  # before any vector, before reset
        assert g.teleport_dangling == "teleport" and g.info()["device_bytes"] == bytes0
        with pytest.raises(ValueError):
            g.set_teleport_dangling("seeds")
        assert L.load().pr_set_teleport_dangling(g._h, 5) == L.PR_ERR_INVALID
        mode = ctypes.c_int32(9)
        assert L.load().pr_get_teleport_dangling(g._h, None) == L.PR_ERR_INVALID
        assert L.load().pr_get_teleport_sum(g._h, None) == L.PR_ERR_INVALID
        assert L.load().pr_get_teleport_dangling(g._h, ctypes.byref(mode)) == 0 and mode.value == 1
        # ts follows every set
        g.set_teleport(np.full(c.V, 0.25))
        assert_bits(g.teleport_sum(), 0.25 * c.V, "ts of a constant vector")
        bytes1 = g.info()["device_bytes"]
        assert bytes1 > bytes0  # the vector itself
        g.set_teleport_sparse([5], [3.0], rest=0.0)
        assert_bits(g.teleport_sum(), 3.0, "ts of one seed")
        g.set_teleport(None)
        assert g.teleport_sum() == 0.0 and g.teleport_dangling == "teleport"
        # the mode survives clearing and re-setting the vector, run and reset
        set_vector(g, c, "dense")
        g.set_teleport_dangling("uniform")
        g.set_teleport_dangling("teleport")
        assert g.info()["device_bytes"] == bytes1
        ranks, _ = g.run(c.n, teleport=0.75, damping=0.5, init_ranks=c.init)
        assert_bits(ranks, last, (cfg[0], "run"))
        assert g.teleport_dangling == "teleport"
        g.reset(teleport=0.75, damping=0.5, init_ranks=c.init)
        g.step(c.n)
        assert_bits(g.ranks(), last, (cfg[0], "reset + step"))
        st = g.stats()
        assert_bits(st["last_dc"], c.run.dc[c.n - 1], "last_dc stays dc")
        assert_bits(st["last_l1"], c.run.l1[c.n - 1], "last_l1")
        assert g.teleport_dangling == "teleport" and g.teleport_sum() == 8.0
        # two step calls are one
        g.reset(teleport=0.75, damping=0.5, init_ranks=c.init)
        g.step(2)
        g.step(c.n - 2)
        assert_bits(g.ranks(), last, (cfg[0], "two step calls"))
        # the same on ordinary numbers: step(3); step(4) is step(7)
        rng = np.random.default_rng(29)
        g.set_teleport(rng.uniform(0.0, 0.3, c.V))
        init = rng.uniform(0.5, 1.5, c.V)
        g.reset(init_ranks=init)
        g.step(7)
        seven = g.ranks().copy()
        g.reset(init_ranks=init)
        g.step(3)
        g.step(4)
        assert_bits(g.ranks(), seven, (cfg[0], "step(3); step(4)"))
        # a switch takes effect from the next iteration enqueued
        g.reset(init_ranks=init)
        g.step(3)
        g.set_teleport_dangling("uniform")
        g.step(4)
        assert not np.array_equal(bits(g.ranks()), bits(seven))


def test_unreachable_vertices_drain(hip):
    """The component 5..9 cannot be reached from the seed 0.  In the mode it receives nothing, neither
    teleport nor dangling mass, so it evolves as if the rest of the graph did not exist: r' = 0.85 * S
    on its own edges (S = the old rank for vertex 9, which has no in-link).  From ranks of 0 it stays
    at exactly 0; from ranks of 1 every rank follows that closed recurrence bit for bit (no row has
    more than two in-links, so no sum has an order), vertex 9 holds exactly 0.85^k, and the component
    drains.  The uniform term feeds it in every iteration."""
    edges = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 4), (5, 6), (6, 7), (7, 5), (6, 8), (9, 5)]
    src = np.array([e[0] for e in edges], np.int32)
    dst = np.array([e[1] for e in edges], np.int32)
    far = np.arange(5, 10)
    with hip.PageRankGraph(10, src, dst) as g:
        g.set_teleport_sparse([0], [1.5], rest=0.0)
        for mode in ("teleport", "uniform"):
            g.set_teleport_dangling(mode)
            assert_bits(g.teleport_sum(), 1.5, "ts")
            hist, dc, _ = engine_history(g, 5, init_ranks=np.array([1.0] * 5 + [0.0] * 5))
            assert (dc > 0).all()  # the sinks 3 and 4 hold mass
            for it, r in enumerate(hist):
                if mode == "teleport":
                    assert np.array_equal(bits(r[far]), np.zeros(5, np.uint64)), (it, r[far])
                    assert (r[:5] > 0).all()
                else:
                    assert (r[far] > 0).all(), (it, r[far])
            hist, _, _ = engine_history(g, 12)  # from ranks of 1.0
            x = {v: np.float64(1.0) for v in far}
            d = np.float64(0.85)
            for it, r in enumerate(hist):
                if mode == "teleport":
                    S = {5: x[7] + x[9], 6: x[5], 7: x[6] / np.float64(2.0), 8: x[6] / np.float64(2.0), 9: x[9]}
                    x = {v: np.float64(0.0) + d * (S[v] + np.float64(0.0)) for v in far}
                    assert_bits(r[far], [x[v] for v in far], ("the closed recurrence, iteration", it + 1))
                else:
                    assert r[9] > 0.85 ** (it + 1)
            if mode == "teleport":
                assert (hist[-1][far] < 0.5).all() and hist[-1][far].sum() < 0.5 * hist[0][far].sum()


# ---- e. both CLIs ----------------------------------------------------------------------------------
def test_cli_dangling_seeds(hip, tmp_path):
    from sparky_hip import read_edge_list
    from sparky_hip._host import seed_teleport
    from sparky_hip.driver import java_double_to_string

    rng = np.random.default_rng(53)
    lines = [f"u{int(s)} u{int(d)}" for s, d in zip(rng.integers(0, 40, 300), rng.integers(0, 60, 300))]  # u40.. are sinks
    inp, fa = tmp_path / "edges.txt", tmp_path / "a.txt"
    inp.write_text("\n".join(lines) + "\n")
    fa.write_text("u3 2\nu7\n")
    urls, src, dst = read_edge_list(lines)
    index = {u: i for i, u in enumerate(urls)}
    ids, values = np.array([index["u3"], index["u7"]], np.int32), seed_teleport([2.0, 1.0], len(urls))
    want = {}
    with hip.PageRankGraph(len(urls), src, dst) as g:
        g.set_teleport_sparse(ids, values)
        for mode in ("teleport", "uniform"):
            g.set_teleport_dangling(mode)
            g.reset()
            g.step(8)
            assert g.stats()["last_dc"] > 0
            top_ids, top_ranks = g.topk(5)
            want[mode] = "".join(f"Starting iter{i}\n" for i in range(8)) + "".join(
                f"{urls[i]} has rank: {java_double_to_string(float(r))}.\n" for i, r in zip(top_ids, top_ranks))
            want[mode + "_ids"] = [urls[i] for i in top_ids]
    assert want["teleport"] != want["uniform"]
    args = [str(inp), "8", "--seeds", str(fa), "--top", "5"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    out = {}
    for runner, base in (("cpp", [CLI]), ("python", [sys.executable, "-m", "sparky_hip"])):
        res = subprocess.run(base + args + ["--dangling=seeds"], capture_output=True, env=env, timeout=120)
        assert res.returncode == 0, res.stderr
        out[runner] = res.stdout
    assert out["cpp"] == out["python"]  # identical bytes
    assert out["cpp"].decode() == want["teleport"]
    res = subprocess.run([CLI] + args, capture_output=True, env=env, timeout=120)
    assert res.returncode == 0 and res.stdout.decode() == want["uniform"]  # without the option: as before
    # two parts on one device list the same URLs (their sums take another order)
    for base in ([CLI], [sys.executable, "-m", "sparky_hip"]):
        res = subprocess.run(base + args + ["--dangling=seeds", "--devices", "0,0"], capture_output=True, env=env, timeout=120)
        assert res.returncode == 0, res.stderr
        listed = [l.split(" has rank: ")[0] for l in res.stdout.decode().splitlines() if " has rank: " in l]
        assert listed == want["teleport_ids"], (base, listed)
