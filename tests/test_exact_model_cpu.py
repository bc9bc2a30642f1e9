"""tests/exact_model.py without a GPU: the model against the oracle, bit for bit, and the inputs
against the edges they exist for.

* Family D: dyadic_run equals oracle_c.run (ranks of every iteration, dc and L1 histories) as bits
  for exact_iters iterations on every builder -- the oracle's compensated sums are exact on these
  inputs too, so this is the model's independent check -- and equals a plain float64 restatement
  where the oracle has no say (a per-vertex teleport vector).
* Family S: iteration 1 equals the oracle on every row, iteration 2 on the masked rows.
* Every builder reaches its edge, proven from the oracle's CSR: degrees, sink counts, the hub's
  per-class segment lengths at 8 classes, piece counts >= 65, and exact_iters >= 8 without sinks,
  >= 3 with sinks.
* The model refuses inputs outside the family.
"""
import numpy as np
import pytest

import exact_model as em
import partition_model as pm


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def inputs(oracle_c):
    """name -> (input, Graph, oracle CSR), built once."""
    out = {}
    for name, build in em.DYADIC_BUILDERS.items():
        inp = build()
        out[name] = (inp, em.Graph(inp.V, inp.src, inp.dst), oracle_c.build_csr(inp.V, inp.src, inp.dst))
    return out


@pytest.fixture(scope="module")
def one_step(oracle_c):
    inp = em.one_step_graph()
    return inp, em.Graph(inp.V, inp.src, inp.dst), oracle_c.build_csr(inp.V, inp.src, inp.dst)


def assert_same_graph(g, csr, oc):
    assert np.array_equal(np.diff(csr.row_ptr), g.in_deg) and np.array_equal(csr.col_idx, g.cols)
    assert np.array_equal(csr.out_deg, g.out_deg)
    assert np.array_equal((csr.vflags & oc.VF_SINK) != 0, g.sink)
    assert np.array_equal((csr.vflags & oc.VF_NOLINK) != 0, g.nolink)
    assert np.array_equal((csr.vflags & oc.VF_INDEG0) != 0, ~g.has_in)


def want_iters(name):
    return em.MIN_ITERS_SINK_FREE if name in em.SINK_FREE else em.MIN_ITERS_SINKS


# ---- the inputs reach their edges -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(em.DYADIC_BUILDERS))
def test_dyadic_inputs(oracle_c, inputs, name):
    inp, g, csr = inputs[name]
    assert_same_graph(g, csr, oracle_c)
    sink = (csr.vflags & oracle_c.VF_SINK) != 0
    assert int(sink.sum()) == inp.n_sinks and (name in em.WITH_SINKS) == (inp.n_sinks > 0)
    assert set(np.unique(csr.out_deg[~sink]).tolist()) == {1, 2, 4} and not csr.out_deg[sink].any()
    assert len(inp.src) > csr.n_edges  # repeated records: the build has something to dedupe
    in_deg = np.diff(csr.row_ptr)
    assert in_deg[inp.hub] >= inp.hub_in and in_deg[inp.hub] == in_deg.max()
    assert int((in_deg == 0).sum()) >= inp.n_indeg0 > 0
    assert in_deg[sink].all()
    if inp.n_sinks:
        assert inp.V & (inp.V - 1) == 0 and 1 <= inp.n_sinks <= 5
    assert csr.n_edges < 1_000_000
    run = em.dyadic_run(g, 10)
    print(name, "V", inp.V, "E'", csr.n_edges, "hub in-degree", int(in_deg[inp.hub]), "rows without in-links",
          int((in_deg == 0).sum()), "exact_iters", run.exact_iters, "grid", run.grid_bits, "width", run.width_bits)
    assert min(run.exact_iters.values()) >= want_iters(name)
    assert all(w <= em.MANT for w in run.width_bits)


def hub_segments(csr, hub, C):
    """Lengths of the hub row's (row, class) segments at C classes of the one-part split layout: the
    class of a source is its index in the degree order modulo C, which is partition_model's owner."""
    cls = pm.owners(csr, C)
    return np.bincount(cls[csr.col_idx[csr.row_ptr[hub]:csr.row_ptr[hub + 1]]], minlength=C)


def test_small_and_hub9k_shapes(inputs):
    inp, _, csr = inputs["small"]
    assert inp.V == 4096 and np.diff(csr.row_ptr)[inp.hub] >= 3000
    inp, _, csr = inputs["hub9k"]
    in_deg = np.diff(csr.row_ptr)
    assert inp.V == 16384 and in_deg[inp.hub] >= 9000
    # fused: one row longer than a unit, and it takes the first lap of k_finalize only
    assert int((in_deg > em.FUSED_UNIT).sum()) == 1 and -(-int(in_deg[inp.hub]) // em.FUSED_UNIT) <= em.LAP
    # 8 classes: every class segment of the hub is cut into PIECE units, summed by k_seg_reduce
    seg = hub_segments(csr, inp.hub, 8)
    assert (seg > em.WAVE_UNIT).all() and (-(-seg // em.WAVE_UNIT) <= em.LAP).all()


def test_hub_fused_65_has_a_second_lap(inputs):
    inp, _, csr = inputs["hub_fused_65"]
    in_deg = np.diff(csr.row_ptr)
    assert in_deg[inp.hub] > em.LAP * em.FUSED_UNIT
    assert -(-int(in_deg[inp.hub]) // em.FUSED_UNIT) >= em.LAP + 1
    assert int((in_deg > em.FUSED_UNIT).sum()) == 1 and 140_000 <= inp.V <= 160_000


def test_hub_split_65_has_a_second_lap_in_every_class(inputs):
    inp, _, csr = inputs["hub_split_65"]
    seg = hub_segments(csr, inp.hub, 8)
    assert seg.sum() == np.diff(csr.row_ptr)[inp.hub] > 262_144
    assert (seg > em.LAP * em.WAVE_UNIT).all() and (-(-seg // em.WAVE_UNIT) >= em.LAP + 1).all()
    assert 290_000 <= inp.V <= 310_000


def test_one_step_input(oracle_c, one_step):
    inp, g, csr = one_step
    assert_same_graph(g, csr, oracle_c)
    assert inp.V == 20011 and inp.V % 64
    f = csr.vflags
    assert np.array_equal(np.nonzero(f & oracle_c.VF_SINK)[0], inp.sinks) and len(inp.sinks) == 2
    assert len(inp.src) > csr.n_edges + 1000  # duplicates
    rows = np.repeat(np.arange(inp.V), np.diff(csr.row_ptr))
    assert int((rows == csr.col_idx).sum()) >= 200  # self-loops
    assert 0.03 * inp.V <= int(((f & oracle_c.VF_NOLINK) != 0).sum()) <= 0.08 * inp.V
    in_deg = np.diff(csr.row_ptr)
    assert int((in_deg == 0).sum()) >= 500 and int((in_deg == 1).sum()) >= 2000
    assert in_deg[inp.hub] >= 2500 and len(np.unique(csr.out_deg)) >= 5
    # masked rows of iteration 2 whose single source lies in another part, at every P the GPU test uses
    one = np.nonzero(in_deg == 1)[0]
    for P in (2, 3, 8, 9):
        own = pm.owners(csr, P)
        assert int((own[csr.col_idx[csr.row_ptr[one]]] != own[one]).sum()) >= 500


# ---- the model against the oracle --------------------------------------------------------------------
def assert_model_is_oracle(oracle_c, g, csr, run, n, **kw):
    assert n >= 1 and run.exact_iters["ranks"] >= n and run.exact_iters["dc"] >= n
    ref = oracle_c.run(csr, n, keep_history=True, **kw)
    for it in range(n):
        diff = np.nonzero(bits(run.ranks[it]) != bits(ref["history"][it]))[0]
        assert diff.size == 0, ("ranks", it, diff.size, diff[:8].tolist())
    assert same_bits(run.dc[:n], ref["dc"]), "dc"
    n_l1 = min(n, run.exact_iters["l1"])
    assert n_l1 >= 1 and same_bits(run.l1[:n_l1], ref["l1"][:n_l1]), "l1"


@pytest.mark.parametrize("init", ["ones", "grid"])
@pytest.mark.parametrize("name", list(em.DYADIC_BUILDERS))
def test_dyadic_model_is_oracle(oracle_c, inputs, name, init):
    inp, g, csr = inputs[name]
    r0 = None if init == "ones" else em.grid_init(inp.V, 7)
    run = em.dyadic_run(g, 10, teleport=0.25, damping=0.5, init=r0)
    n = run.exact_iters["ranks"]
    if init == "ones":
        assert n >= want_iters(name)
    assert_model_is_oracle(oracle_c, g, csr, run, n, teleport=0.25, damping=0.5, init=r0)


@pytest.mark.parametrize("name", em.WITH_SINKS)
def test_dyadic_model_is_oracle_dangling_none(oracle_c, inputs, name):
    """dangling = "none": dc is 0, N need not be a power of two, and the grid grows as without sinks."""
    inp, g, csr = inputs[name]
    run = em.dyadic_run(g, 10, dangling="none")
    assert run.exact_iters["ranks"] >= em.MIN_ITERS_SINK_FREE and not run.dc.any()
    assert_model_is_oracle(oracle_c, g, csr, run, run.exact_iters["ranks"], teleport=0.25, damping=0.5,
                           dangling_none=True)


@pytest.mark.parametrize("name", ["small", "hub9k", "sinks3"])
def test_dyadic_model_is_float_restatement_with_a_vector(inputs, name):
    """A per-vertex teleport vector (the oracle takes a scalar only): the integer recurrence against
    the float64 restatement, whose sums are exact on these inputs in numpy's order as in any other."""
    inp, g, _ = inputs[name]
    t = em.grid_vector(inp.V, 9, hot=[inp.hub])
    r0 = em.grid_init(inp.V, 8) if name != "sinks3" else None
    run = em.dyadic_run(g, 10, teleport=t, init=r0)
    n = run.exact_iters["ranks"]
    assert n >= want_iters(name)
    ranks, dc, l1 = em.float_run(g, n, t, 0.5, init=r0)
    for it in range(n):
        assert same_bits(run.ranks[it], ranks[it]), it
    assert same_bits(run.dc, dc) and same_bits(run.l1[:run.exact_iters["l1"]], l1[:run.exact_iters["l1"]])


def test_mutations_change_the_bits(inputs):
    """What the inputs are for: the three arithmetic slips the 1e-9 bar hides each move bits of Family S's
    iteration 1 (fused multiply-add, dc / N folded into another term) or iteration 2 (reciprocal)."""
    inp = em.one_step_graph()
    g = em.Graph(inp.V, inp.src, inp.dst)
    r0, k = em.one_step_init(g, 5)
    m = em.one_step(g, k)
    S = np.ldexp(g.row_sums(np.where(g.out_deg > 0, k, 0)).astype(np.float64), -em.S_SHIFT)
    S[~g.has_in] = r0[~g.has_in]
    dc0 = m.dc[0]
    assert dc0 > 0
    reassoc = 0.15 + (0.85 * S + 0.85 * (dc0 / inp.V))
    assert np.mean(bits(reassoc) != bits(m.r1)) > 0.1
    import math

    fused = np.array([math.fma(0.85, s + dc0 / inp.V, 0.15) for s in S[:5000]]) if hasattr(math, "fma") else None
    if fused is not None:
        assert np.mean(bits(fused) != bits(m.r1[:5000])) > 0.1
    one = np.nonzero(g.in_deg == 1)[0]
    starts = np.concatenate([[0], np.cumsum(g.in_deg)])[:-1]
    u = g.cols[starts[one]]
    recip = 0.15 + 0.85 * (m.r1[u] * (1.0 / g.out_deg[u]) + m.dc[1] / inp.V)
    assert np.mean(bits(recip) != bits(m.r2[one])) > 0.05


# ---- Family S against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("dangling", ["local", "none"])
def test_one_step_is_oracle(oracle_c, one_step, dangling):
    inp, g, csr = one_step
    r0, k = em.one_step_init(g, 5)
    m = em.one_step(g, k, dangling=dangling)
    assert same_bits(m.r0, r0)
    # r0 / d is exactly k 2^-10
    d = np.maximum(csr.out_deg, 1).astype(np.float64)
    assert np.array_equal(np.ldexp(r0 / d, em.S_SHIFT), k.astype(np.float64))
    ref = oracle_c.run(csr, 2, init=r0, keep_history=True, dangling_none=dangling == "none")
    assert same_bits(m.r1, ref["history"][0])
    assert m.mask.sum() >= 2500 and np.array_equal(m.mask, np.diff(csr.row_ptr) <= 1)
    assert same_bits(m.r2[m.mask], ref["history"][1][m.mask])
    assert np.isnan(m.r2[~m.mask]).all()
    assert same_bits(m.dc, ref["dc"])
    assert (m.dc > 0).all() if dangling == "local" else not m.dc.any()


def test_one_step_mask_is_empty_with_many_sinks(inputs):
    inp, g, _ = inputs["sinks5"]
    _, k = em.one_step_init(g, 3)
    m = em.one_step(g, k)
    assert not m.mask.any() and np.isnan(m.dc[1]) and np.isfinite(m.r1).all()
    assert em.one_step(g, k, dangling="none").mask.any()


# ---- refusal -------------------------------------------------------------------------------------
def test_model_refuses_inputs_outside_the_family(inputs):
    inp, g, _ = inputs["small"]
    V = inp.V
    for kw in (dict(teleport=0.15), dict(damping=0.85), dict(damping=2.0), dict(teleport=-0.25),
               dict(teleport=np.full(V, 0.3)), dict(teleport=np.full(V - 1, 0.25)), dict(init=np.full(V, 1.0 / 32)),
               dict(init=np.full(V, np.nan)), dict(init=np.full(V, -1.0)), dict(dangling="teleport")):
        with pytest.raises(ValueError):
            em.dyadic_run(g, 2, **kw)
    # an out-degree of 3; a record without links
    tri = em.Graph(4, [0, 0, 0, 1, 2, 3], [1, 2, 3, 0, 0, 0])
    with pytest.raises(ValueError):
        em.dyadic_run(tri, 2)
    with pytest.raises(ValueError):
        em.dyadic_run(em.Graph(3, [0, 1, 2], [1, 0, -1]), 2)
    # sinks with N no power of two: refused when their mass is shared out, fine when it is not
    three = em.Graph(3, [0, 1], [2, 2])
    with pytest.raises(ValueError):
        em.dyadic_run(three, 2)
    assert em.dyadic_run(three, 2, dangling="none").exact_iters["ranks"] == 2
    # past 2^53 the model stops instead of returning rounded numbers
    _, g5, _ = inputs["sinks5"]
    run = em.dyadic_run(g5, 10)
    assert em.MIN_ITERS_SINKS <= run.exact_iters["ranks"] == len(run.ranks) < 10
    with pytest.raises(ValueError):
        em.one_step(g, np.zeros(V, np.int64))
