"""The graph generators and the device interner (csrc/pr_gen.hip) against the plain model in
tests/gen_model.py, bit for bit.

Every number the project quotes is measured on a graph these kernels make, and the rest of the suite
compares what is built from their edges with the oracle on the same edges: a generator that emits
the wrong graph passes all of it.  Here the edges themselves are compared with a model written from
the definition (gen_model's docstring; tests/test_gen_model_cpu.py checks the model against it).

The one floating-point step, the Chung-Lu power law, is compared bitwise outside the ambiguity band
gen_model derives; inside it the device's rank may be the model's +-1 and nothing else.  The test
prints how many draws differed: a measurement of the device pow, not a tolerance.
"""
import ctypes
import inspect

import numpy as np
import pytest

import gen_model as gm

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -1515870811  # 0xA5A5A5A5: neither a label nor the -1 of a link-less record
PR_ERR_INVALID = -1
GRID_LIMIT = 65536 * 256  # pr_gen.hip: grid_for(n, 256, 65536); past it a thread takes a second edge


@pytest.fixture(scope="module")
def hip():
    import sparky_hip
    import sparky_hip.workloads  # noqa: F401  (hip.workloads: the bench's seeds)

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


class DevPair:
    """Two int32 device arrays of n elements plus GUARD guard elements, pre-filled."""

    def __init__(self, torch, n, src=None, dst=None):
        self.torch, self.n = torch, n
        self.s = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.d = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        if src is not None:
            self.s[:n] = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
            self.d[:n] = torch.from_numpy(np.ascontiguousarray(dst, np.int32)).cuda()
        torch.cuda.synchronize()

    def ptrs(self):
        return self.s.data_ptr(), self.d.data_ptr()

    def fetch(self):
        """(src, dst) of the n elements, after asserting that the guards are untouched."""
        self.torch.cuda.synchronize()
        s, d = self.s.cpu().numpy(), self.d.cpu().numpy()
        assert np.all(s[self.n:] == SENTINEL) and np.all(d[self.n:] == SENTINEL), "guard elements overwritten"
        return s[:self.n], d[:self.n]

    def assert_untouched(self):
        s, d = self.fetch()
        assert np.all(s == SENTINEL) and np.all(d == SENTINEL)


RMAT_DEFAULT = (0.57, 0.19, 0.19)


def run_rmat(hip, torch, scale, E, abc=RMAT_DEFAULT, seed=1):
    p = DevPair(torch, E)
    hip.gen_rmat(0, scale, E, *p.ptrs(), a=abc[0], b=abc[1], c=abc[2], seed=seed)
    return p.fetch()


def run_er(hip, torch, scale, E, seed=3):
    p = DevPair(torch, E)
    hip.gen_er(0, scale, E, *p.ptrs(), seed=seed)
    return p.fetch()


def assert_edges_equal(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), f"src: first difference at {int(np.argmax(got[0] != want[0]))}"
    assert np.array_equal(got[1], want[1]), f"dst: first difference at {int(np.argmax(got[1] != want[1]))}"


# ---- generators, bitwise --------------------------------------------------------------------------------

E_ODD = 70_001  # not a multiple of the 256-thread workgroup


def test_wrapper_defaults_are_graph500(hip):
    sig = inspect.signature(hip.gen_rmat).parameters
    assert (sig["a"].default, sig["b"].default, sig["c"].default) == RMAT_DEFAULT


@pytest.mark.parametrize("scale", [1, 2, 5, 16, 31])  # 5: odd, the top level has no partner; 31: labels to 2^31-1
def test_rmat_scales(hip, torch, scale):
    want = gm.rmat(scale, E_ODD, *RMAT_DEFAULT, 1)
    assert_edges_equal(run_rmat(hip, torch, scale, E_ODD), want)
    if scale == 31:
        assert int(max(want[0].max(), want[1].max())) >= 1 << 30 and min(want[0].min(), want[1].min()) >= 0


@pytest.mark.parametrize("abc", [(0.45, 0.30, 0.10), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.25, 0.25)])
def test_rmat_probabilities(hip, torch, abc):
    assert_edges_equal(run_rmat(hip, torch, 16, E_ODD, abc=abc), gm.rmat(16, E_ODD, *abc, 1))


@pytest.mark.parametrize("seed", [2, 0, (1 << 63) + 12345])  # the last: the u64 passes through ctypes whole
def test_rmat_seeds(hip, torch, seed):
    assert_edges_equal(run_rmat(hip, torch, 16, E_ODD, seed=seed), gm.rmat(16, E_ODD, *RMAT_DEFAULT, seed))


@pytest.mark.parametrize("scale", [1, 13, 24, 31])
def test_er_scales(hip, torch, scale):
    assert_edges_equal(run_er(hip, torch, scale, E_ODD), gm.er(scale, E_ODD, 3))


@pytest.mark.parametrize("seed", [0, (1 << 63) + 12345])
def test_er_seeds(hip, torch, seed):
    assert_edges_equal(run_er(hip, torch, 13, E_ODD, seed=seed), gm.er(13, E_ODD, seed))


@pytest.mark.parametrize("gen", ["rmat", "er"])
def test_grid_stride_branch(hip, torch, gen):
    """E > 65536 * 256: the grid is capped and the kernels' loops take a second trip, which otherwise
    only the headline workloads reach.  Whole arrays."""
    E = GRID_LIMIT + 777
    if gen == "rmat":
        assert_edges_equal(run_rmat(hip, torch, 2, E), gm.rmat(2, E, *RMAT_DEFAULT, 1))
    else:
        assert_edges_equal(run_er(hip, torch, 24, E), gm.er(24, E, 3))


def test_edge_does_not_depend_on_edge_count(hip, torch):
    for scale in (16, 5):
        short, long_ = run_rmat(hip, torch, scale, 1000), run_rmat(hip, torch, scale, E_ODD)
        assert np.array_equal(short[0], long_[0][:1000]) and np.array_equal(short[1], long_[1][:1000])
    short, long_ = run_er(hip, torch, 13, 1000), run_er(hip, torch, 13, E_ODD)
    assert np.array_equal(short[0], long_[0][:1000]) and np.array_equal(short[1], long_[1][:1000])


# ---- Chung-Lu -----------------------------------------------------------------------------------------

def run_chunglu(hip, torch, n_labels, E, go, vo, gi, vi, frac, nolink, seed):
    p = DevPair(torch, E + nolink)
    hip.gen_chunglu(0, n_labels, E, *p.ptrs(), gamma_out=go, v0_out=vo, gamma_in=gi, v0_in=vi, src_frac=frac,
                    n_nolink=nolink, seed=seed)
    return p.fetch()


def assert_chunglu_equal(name, got, g, E):
    """Link-less records and every draw outside the band: bitwise.  Inside the band: the label of the
    model's rank or of rank +- 1.  Returns (and prints) the number of draws that differed."""
    assert np.array_equal(got[0][E:], g.src[E:]) and np.array_equal(got[1][E:], g.dst[E:])
    assert np.all(got[1][E:] == -1)
    differed = []
    for end, dev, lab, rank, x, pl in (("src", got[0][:E], g.src[:E], g.rs[:E], g.xs, g.out),
                                       ("dst", got[1][:E], g.dst[:E], g.rd[:E], g.xd, g.inn)):
        amb = gm.ambiguous(x, pl.v0, pl.one_over_a)
        assert int(amb.sum()) <= 8, "test input outside the cap tests/test_gen_model_cpu.py checks"
        diff = dev != lab
        assert not np.any(diff & ~amb), (
            f"{name} {end}: {int((diff & ~amb).sum())} draws outside the band differ, first at "
            f"{int(np.argmax(diff & ~amb))}")
        for i in np.flatnonzero(diff):
            near = np.clip(np.array([rank[i] - 1, rank[i] + 1]), 0, pl.n - 1)
            assert int(dev[i]) in gm.apply_label_map(near, g.mul, g.add, g.n_labels).tolist(), (name, end, int(i))
        differed.append(int(diff.sum()))
        print(f"chunglu {name} {end}: {int(amb.sum())} draws in the band, {differed[-1]} differ from the model")
    return differed


@pytest.mark.parametrize("case", gm.CHUNGLU_CASES[:2], ids=[c[0] for c in gm.CHUNGLU_CASES[:2]])
def test_chunglu_small(hip, torch, case):
    name, n_labels, E, go, vo, gi, vi, frac, seed = case
    nolink = 1500
    g = gm.chunglu(n_labels, E, go, vo, gi, vi, frac, nolink, seed)
    assert_chunglu_equal(name, run_chunglu(hip, torch, n_labels, E, go, vo, gi, vi, frac, nolink, seed), g, E)


# ---- the bench's own workloads --------------------------------------------------------------------------

@pytest.mark.parametrize("graph,scale", [("rmat", 20), ("rmat", 26), ("er", 24)])
def test_baseline_rmat_er_prefix(hip, torch, graph, scale):
    """The first 2^20 raw records of the call sparky_hip.workloads.generate makes for BASELINE.json's
    R-MAT and Erdos-Renyi configs (edge i does not depend on the edge count)."""
    seed = hip.workloads.default_seed(graph, scale)
    if graph == "rmat":
        p = DevPair(torch, gm.PREFIX)
        hip.gen_rmat(0, scale, gm.PREFIX, *p.ptrs(), seed=seed)  # a, b, c: the wrapper's defaults, as generate()
        assert_edges_equal(p.fetch(), gm.rmat(scale, gm.PREFIX, *RMAT_DEFAULT, seed))
    else:
        assert_edges_equal(run_er(hip, torch, scale, gm.PREFIX, seed=seed), gm.er(scale, gm.PREFIX, seed))


@pytest.mark.parametrize("graph,case", [("lj", gm.CHUNGLU_CASES[2]), ("twitter", gm.CHUNGLU_CASES[3])])
def test_baseline_chunglu_prefix(hip, torch, graph, case):
    """The same for the two Chung-Lu presets, at the real n_labels and src_frac, with link-less records
    after the prefix: 1000 of them, or as many as the preset's sink-only ranks leave room for (the
    LiveJournal preset sends links from every rank, so none: the library refuses more)."""
    pre = hip.CHUNGLU_PRESETS[graph]
    seed = hip.workloads.default_seed(graph, 0)
    name, n_labels, E, go, vo, gi, vi, frac, case_seed = case
    assert (pre["n_labels"], pre["gamma_out"], pre["v0_out"], pre["gamma_in"], pre["v0_in"], pre["src_frac"],
            seed) == (n_labels, go, vo, gi, vi, frac, case_seed), "gen_model.CHUNGLU_CASES is out of date"
    assert E <= pre["n_edges"]
    nolink = min(1000, n_labels - int(frac * n_labels))
    assert nolink == (1000 if graph == "twitter" else 0)
    g = gm.chunglu(n_labels, E, go, vo, gi, vi, frac, nolink, seed)
    got = run_chunglu(hip, torch, pre["n_labels"], E, pre["gamma_out"], pre["v0_out"], pre["gamma_in"], pre["v0_in"],
                      pre["src_frac"], nolink, seed)
    assert_chunglu_equal(name, got, g, E)


# ---- the interner against first_appearance ---------------------------------------------------------------

def run_intern(hip, torch, src, dst, bound):
    """(V, src', dst', DevPair) through sparky_hip.intern_device."""
    p = DevPair(torch, len(src), src, dst)
    V = hip.intern_device(0, len(src), bound, *p.ptrs())
    s, d = p.fetch()
    return V, s, d, p


def assert_interned(hip, torch, src, dst, bound):
    src, dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    V, s, d, p = run_intern(hip, torch, src, dst, bound)
    Vm, sm, dm = gm.first_appearance(src, dst)
    assert V == Vm
    assert np.array_equal(s, sm), f"src: first difference at edge {int(np.argmax(s != sm))}"
    assert np.array_equal(d, dm), f"dst: first difference at edge {int(np.argmax(d != dm))}"
    return V, sm, dm, p


def assert_csr_builds(hip, oracle_c, V, sm, dm, p):
    csr = oracle_c.build_csr(V, sm, dm)
    with hip.PageRankGraph(V, *p.ptrs(), device_input=True, n_edges=p.n) as g:
        ex = g.export_csr()
    assert np.array_equal(ex.row_ptr, csr.row_ptr) and np.array_equal(ex.col_idx, csr.col_idx)
    assert np.array_equal(ex.out_deg, csr.out_deg) and np.array_equal(ex.vflags, csr.vflags)


def all_first_edges(rng, E, spare=3):
    """E edges whose 2E endpoints are distinct labels of [0, 2E + spare) in random order: every position is
    a first appearance, so the sort keys use every bit of bits_for(2E + 1)."""
    occ = rng.permutation(2 * E + spare)[:2 * E].astype(np.int32).reshape(E, 2)
    return occ[:, 0].copy(), occ[:, 1].copy(), 2 * E + spare


def test_intern_single_edge(hip, torch):
    assert_interned(hip, torch, [3], [5], 8)
    assert_interned(hip, torch, [3], [3], 8)
    assert_interned(hip, torch, [7], [-1], 8)
    assert_interned(hip, torch, [0], [0], 1)


def test_intern_self_loop_and_target_first(hip, torch):
    # 4 first appears as a self-loop (positions 0 and 1); 9 and 6 are first seen as targets and are the
    # source of the next edge; 6 then is a self-loop; 2 is first seen after a link-less record
    src = [4, 1, 9, 6, 2, 6]
    dst = [4, 9, 6, 6, -1, 2]
    V, sm, dm, _ = assert_interned(hip, torch, src, dst, 10)
    assert (V, sm.tolist(), dm.tolist()) == (5, [0, 1, 2, 3, 4, 3], [0, 2, 3, 3, -1, 4])


def test_intern_linkless_records(hip, torch):
    rng = np.random.default_rng(11)
    E, bound = 50_000, 20_000
    src = rng.integers(0, bound, E)
    dst = np.where(rng.random(E) < 0.3, -1, rng.integers(0, bound, E))
    assert 0.28 < np.mean(dst == -1) < 0.32
    assert_interned(hip, torch, src, dst, bound)


def test_intern_contended_hub(hip, torch, oracle_c):
    """One label in half of all positions: ~200 000 atomicMin candidates on one word, whose first
    occurrence is a target, not position 0."""
    rng = np.random.default_rng(12)
    E, bound, hub = 200_000, 5000, 4321
    occ = rng.integers(0, bound, 2 * E)
    occ[rng.random(2 * E) < 0.5] = hub
    occ[:7] = [17, 18, 19, 20, 21, 22, 23]
    occ[7] = hub  # the target of edge 3
    src, dst = occ[0::2].copy(), occ[1::2].copy()
    assert 0.49 < np.mean(occ == hub) < 0.51 and int(np.argmax(occ == hub)) == 7
    V, sm, dm, p = assert_interned(hip, torch, src, dst, bound)
    assert dm[3] == 7
    assert_csr_builds(hip, oracle_c, V, sm, dm, p)


def test_intern_sparse_label_bound(hip, torch):
    """1000 labels of a bound of 5 000 003 (no multiple of the 2048 tile): most compaction workgroups
    select nothing.  Labels 0 and bound - 1 are among them."""
    rng = np.random.default_rng(13)
    bound, E = 5_000_003, 20_000
    used = np.concatenate([[0, bound - 1], rng.choice(np.arange(1, bound - 1), 998, replace=False)])
    occ = used[rng.integers(0, used.size, 2 * E)]
    occ[:used.size] = rng.permutation(used)  # every one of the 1000 appears
    V, sm, dm, _ = assert_interned(hip, torch, occ[0::2], occ[1::2], bound)
    assert V == 1000


def test_intern_extreme_labels_first_and_last(hip, torch):
    bound = 4097
    V, sm, dm, _ = assert_interned(hip, torch, [bound - 1, 0, 5], [0, bound - 1, -1], bound)
    assert (V, sm.tolist(), dm.tolist()) == (3, [0, 1, 2], [1, 0, -1])


@pytest.mark.parametrize("nv", [2047, 2048, 2049])
def test_intern_around_one_tile(hip, torch, nv):
    rng = np.random.default_rng(nv)
    bound = 10_000
    used = rng.choice(bound, nv, replace=False)
    occ = np.concatenate([used, used[rng.integers(0, nv, nv + 2)]])  # 2 nv + 2 positions: E = nv + 1
    rng.shuffle(occ)
    V, sm, dm, _ = assert_interned(hip, torch, occ[0::2], occ[1::2], bound)
    assert V == nv


# E with bits_for(2E + 1) = 2, 8, 9, 15, 16, 17: the sort's last pass has 2, 8, 1, 7, 8, 1 bits
@pytest.mark.parametrize("E,bits", [(1, 2), (100, 8), (200, 9), (10_000, 15), (20_000, 16), (40_000, 17)])
def test_intern_sort_bit_counts(hip, torch, E, bits):
    assert (2 * E + 1).bit_length() == bits
    src, dst, bound = all_first_edges(np.random.default_rng(bits), E)
    V, sm, dm, _ = assert_interned(hip, torch, src, dst, bound)
    assert V == 2 * E and np.array_equal(sm, 2 * np.arange(E)) and np.array_equal(dm, 2 * np.arange(E) + 1)


def test_intern_two_tiles_per_workgroup(hip, torch, oracle_c):
    """4 400 000 labels, each once: label_bound and the number of keys both exceed 2048 * 2048, so the
    compaction and every radix pass give each workgroup two tiles (elsewhere reached at scale 20 and up,
    and compared with nothing but the CSR built downstream)."""
    E = 2_200_000
    assert 2 * E > 2048 * 2048
    src, dst, bound = all_first_edges(np.random.default_rng(14), E, spare=0)
    V, sm, dm, p = assert_interned(hip, torch, src, dst, bound)
    assert V == bound == 4_400_000
    assert_csr_builds(hip, oracle_c, V, sm, dm, p)


# ---- errors change nothing -------------------------------------------------------------------------------

def test_generator_errors_write_nothing(hip, torch):
    n = 1000
    p = DevPair(torch, 8192)  # room for every record a refused call asked for
    ok_cl = dict(gamma_out=2.2, v0_out=20.0, gamma_in=2.1, v0_in=10.0, src_frac=0.85, n_nolink=0, seed=5)
    lj = hip.CHUNGLU_PRESETS["lj"]
    calls = [
        lambda: hip.gen_rmat(0, 0, n, *p.ptrs()),
        lambda: hip.gen_rmat(0, 32, n, *p.ptrs()),
        lambda: hip.gen_er(0, 0, n, *p.ptrs()),
        lambda: hip.gen_er(0, 32, n, *p.ptrs()),
        lambda: hip.gen_rmat(0, 10, n, *p.ptrs(), a=-0.1),
        lambda: hip.gen_rmat(0, 10, n, *p.ptrs(), c=-1e-9),
        lambda: hip.gen_rmat(0, 10, n, *p.ptrs(), a=0.6, b=0.3, c=0.2),
        lambda: hip.gen_rmat(0, 10, n, *p.ptrs(), a=float("nan")),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "gamma_out": 2.0}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "gamma_in": 2.0}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "gamma_out": 1.0}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "gamma_in": 0.5}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "v0_out": 0.0}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "v0_in": -1.0}),
        lambda: hip.gen_chunglu(0, 30011, n - 10, *p.ptrs(), **{**ok_cl, "n_nolink": 30011 - int(0.85 * 30011) + 1}),
        lambda: hip.gen_chunglu(0, lj["n_labels"], n - 1, *p.ptrs(), **{**ok_cl, "src_frac": lj["src_frac"],
                                                                        "n_nolink": 1}),
        lambda: hip.gen_chunglu(0, 30011, n, *p.ptrs(), **{**ok_cl, "n_nolink": -1}),
        lambda: hip.gen_chunglu(0, 0, n, *p.ptrs(), **ok_cl),
        lambda: hip.gen_chunglu(0, -5, n, *p.ptrs(), **ok_cl),
        lambda: hip.gen_rmat(hip.device_count(), 10, n, *p.ptrs()),
        lambda: hip.gen_er(-1, 10, n, *p.ptrs()),
        lambda: hip.gen_chunglu(hip.device_count(), 30011, n, *p.ptrs(), **ok_cl),
        lambda: hip.gen_rmat(0, 10, -1, *p.ptrs()),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(hip.PageRankError) as e:
            call()
        assert e.value.code == PR_ERR_INVALID, k
    p.assert_untouched()
    # the largest n_nolink that fits is accepted (and the generators still work after the errors)
    room = 30011 - int(0.85 * 30011)
    q = DevPair(torch, 10 + room)
    hip.gen_chunglu(0, 30011, 10, *q.ptrs(), **{**ok_cl, "n_nolink": room})
    g = gm.chunglu(30011, 10, 2.2, 20.0, 2.1, 10.0, 0.85, room, 5)
    assert_chunglu_equal("errors_then_ok", q.fetch(), g, 10)


def test_zero_edges_is_not_an_error(hip, torch):
    p = DevPair(torch, 0)
    hip.gen_rmat(0, 10, 0, *p.ptrs())
    hip.gen_er(0, 10, 0, *p.ptrs())
    hip.gen_chunglu(0, 30011, 0, *p.ptrs(), gamma_out=2.2, v0_out=20.0, gamma_in=2.1, v0_in=10.0, src_frac=0.85,
                    n_nolink=0, seed=5)
    assert hip.intern_device(0, 0, 100, *p.ptrs()) == 0
    p.assert_untouched()


def test_intern_errors_change_nothing(hip, torch):
    from sparky_hip import _lib

    L = _lib.load()
    bound = 1000
    rng = np.random.default_rng(15)
    base_s, base_d = rng.integers(0, bound, 5000).astype(np.int32), rng.integers(0, bound, 5000).astype(np.int32)
    base_d[::7] = -1

    def call(src, dst, label_bound):
        p = DevPair(torch, len(src), src, dst)
        nv = ctypes.c_int32(-77)
        rc = L.pr_intern_device(0, len(src), label_bound, ctypes.c_void_p(p.s.data_ptr()),
                                ctypes.c_void_p(p.d.data_ptr()), ctypes.byref(nv))
        s, d = p.fetch()
        return rc, nv.value, s, d

    bad = []
    for which, value in (("s", bound), ("s", -1), ("d", -2), ("d", bound), ("s", 2**31 - 1), ("d", -(2**31))):
        s, d = base_s.copy(), base_d.copy()
        (s if which == "s" else d)[3210] = value
        bad.append((s, d, bound))
    bad.append((base_s, base_d, 0))
    bad.append((base_s, base_d, -3))
    for k, (s, d, b) in enumerate(bad):
        rc, nv, s2, d2 = call(s, d, b)
        assert rc == PR_ERR_INVALID, k
        assert nv == -77, k
        assert np.array_equal(s2, s) and np.array_equal(d2, d), k
    # and the same arrays without the bad label intern as the model says
    rc, nv, s2, d2 = call(base_s, base_d, bound)
    Vm, sm, dm = gm.first_appearance(base_s, base_d)
    assert rc == 0 and nv == Vm and np.array_equal(s2, sm) and np.array_equal(d2, dm)
