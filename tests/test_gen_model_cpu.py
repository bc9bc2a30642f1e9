"""tests/gen_model.py against the generators' definition (no GPU): every test checks a property the
definition states -- a bijection, a quadrant probability, a power law, a record layout -- never the
model's agreement with any code.  Statistical bounds are computed from n and the stated probability:
6 sigma for a binomial share or a correlation, the DKW bound with delta = 1e-9 for a CDF distance,
the 1e-9 upper quantile for a chi-square.  All seeds are fixed, so every test is deterministic.
"""
import math
from statistics import NormalDist

import numpy as np
import pytest

import gen_model as gm

DELTA = 1e-9

CHUNGLU_CASES = gm.CHUNGLU_CASES
AMBIGUOUS_CAP = 8


def chi2_upper(dof: int, delta: float) -> float:
    """Wilson-Hilferty: (X/dof)^(1/3) is normal(1 - 2/(9 dof), 2/(9 dof)) to O(dof^-3/2); at dof >= 255
    the quantile it gives is within 0.1 % of the exact one, and the statistics below sit near dof."""
    z = NormalDist().inv_cdf(1.0 - delta)
    v = 2.0 / (9.0 * dof)
    return dof * (1.0 - v + z * math.sqrt(v)) ** 3


def dkw(n: int, delta: float = DELTA) -> float:
    return math.sqrt(math.log(2.0 / delta) / (2.0 * n))


def corr(x, y) -> float:
    x = x.astype(np.float64) - x.mean()
    y = y.astype(np.float64) - y.mean()
    return float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum()))


def test_splitmix64_known_values():
    # the published SplitMix64 stream from state 0 (Steele, Lea, Flood 2014; Vigna's splitmix64.c):
    # splitmix64(x) here is "advance the state x by the golden gamma, then mix"
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    state = 0
    for w in want:
        assert gm.splitmix64_int(state) == w
        assert int(gm.splitmix64(np.array([state], np.uint64))[0]) == w
        state = (state + gm.GOLDEN) & gm.MASK64


def test_edge_hash_is_counter_based():
    i = np.arange(1000, dtype=np.uint64)
    a = gm.edge_hash(7, i, 3)
    assert np.array_equal(a[500:], gm.edge_hash(7, i[500:], 3))
    assert not np.array_equal(a, gm.edge_hash(7, i, 4)) and not np.array_equal(a, gm.edge_hash(8, i, 3))
    assert np.unique(a).size == 1000


@pytest.mark.parametrize("seed", [0, 1, (1 << 63) + 12345])
def test_scramble_is_a_bijection(seed):
    for scale in range(1, 17):
        out = gm.scramble(np.arange(1 << scale, dtype=np.uint64), scale, seed)
        assert out.max() < (1 << scale)
        assert np.unique(out).size == 1 << scale, scale


def test_thr_saturates():
    assert gm.thr(0.0) == 0 and gm.thr(1.0) == 0xFFFFFFFF and gm.thr(0.5) == 1 << 31
    assert gm.thr(1.0 - 2.0 ** -33) == 0xFFFFFFFF  # x = 2^32 - 0.5 >= 4294967295.0
    assert gm.thr(0.57) == int(0.57 * 4294967296.0)


def test_rmat_quadrant_shares_and_independence():
    a, b, c = 0.57, 0.19, 0.05  # b != c on purpose: a swapped convention cannot pass
    scale, n = 11, 1 << 20
    s, d = gm.rmat(scale, n, a, b, c, 1234, scrambled=False)
    assert s.max() < (1 << scale) and d.max() < (1 << scale)
    probs = [a, b, c, 1.0 - a - b - c]  # quadrant index = 2 * src bit + dst bit
    quad = [2 * ((s >> l) & 1) + ((d >> l) & 1) for l in range(scale)]
    for l in range(scale):
        shares = np.bincount(quad[l], minlength=4) / n
        for q, p in enumerate(probs):
            assert abs(shares[q] - p) <= 6.0 * math.sqrt(p * (1.0 - p) / n), (l, q, shares[q])
    # levels (2k, 2k+1) share one hash (its two halves); (2k+1, 2k+2) come from different hashes
    for l in range(scale - 1):
        for q0 in range(4):
            for q1 in range(4):
                r = corr(quad[l] == q0, quad[l + 1] == q1)
                assert abs(r) <= 6.0 / math.sqrt(n), (l, q0, q1, r)


def test_rmat_top_bit_of_an_odd_scale():
    # scale 5: level 4 is the low half of hash 2 and no level 5 exists
    s, d = gm.rmat(5, 1 << 16, 0.57, 0.19, 0.19, 9, scrambled=False)
    s4, d4 = gm.rmat(4, 1 << 16, 0.57, 0.19, 0.19, 9, scrambled=False)
    assert s.max() < 32 and d.max() < 32
    assert np.array_equal(s & 15, s4) and np.array_equal(d & 15, d4)
    top = 2 * (s >> 4) + (d >> 4)
    assert abs(np.mean(top == 0) - 0.57) <= 6.0 * math.sqrt(0.57 * 0.43 / (1 << 16))


def test_rmat_degenerate_corners():
    scale, n, seed = 16, 1 << 16, 3
    s, d = gm.rmat(scale, n, 1.0, 0.0, 0.0, seed)
    zero = int(gm.scramble(np.array([0], np.uint64), scale, seed)[0])
    assert np.all(s == zero) and np.all(d == zero)
    s, d = gm.rmat(scale, n, 0.0, 0.0, 0.0, seed)
    ones = int(gm.scramble(np.array([(1 << scale) - 1], np.uint64), scale, seed)[0])
    assert np.all(s == ones) and np.all(d == ones)
    # a + b + c == 1.0 is accepted and leaves quadrant d empty (but for u == 0xFFFFFFFF, 2^-32 a bit)
    s, d = gm.rmat(scale, n, 0.5, 0.25, 0.25, seed, scrambled=False)
    assert not np.any(s & d)
    with pytest.raises(ValueError):
        gm.rmat(scale, n, 0.5, 0.3, 0.25, seed)
    with pytest.raises(ValueError):
        gm.rmat(scale, n, -0.1, 0.3, 0.25, seed)


def test_er_uniform_and_uncorrelated():
    scale, n = 8, 1 << 20
    L = 1 << scale
    s, d = gm.er(scale, n, 3)
    for x in (s, d):
        cnt = np.bincount(x, minlength=L)
        assert cnt.size == L
        assert float(((cnt - n / L) ** 2).sum() / (n / L)) <= chi2_upper(L - 1, DELTA)
    assert abs(corr(s, d)) <= 6.0 / math.sqrt(n)
    joint = np.bincount(s.astype(np.int64) * L + d, minlength=L * L)
    assert float(((joint - n / (L * L)) ** 2).sum() / (n / (L * L))) <= chi2_upper(L * L - 1, DELTA)


@pytest.mark.parametrize("gamma_out,gamma_in", [(2.2, 2.1), (1.5, 1.8), (3.0, 1.2)])
def test_chunglu_rank_distribution(gamma_out, gamma_in):
    n_labels, E = 30011, 400_000
    g = gm.chunglu(n_labels, E, gamma_out, 20.0, gamma_in, 10.0, 0.85, 100, 5)
    assert (g.out.a < 0) == (gamma_out < 2) and (g.inn.a < 0) == (gamma_in < 2)
    for ranks, pl in ((g.rs[:E], g.out), (g.rd[:E], g.inn)):
        assert ranks.min() >= 0 and ranks.max() < pl.n
        ecdf = np.cumsum(np.bincount(ranks, minlength=pl.n)) / E
        want = pl.cdf(np.arange(1, pl.n + 1, dtype=np.float64))  # P(rank <= r) = F(r + 1)
        assert abs(want[-1] - 1.0) < 1e-12 and abs(pl.cdf(0.0)) < 1e-12
        assert float(np.max(np.abs(ecdf - want))) <= dkw(E)
    # the two endpoints come from different draws
    assert abs(corr(g.rs[:E], g.rd[:E])) <= 6.0 / math.sqrt(E)


# prime, and composite 30030 = 2*3*5*7*11*13 with a seed whose first multiplier candidate is not coprime
# to it (18681 = 3*13*479; with seed 5 it would be), so that the gcd loop has to step: five times, to 18691
COMPOSITE = (gm.CHUNGLU_CASES[1][1], gm.CHUNGLU_CASES[1][-1])


@pytest.mark.parametrize("n_labels,seed", [(30011, 5), COMPOSITE])
def test_chunglu_records_and_label_map(n_labels, seed):
    E, nolink = 400_000, 1500
    g = gm.chunglu(n_labels, E, 2.2, 20.0, 2.1, 10.0, 0.85, nolink, seed)
    assert g.n_src == int(0.85 * n_labels)
    assert g.rs[:E].max() < g.n_src  # sink-only ranks never send a link
    assert np.array_equal(g.rs[E:], g.n_src + np.arange(nolink)) and np.all(g.rd[E:] == -1)
    assert np.all(g.dst[E:] == -1) and np.all(g.dst[:E] >= 0)
    assert math.gcd(g.mul, n_labels) == 1 and g.mul % 2 == 1 and 0 <= g.add < n_labels
    lab = gm.apply_label_map(np.arange(n_labels), g.mul, g.add, n_labels)
    assert lab.min() == 0 and lab.max() == n_labels - 1 and np.unique(lab).size == n_labels
    assert np.array_equal(g.src, lab[g.rs]) and np.array_equal(g.dst[:E], lab[g.rd[:E]])
    if n_labels == 30030:  # the first candidate shares a factor with 2*3*5*7*11*13: the gcd loop ran
        first = (gm.splitmix64_int(seed + 23) % n_labels) | 1
        assert (n_labels, seed, first) == (30030, 7, 18681)
        assert math.gcd(first, n_labels) != 1 and g.mul > first and (g.mul - first) % 2 == 0
        assert all(math.gcd(m, n_labels) != 1 for m in range(first, g.mul, 2))


@pytest.mark.parametrize("case", CHUNGLU_CASES, ids=[c[0] for c in CHUNGLU_CASES])
def test_chunglu_ambiguity_cap(case):
    """A condition on the test inputs, not a measurement of any device: the model alone finds at most
    AMBIGUOUS_CAP draws per endpoint array inside the derived band, so the GPU comparison is bitwise
    on all but a handful of named draws."""
    name, n_labels, E, go, vo, gi, vi, frac, seed = case
    g = gm.chunglu(n_labels, E, go, vo, gi, vi, frac, 0, seed)
    for x, pl in ((g.xs, g.out), (g.xd, g.inn)):
        assert pl.a > 0 and gm.band(pl.one_over_a) < 2.0 ** -43
        n_amb = int(gm.ambiguous(x, pl.v0, pl.one_over_a).sum())
        print(f"{name}: 1/a={pl.one_over_a:.3f} band={gm.band(pl.one_over_a):.3e} ambiguous={n_amb}")
        assert n_amb <= AMBIGUOUS_CAP


def test_ambiguous_marks_only_integer_boundaries():
    v0, ooa = 50.0, 11.0
    w = gm.band(ooa)
    x = np.array([5.0, 5.0 + 0.5 * w * 55, 5.0 - 0.5 * w * 55, 5.0 + 4 * w * 55, 5.5, 0.0, -1e-13, 1e-13, 1.0])
    assert gm.ambiguous(x, v0, ooa).tolist() == [True, True, True, False, False, False, False, False, True]
    with pytest.raises(ValueError):
        gm.band(-1.0)


def test_first_appearance():
    src = np.array([7, 7, 3, 9, 3], np.int32)
    dst = np.array([7, 2, -1, 3, 0], np.int32)
    V, s, d = gm.first_appearance(src, dst)
    # positions: 7@0, 7@1, 7@2, 2@3, 3@4, 9@6, 3@7, 3@8, 0@9  ->  7:0 2:1 3:2 9:3 0:4
    assert V == 5 and s.tolist() == [0, 0, 2, 3, 2] and d.tolist() == [0, 1, -1, 2, 4]
    V, s, d = gm.first_appearance(np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert V == 0 and s.size == 0 and d.size == 0
    # a label first seen as a target is numbered before the source of the next edge
    V, s, d = gm.first_appearance(np.array([5, 1], np.int32), np.array([1, 5], np.int32))
    assert V == 2 and s.tolist() == [0, 1] and d.tolist() == [1, 0]


def test_recorded_rmat_s20_workload():
    """BASELINE.json configs[0] -- R-MAT scale 20, edge factor 16, seed 1 -- as recorded by the bench in
    profiles/r06/validate_final6/bench_s20.log:
        [bench] rank 0: generated + interned 16777216 edges, V=646540 in 0.09s
        [bench] rank 0: build 22 ms; info {'n_vertices': 646540, 'n_edges': 16085535, ...
    The model, written from the definition, reproduces both counts: it generates the graph every
    recorded number was measured on."""
    scale, E, chunk = 20, 16 << 20, 1 << 21
    seen = np.zeros(1 << scale, bool)
    keys = np.empty(E, np.uint64)
    for start in range(0, E, chunk):
        s, d = gm.rmat(scale, chunk, 0.57, 0.19, 0.19, 1, start=start)
        seen[s] = True
        seen[d] = True
        keys[start:start + chunk] = (d.astype(np.uint64) << np.uint64(scale)) | s.astype(np.uint64)
    assert int(seen.sum()) == 646_540
    keys.sort()
    assert 1 + int(np.count_nonzero(keys[1:] != keys[:-1])) == 16_085_535
