"""Inputs on which one PageRank iteration has exactly one correct bit pattern, and that pattern.

The engine's claims are bit-level claims (A6 `c = r / d` is a true division, A10
`t + damping * (S + dc / N)` with every operation rounded on its own, A8 `S = r_old` for rows without
in-links, "every sum has a fixed order"), but a floating-point sum has as many correct answers as
it has orders, so a test against the oracle needs a tolerance and a test between two variants of the
engine sees nothing that all variants share.  This module removes the order: it builds inputs on
which every sum is exact in any association, so the expected bits follow from the specification
alone and every path -- layout, class count, code width, gather path, epilogue form, partition,
exchange mode, the batch -- has to produce them.  numpy and Python integers only; it imports nothing
from sparky_hip and loads no shared library.  tests/test_exact_model_cpu.py checks it against the
oracle without a GPU, tests/test_gpu_exact.py holds the library to it.

Family D ("dyadic", dyadic_run): exact for several iterations.
  Every source has a power-of-two out-degree, damping is a power of two (0.5), the teleport term
  (scalar or per-vertex) and the initial ranks are non-negative multiples of 2^-4, and N is a power
  of two when the graph has sinks and their mass is shared out (so dc / N is a shift).  Then after
  iteration k every rank, contribution, row sum, dc and L1 term is a non-negative multiple of
  2^-F_k.  All addends being non-negative, every partial sum of any association is bounded by the
  total, so if total * 2^F_k < 2^53 every partial sum is an integer below 2^53 on that grid: exactly
  representable, and every order gives the same bits.  The model carries the iteration in integers on
  that grid and says for how many iterations the bound holds (`exact_iters`).

Family S ("one step", one_step): the product's own 0.15 / 0.85 on any graph.
  r0[v] = k_v * d(v) * 2^-10 with random integers k_v in [1, 2^20) (d(v) = 0: k_v * 2^-10), so
  r0 / d is exactly k_v * 2^-10 and all row sums and dc are integers on that grid.  Iteration 1 is
  then exact for every row under the four separately rounded operations of A10; iteration 2 is exact
  for the rows with in-degree 0 (S = r1[v]) or 1 (S = fl(r1[u] / d(u))) as long as dc1 is order-free
  (at most two sinks, or dangling = "none").  Iteration 2 is what pins the true division of every
  site that writes c', and the exchange that carries c' to another part.
"""
from collections import namedtuple

import numpy as np

GRID_BITS = 4  # teleport terms and initial ranks: non-negative multiples of 2^-4
MANT = 53  # an integer below 2^53 times a power of two is a float64
S_SHIFT = 10  # Family S: r0 / d = k * 2^-10
S_KMAX = 1 << 20


class Graph:
    """The deduplicated in-link structure of a raw edge list (dst == -1: a record without links),
    restated with numpy: SURVEY.md A1-A4."""

    def __init__(self, V, src, dst):
        src = np.asarray(src, np.int64)
        dst = np.asarray(dst, np.int64)
        if src.shape != dst.shape or src.ndim != 1:
            raise ValueError("src and dst: 1-D arrays of one length")
        if src.size and (src.min() < 0 or src.max() >= V or dst.min() < -1 or dst.max() >= V):
            raise ValueError("ID out of range")
        link = dst >= 0
        key = np.unique(dst[link] * V + src[link])  # distinct (dst, src), rows ascending, sources ascending
        self.V = int(V)
        self.rows = key // V
        self.cols = key % V
        self.out_deg = np.bincount(self.cols, minlength=V).astype(np.int64)
        self.in_deg = np.bincount(self.rows, minlength=V).astype(np.int64)
        is_key = np.zeros(V, bool)
        is_key[src] = True
        seen = is_key.copy()
        seen[dst[link]] = True
        if not seen.all():
            raise ValueError("an ID in [0, V) appears nowhere")
        self.sink = ~is_key  # targets that are never a record (A4)
        self.nolink = is_key & (self.out_deg == 0)
        self.has_in = self.in_deg > 0
        # row sums by reduceat over the non-empty rows (rows is sorted)
        self._starts = np.concatenate([[0], np.cumsum(self.in_deg)])[:-1][self.has_in]

    def row_sums(self, per_source):
        """sum over in-links of per_source[source], for every row (0 for rows without in-links), in
        the dtype of per_source (int64: exact as long as no row sum reaches 2^63)."""
        out = np.zeros(self.V, per_source.dtype)
        if self.cols.size:
            out[self.has_in] = np.add.reduceat(per_source[self.cols], self._starts)
        return out


def _on_grid(x, what):
    """x * 2^GRID_BITS as int64, or ValueError if x is not a finite non-negative multiple of 2^-GRID_BITS."""
    a = np.atleast_1d(np.asarray(x, np.float64))
    s = a * float(1 << GRID_BITS)
    if not (np.isfinite(a).all() and (a >= 0).all() and (a < 2.0 ** 31).all() and (s == np.floor(s)).all()):
        raise ValueError(f"{what} must be non-negative multiples of 2^-{GRID_BITS}")
    return s.astype(np.int64)


def _bits(n):
    return int(n).bit_length()


_HALF = 30


def _int_sum(a):
    """The sum of non-negative int64 values below 2^62 as a Python integer (fewer than 2^30 of them)."""
    return (int((a >> _HALF).sum()) << _HALF) + int((a & ((1 << _HALF) - 1)).sum())


def _pow2_shift(x, what):
    """s with x == 2^-s, s >= 0."""
    m, e = np.frexp(float(x))
    if m != 0.5 or e > 1:
        raise ValueError(f"{what} must be 2^-s with s >= 0")
    return 1 - int(e)


DyadicRun = namedtuple("DyadicRun", "ranks dc l1 exact_iters grid_bits width_bits")


def dyadic_run(g, iters, teleport=0.25, damping=0.5, init=None, dangling="local"):
    """Family D on Graph `g`.  Returns DyadicRun:

      ranks[k], dc[k], l1[k]   float64, iteration k + 1's ranks (original-ID order), the dangling sum
                               it used and its L1 delta (the oracle's indexing), for as many
                               iterations (<= iters) as the ranks are certified exact;
      exact_iters              {"ranks", "dc", "l1"}: the number of leading iterations for which the
                               bound total * 2^F < 2^53 holds for every quantity of that kind
                               (and for what it is computed from);
      grid_bits[k]             F after iteration k + 1;
      width_bits[k]            bit length of the largest integer iteration k + 1 met on its grids
                               (L1 excluded): <= 53 is what "exact" means.

    Raises ValueError for an input outside the family: a source whose out-degree is not a power of
    two, sinks with N not a power of two (dangling = "local"), teleport terms or initial ranks off the
    2^-4 grid or negative, a damping that is not 2^-s."""
    V = g.V
    if dangling not in ("local", "none"):
        raise ValueError("dangling must be 'local' or 'none'")
    d = g.out_deg
    if (g.nolink.any()) or (d[~g.sink] & (d[~g.sink] - 1)).any():
        raise ValueError("every source's out-degree must be a power of two")
    lgd = np.zeros(V, np.int64)
    lgd[~g.sink] = np.round(np.log2(d[~g.sink])).astype(np.int64)
    lgd_max = int(lgd.max()) if V else 0
    share = dangling == "local" and bool(g.sink.any())
    lgN = 0
    if share:
        if V & (V - 1):
            raise ValueError("with sinks, N must be a power of two")
        lgN = V.bit_length() - 1
    s_damp = _pow2_shift(damping, "damping")
    t_int = _on_grid(teleport, "teleport terms")
    if t_int.shape not in ((1,), (V,)):
        raise ValueError("teleport: a scalar or V values")
    r_int = _on_grid(np.ones(V) if init is None else init, "initial ranks")
    if r_int.shape != (V,):
        raise ValueError("init: V values")
    F = GRID_BITS
    # drop the grid bits nobody uses, so that ranks of 1.0 start at F = 0
    while F > 0 and not (r_int & 1).any():
        r_int >>= 1
        F -= 1
    t_bits = GRID_BITS
    while t_bits > 0 and not (t_int & 1).any():
        t_int >>= 1
        t_bits -= 1
    in_max = int(g.in_deg.max()) if V else 0

    ranks, dcs, l1s, grid, width = [], [], [], [], []
    l1_ok = True
    n_l1 = 0
    for _ in range(iters):
        G = F + lgd_max  # contributions: r / d
        c_int = r_int << (lgd_max - lgd)
        c_int[g.sink] = 0
        c_max = int(c_int.max()) if V else 0
        if _bits(c_max) > MANT:
            break
        s_hi = g.row_sums(c_int >> _HALF)  # in two halves, so that no int64 sum can wrap
        if _bits(int(s_hi.max())) + _HALF > 62:
            break  # a row sum far past 2^53
        S = (s_hi << _HALF) + g.row_sums(c_int & ((1 << _HALF) - 1))
        S[~g.has_in] = r_int[~g.has_in] << lgd_max  # A8: the old rank as the sum
        dc_int = _int_sum(r_int[g.sink]) if share else 0  # on grid F
        G2 = max(G, F + lgN) if share else G
        x_int = (S << (G2 - G)) + (dc_int << (G2 - F - lgN))  # S + dc / N
        Fn = max(G2 + s_damp, t_bits)  # damping * x is the same integer on grid G2 + s
        if _bits(int(x_int.max())) + (Fn - G2 - s_damp) > 62 or _bits(int(t_int.max())) + Fn - t_bits > 62:
            break
        rn_int = (t_int << (Fn - t_bits)) + (x_int << (Fn - G2 - s_damp))
        w = max(_bits(c_max), _bits(int(S.max())), _bits(dc_int), _bits(int(x_int.max())), _bits(int(rn_int.max())))
        if w > MANT:
            break
        l1_int = _int_sum(np.abs(rn_int - (r_int << (Fn - F))))
        l1_ok = l1_ok and _bits(l1_int) <= MANT
        n_l1 += l1_ok
        ranks.append(np.ldexp(rn_int.astype(np.float64), -Fn))
        dcs.append(float(np.ldexp(float(dc_int), -F)))
        l1s.append(float(np.ldexp(float(l1_int), -Fn)) if l1_ok else float("nan"))
        grid.append(Fn)
        width.append(w)
        r_int, F = rn_int, Fn
    n = len(ranks)
    return DyadicRun(ranks, np.array(dcs), np.array(l1s), {"ranks": n, "dc": n, "l1": n_l1}, grid, width)


def float_run(g, iters, teleport, damping, init=None, dangling="local"):
    """The specification in float64 with numpy's own sequential sums (np.add.reduceat), every
    operation a ufunc call of its own: on a Family D input it must reproduce dyadic_run's bits, which
    checks the integer recurrence where the oracle cannot (a per-vertex teleport vector).  Returns
    (ranks[k], dc[k], l1[k])."""
    V = g.V
    r = np.ones(V) if init is None else np.array(init, np.float64)
    t = np.asarray(teleport, np.float64)
    d = np.where(g.out_deg > 0, g.out_deg, 1).astype(np.float64)
    ranks, dcs, l1s = [], [], []
    for _ in range(iters):
        c = np.divide(r, d)
        c[g.out_deg == 0] = 0.0
        S = g.row_sums(c)
        S[~g.has_in] = r[~g.has_in]
        dc = float(np.add.reduce(r[g.sink])) if dangling == "local" else 0.0
        x = np.add(S, np.divide(dc, float(V)))
        y = np.multiply(damping, x)
        rn = np.add(t, y)
        ranks.append(rn)
        dcs.append(dc)
        l1s.append(float(np.add.reduce(np.abs(np.subtract(rn, r)))))
        r = rn
    return ranks, np.array(dcs), np.array(l1s)


OneStep = namedtuple("OneStep", "r0 r1 r2 mask dc")


def one_step_init(g, seed):
    """Family S initial ranks: r0[v] = k_v * d(v) * 2^-10, k_v a random integer in [1, 2^20)
    (d(v) = 0: k_v * 2^-10).  Returns (r0, k)."""
    k = np.random.default_rng(seed).integers(1, S_KMAX, g.V, dtype=np.int64)
    r0 = np.ldexp((k * np.maximum(g.out_deg, 1)).astype(np.float64), -S_SHIFT)
    return r0, k


def one_step(g, k, teleport=0.15, damping=0.85, dangling="local"):
    """Family S on Graph `g` from one_step_init's k.  Returns OneStep:

      r0, r1   the initial ranks and the exact ranks after iteration 1, all rows;
      r2, mask ranks after iteration 2, exact where mask (in-degree 0 or 1), NaN elsewhere; the mask
               is empty when dc1 would depend on the order (more than two sinks, dangling "local");
      dc       [dc0, dc1] (dc1 NaN with an empty mask).

    teleport: a scalar or V values, any float64."""
    V = g.V
    if k.shape != (V,) or k.min() < 1 or k.max() >= S_KMAX:
        raise ValueError("k: V integers in [1, 2^20)")
    if int(g.in_deg.max()) * S_KMAX >= 1 << MANT or int(g.out_deg.max()) * S_KMAX >= 1 << MANT:
        raise ValueError("degrees too large for exact sums")
    t = np.asarray(teleport, np.float64)
    d = np.maximum(g.out_deg, 1)
    r0 = np.ldexp((k * d).astype(np.float64), -S_SHIFT)
    c_int = np.where(g.out_deg > 0, k, 0)
    S = np.ldexp(g.row_sums(c_int).astype(np.float64), -S_SHIFT)
    S[~g.has_in] = r0[~g.has_in]
    share = dangling == "local"
    dc0 = float(np.ldexp(float(int(k[g.sink].sum())), -S_SHIFT)) if share else 0.0
    if int(k[g.sink].sum()) >= 1 << MANT:
        raise ValueError("too many sinks for an exact dc")

    def affine(S_, dc_):
        tdc = np.divide(np.float64(dc_), np.float64(V))
        x = np.add(S_, tdc)
        y = np.multiply(np.float64(damping), x)
        return np.add(t, y)

    r1 = affine(S, dc0)
    sinks = np.nonzero(g.sink)[0]
    order_free = (not share) or sinks.size <= 2
    mask = (g.in_deg <= 1) & order_free
    r2 = np.full(V, np.nan)
    dc1 = float("nan")
    if order_free:
        dc1 = 0.0
        if share:
            for s in sinks:  # at most two terms: a float sum of two is commutative, and 0 + x is x
                dc1 = float(np.add(np.float64(dc1), r1[s]))
        S2 = r1.copy()  # in-degree 0: the old rank
        one = np.nonzero(g.in_deg == 1)[0]
        starts = np.concatenate([[0], np.cumsum(g.in_deg)])[:-1]
        u = g.cols[starts[one]]  # the single source of such a row
        S2[one] = np.divide(r1[u], g.out_deg[u].astype(np.float64))
        full = affine(S2, dc1)
        r2[mask] = full[mask]
    return OneStep(r0, r1, r2, mask, np.array([dc0, dc1]))


# ---- input builders (seeded; each returns a namedtuple with (V, src, dst) and the facts the CPU test asserts) ----
DyadicInput = namedtuple("DyadicInput", "name V src dst hub hub_in n_sinks n_indeg0")


def dyadic_graph(name, V, seed, hub_in, n_sinks=0, n_indeg0=0, n_dup=500, deg_p=(1 / 3, 1 / 3, 1 / 3)):
    """V vertices, of which the last-but-spread n_sinks are sink-only; every other vertex is a source
    with 1, 2 or 4 distinct targets.  Vertex `hub` is a target of at least hub_in sources; n_indeg0
    sources are nobody's target.  n_dup raw records are repeated (the build dedupes them).  deg_p: the
    shares of out-degree 1, 2 and 4."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(V)
    sinks = np.sort(ids[:n_sinks])
    lonely = ids[n_sinks:n_sinks + n_indeg0]  # sources without in-links
    hub = int(ids[n_sinks + n_indeg0])
    is_src = np.ones(V, bool)
    is_src[sinks] = False
    srcs = np.nonzero(is_src)[0]
    in_pool = np.ones(V, bool)
    in_pool[lonely] = False
    pool = np.nonzero(in_pool)[0]  # targets: everything but the lonely sources (sinks and the hub included)
    M, n = pool.size, srcs.size
    # four distinct targets per source: pool[(b + o_j) % M] with 0 = o_0 < o_1 < o_2 < o_3 < M
    q = M // 4
    b = rng.integers(0, M, n)
    o1 = 1 + rng.integers(0, q - 1, n)
    o2 = o1 + 1 + rng.integers(0, q - 1, n)
    o3 = o2 + 1 + rng.integers(0, q - 1, n)
    tgt = pool[(b[:, None] + np.stack([np.zeros(n, np.int64), o1, o2, o3], 1)) % M]
    deg = rng.choice(np.array([1, 2, 4]), n, p=deg_p)
    # forced targets go to slot 0 of sources none of whose slots holds one yet
    special = np.concatenate([[hub], sinks])
    free = np.nonzero(~np.isin(tgt, special).any(axis=1))[0]
    free = free[rng.permutation(free.size)]
    if free.size < hub_in + n_sinks:
        raise ValueError("not enough sources for the hub")
    tgt[free[:hub_in], 0] = hub
    for i, s in enumerate(sinks):  # every sink is somebody's target
        tgt[free[hub_in + i], 0] = s
    keep = np.arange(4)[None, :] < deg[:, None]
    src = np.repeat(srcs, 4).reshape(n, 4)[keep]
    dst = tgt[keep]
    dup = rng.integers(0, src.size, n_dup)
    src = np.concatenate([src, src[dup]]).astype(np.int32)
    dst = np.concatenate([dst, dst[dup]]).astype(np.int32)
    return DyadicInput(name, V, src, dst, hub, hub_in, n_sinks, n_indeg0)


# The small inputs are sparse beside their hub (about one in-link per row), so that the 512-row
# groups of the split layout's epilogue fit one window and walk their rows' own slots at every class
# count up to 64 (PR_INFO_WALK_GROUPS); PR_BOPT_EPI_WALK = 0 and 128 classes run the class loop.
SPARSE = (0.7, 0.2, 0.1)


def small():
    return dyadic_graph("small", 4096, 101, 3000, n_indeg0=300, deg_p=SPARSE)


def hub9k():
    return dyadic_graph("hub9k", 16384, 102, 9000, n_indeg0=500, deg_p=SPARSE)


def hub_fused_65():
    """A row of more than 64 * 2048 in-links: 65 or more pieces in the fused layout's k_finalize."""
    return dyadic_graph("hub_fused_65", 150000, 103, 135000, n_indeg0=1000)


def hub_split_65():
    """At 8 classes every class segment of the hub has more than 64 * 512 in-links: 65 or more
    pieces per segment in k_seg_reduce."""
    return dyadic_graph("hub_split_65", 300000, 104, 282000, n_indeg0=1000)


def sinks5():
    return dyadic_graph("sinks5", 4096, 105, 3000, n_sinks=5, n_indeg0=300, deg_p=SPARSE)


def sinks3():
    return dyadic_graph("sinks3", 1024, 106, 700, n_sinks=3, n_indeg0=60)


def sinks1():
    return dyadic_graph("sinks1", 4096, 107, 3000, n_sinks=1, n_indeg0=300)


DYADIC_BUILDERS = {"small": small, "hub9k": hub9k, "hub_fused_65": hub_fused_65, "hub_split_65": hub_split_65,
                   "sinks5": sinks5, "sinks3": sinks3, "sinks1": sinks1}
SINK_FREE = ("small", "hub9k", "hub_fused_65", "hub_split_65")
WITH_SINKS = ("sinks5", "sinks3", "sinks1")
MIN_ITERS_SINK_FREE = 8  # exact_iters the tests require of the model
MIN_ITERS_SINKS = 3

FUSED_UNIT = 2048  # in-links of a fused-layout unit (pr_internal.h kUnitNnz): a longer row is cut into pieces
WAVE_UNIT = 512  # entries of a wave unit (pr_internal.h kWaveUnit): a longer (row, class) segment is cut into pieces
LAP = 64  # pieces one lap of k_finalize's / k_seg_reduce's loop adds


def grid_vector(V, seed, hot=()):
    """A per-vertex teleport vector on the grid: multiples of 1/16 in [0, 2], with `hot` set to 1.75."""
    t = np.random.default_rng(seed).integers(0, 33, V).astype(np.float64) / 16.0
    for v in hot:
        t[v] = 1.75
    return t


def grid_init(V, seed):
    """Initial ranks on the grid: multiples of 2^-4 in [1/16, 2]."""
    return np.random.default_rng(seed).integers(1, 33, V).astype(np.float64) / 16.0


OneStepInput = namedtuple("OneStepInput", "V src dst sinks hub")
S_V, S_E, S_SEED = 20011, 26000, 201


def one_step_graph():
    """Family S graph: V = 20011 (ragged: no multiple of 64), ~1.3 in-links per vertex so that
    thousands of rows have in-degree 0 or 1 (and the epilogue groups walk), a hub, duplicates, self-loops, 5 % records without
    links, two sink-only vertices."""
    rng = np.random.default_rng(S_SEED)
    V, E = S_V, S_E
    src = rng.integers(0, V, E, dtype=np.int64)
    dst = rng.integers(0, V, E, dtype=np.int64)
    hub = 7
    dst[rng.random(E) < 0.12] = hub
    dst[rng.random(E) < 0.02] = -1  # null entries of records that also hold links
    loops = rng.integers(0, V, 300)
    dup = rng.integers(0, E, 2000)
    src = np.concatenate([src, loops, src[dup]])
    dst = np.concatenate([dst, loops, dst[dup]])
    sinks = np.array([4321, 17017])
    keep = ~np.isin(src, sinks)
    src, dst = src[keep], dst[keep]
    src = np.concatenate([src, [11, 12, 13]])  # the sinks are targets
    dst = np.concatenate([dst, [sinks[0], sinks[1], sinks[1]]])
    nolink = rng.permutation(V)[:V // 20]
    nolink = nolink[~np.isin(nolink, np.concatenate([sinks, [11, 12, 13]]))]  # records that hold only null
    keep = ~np.isin(src, nolink)
    src, dst = np.concatenate([src[keep], nolink]), np.concatenate([dst[keep], np.full(nolink.shape, -1)])
    is_key = np.zeros(V, bool)
    is_key[src] = True
    is_key[sinks] = True
    miss = np.nonzero(~is_key)[0]  # every other vertex is a source
    src = np.concatenate([src, miss])
    dst = np.concatenate([dst, rng.integers(0, V, miss.size)])
    return OneStepInput(V, src.astype(np.int32), dst.astype(np.int32), sinks, hub)
