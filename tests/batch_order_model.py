"""An order-exact model of one batched PageRank iteration (csrc/pr_batch.hip), and the inputs whose
rows sit on its unit, chunk and grid boundaries.  Pure numpy; tests/test_batch_order_model_cpu.py
proves the claims made here without a GPU, tests/test_gpu_batch_boundaries.py runs the kernels
against the model, bit for bit.

The model follows csrc/pr_batch.h: "the order of a row's sum is a function of the row's length and
the stride alone".  With G = 64 / stride lane groups and cap = 64 G in-links per unit, for a row
whose in-links are x_0 .. x_(n-1) in col_idx order:

  n == 0         S = the row's old rank
  1 <= n <= 8    ((0.0 + x_0) + x_1) + ...                       (one lane group, in-link order)
  8 < n <= cap   group g: ((0.0 + x_g) + x_(g+G)) + ...; the G group sums are combined by the
                 pairwise tree (0,1),(2,3),... level by level -- the butterfly over the lane
                 offsets stride, 2 stride, ..., 32; addition commutes, so every lane has these bits
  n > cap        chunks of cap consecutive in-links, the last one shorter; every chunk, whatever
                 its length, is summed like a row of 8 < n <= cap; the chunk sums are added to
                 +0.0 in chunk order

and then r' = t + damping * (S + dc / N), every operation rounded to float64 on its own, with
c = r / out_deg (out_deg > 0) as the contribution a vertex sends along each out-link.

Every sum below is written as separate element-wise numpy operations: numpy rounds each one to
float64 and never contracts two of them.  Two shortcuts are used, both exact:
* a group (or a step of a group) that holds no in-link adds +0.0.  A running sum that started at
  +0.0 is never -0.0 under round-to-nearest (x + -x and +0.0 + -0.0 are both +0.0), so adding +0.0
  returns it unchanged;
* a row of n < G in-links leaves the groups n .. G-1 at +0.0; whole subtrees of the combine are then
  +0.0 and add nothing, so the tree is evaluated over the next power of two >= n groups only.
row_sum_lanes() is the deliberately slow form without either shortcut: 64 lanes, the kernel's loop
and the xor shuffles.
"""
import math

import numpy as np

WAVE = 64
STEPS = 64       # pr_batch.h kBatchSteps
UNIT_ROWS = 64   # kBatchUnitRows
SHORT_ROW = 8    # kBatchShortRow
GRID_MAX = 8192  # pr_batch.hip kBatchGridMax
STRIDES = (1, 2, 4, 8, 16)
VF_KEY, VF_SINK, VF_NOLINK, VF_INDEG0 = 1, 2, 4, 8


def stride_of(width):
    s = 1
    while s < width:
        s <<= 1
    return s


def groups(stride):
    return WAVE // stride


def unit_cap(stride):
    return groups(stride) * STEPS


def _pow2_ceil(n):
    p = 1
    while p < n:
        p <<= 1
    return p


# ---- the row sum ---------------------------------------------------------------------------------
def row_sum_lanes(x, stride):
    """k_batch_units' row_sum<S> lane by lane.  x is float64[n, stride]: column j of in-link i.
    Returns float64[64]: what every lane holds after the butterfly (lane = g * stride + j)."""
    S, G = stride, groups(stride)
    n = x.shape[0]
    acc = np.zeros(WAVE)
    for lane in range(WAVE):
        g, j = lane // S, lane % S
        a = np.float64(0.0)
        i = g
        while i + 3 * G < n:  # four gathers in flight, added in order
            a = a + x[i, j]
            a = a + x[i + G, j]
            a = a + x[i + 2 * G, j]
            a = a + x[i + 3 * G, j]
            i += 4 * G
        while i < n:
            a = a + x[i, j]
            i += G
        acc[lane] = a
    off = S
    while off < WAVE:
        other = acc[np.arange(WAVE) ^ off]
        acc = acc + other
        off <<= 1
    return acc


def _index_matrix(begin, n):
    return begin[:, None] + np.arange(n, dtype=np.int64)[None, :]


def _sum_in_order(vals):
    """vals float64[m, n]: ((0.0 + v_0) + v_1) + ... per line."""
    acc = np.zeros(vals.shape[0])
    for q in range(vals.shape[1]):
        acc = acc + vals[:, q]
    return acc


def _sum_grouped(vals, G):
    """vals float64[m, n]: row_sum's order per line -- G strided group sums, then the pairwise tree."""
    m, n = vals.shape
    steps = -(-n // G)
    width = min(G, _pow2_ceil(n))  # the groups past it hold +0.0
    if steps * G != n:
        padded = np.zeros((m, steps * G))
        padded[:, :n] = vals
        vals = padded
    vals = vals.reshape(m, steps, G)
    acc = np.zeros((m, width))
    for s in range(steps):
        acc = acc + vals[:, s, :width]
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def row_sum_vec(x, stride):
    """The vectorised row sum of one row or chunk of any length >= 1 (x float64[n]), in row_sum's order."""
    return float(_sum_grouped(np.asarray(x, np.float64)[None, :], groups(stride))[0])


# ---- the plan ------------------------------------------------------------------------------------
def chunk_ranges(deg, cap):
    """(begin within the row, length) of every chunk of a row of deg > cap in-links."""
    return [(k * cap, min(cap, deg - k * cap)) for k in range(-(-deg // cap))]


def plan_units(row_ptr, stride):
    """pr_batch.h batch_plan restated: a list of (e0, row0, rows, n, slot); rows < 0: chunk -(k + 1).
    A plain loop over the rows: for the small graphs only."""
    cap = unit_cap(stride)
    rp = [int(x) for x in row_ptr]
    units, cur, slots = [], None, 0
    for v in range(len(rp) - 1):
        b, deg = rp[v], rp[v + 1] - rp[v]
        if deg > cap:
            if cur:
                units.append(tuple(cur))
                cur = None
            for k, (cb, cn) in enumerate(chunk_ranges(deg, cap)):
                units.append((b + cb, v, -(k + 1), cn, slots))
                slots += 1
            continue
        if cur and not (cur[2] < UNIT_ROWS and cur[3] + deg <= cap):
            units.append(tuple(cur))
            cur = None
        if cur is None:
            cur = [b, v, 0, 0, 0]
        cur[2] += 1
        cur[3] += deg
    if cur:
        units.append(tuple(cur))
    return units


class BatchModel:
    """One column's iteration over a canonical CSR (rows = dst, columns = src) at one stride."""

    def __init__(self, csr, stride, dangling_none=False):
        self.stride, self.G, self.cap = stride, groups(stride), unit_cap(stride)
        self.V = len(csr.out_deg)
        self.row_ptr = np.asarray(csr.row_ptr, np.int64)
        self.col = np.asarray(csr.col_idx, np.int64)
        self.deg = np.asarray(csr.out_deg, np.float64)
        self.has_out = self.deg > 0
        self.indeg = np.diff(self.row_ptr)
        self.sink = ((np.asarray(csr.vflags) & VF_SINK) != 0) & (not dangling_none)
        begin = self.row_ptr[:-1]
        self.short, self.grouped = [], []  # (rows, index matrix into col) per row length
        for n in np.unique(self.indeg):
            n = int(n)
            if n == 0 or n > self.cap:
                continue
            rows = np.nonzero(self.indeg == n)[0]
            (self.short if n <= SHORT_ROW else self.grouped).append((rows, _index_matrix(begin[rows], n)))
        self.long_rows = np.nonzero(self.indeg > self.cap)[0]
        self.chunks = []  # per long row: [(first in-link, length)] in chunk order
        for v in self.long_rows:
            b = int(begin[v])
            self.chunks.append([(b + cb, cn) for cb, cn in chunk_ranges(int(self.indeg[v]), self.cap)])

    def kinds(self):
        """Per row: 0 empty, 1 one lane group in order, 2 row_sum in a PACK unit, 3 chunks."""
        k = np.zeros(self.V, np.int8)
        k[self.indeg > 0] = 1
        k[self.indeg > SHORT_ROW] = 2
        k[self.indeg > self.cap] = 3
        return k

    def contributions(self, r):
        c = np.zeros(self.V)
        c[self.has_out] = r[self.has_out] / self.deg[self.has_out]
        return c

    def row_sums(self, r):
        """S per row from the previous ranks r, in the kernels' order."""
        x = self.contributions(r)[self.col]  # per in-link, col_idx order
        S = np.array(r, np.float64)  # an empty row keeps its old rank
        for rows, idx in self.short:
            S[rows] = _sum_in_order(x[idx])
        for rows, idx in self.grouped:
            S[rows] = _sum_grouped(x[idx], self.G)
        for v, chunks in zip(self.long_rows, self.chunks):
            acc = np.float64(0.0)
            for b, n in chunks:
                part = _sum_grouped(x[None, b:b + n], self.G)[0]
                acc = acc + part
            S[v] = acc
        return S

    def step(self, r, t, dc, damping=0.85):
        """The new ranks of one column: r previous ranks, t teleport terms, dc the dangling sum used."""
        S = self.row_sums(np.asarray(r, np.float64))
        tdc = np.float64(dc) / np.float64(self.V)
        inner = S + tdc
        scaled = np.float64(damping) * inner
        return t + scaled

    def exact_row_sum(self, r, v):
        """math.fsum of row v's contributions (an empty row: its old rank): the correctly rounded sum."""
        b, e = int(self.row_ptr[v]), int(self.row_ptr[v + 1])
        if b == e:
            return float(r[v])
        return math.fsum(self.contributions(r)[self.col[b:e]].tolist())

    def abs_row_sum(self, r, v):
        b, e = int(self.row_ptr[v]), int(self.row_ptr[v + 1])
        return math.fsum(np.abs(self.contributions(r)[self.col[b:e]]).tolist()) if e > b else abs(float(r[v]))


# ---- inputs --------------------------------------------------------------------------------------
LONG = 8193  # more than the capacity of every stride (4096 at stride 1)
CAPS = tuple(unit_cap(s) for s in STRIDES)  # 4096 .. 256
FILLER = (1, 0, 3, 2, 0, 1, 12, 5, 0, 0, 9, 1, 8, 2, 1, 17)


def _edges(indeg, no_source, nolink):
    """An edge list with the prescribed in-degrees.  The sources of all in-links, in row order, sweep
    the vertices outside `no_source` cyclically, so a row's sources are distinct while it has no more
    in-links than there are such vertices, and every one of them is a source once the edges outnumber
    them.  `nolink` vertices also get a (v, -1) record."""
    V = len(indeg)
    pool = np.setdiff1d(np.arange(V, dtype=np.int64), np.asarray(no_source, np.int64))
    E = int(indeg.sum())
    assert int(indeg.max()) <= len(pool) <= E
    dst = np.repeat(np.arange(V, dtype=np.int64), indeg)
    src = pool[np.arange(E, dtype=np.int64) % len(pool)]
    src = np.concatenate([src, np.asarray(nolink, np.int64)])
    dst = np.concatenate([dst, np.full(len(nolink), -1, np.int64)])
    return src.astype(np.int32), dst.astype(np.int32)


def boundary_graph():
    """Returns (V, src, dst, plan).  One graph for every stride; plan = dict(indeg[V], and row numbers:
    rows_a / rows_b / rows_c (lists of (row, in-degree)), unit64_row0, empty_unit_row0,
    full_unit_row0 {cap: row}, long_rows (of LONG in-links), sinks, nolinks, indeg0_keys)."""
    deg, plan = [], dict(rows_a=[], rows_b=[], rows_c=[], full_unit_row0={}, long_rows=[])

    def add(d, to=None):
        if to is not None:
            plan[to].append((len(deg), d))
        if d == LONG:
            plan["long_rows"].append(len(deg))
        deg.append(d)

    add(LONG)  # g) a long row at row 0
    for d in (0, 1, 2, 7, 8, 9, 10):  # a)
        add(d, "rows_a")
    for s in STRIDES:  # b)
        G = groups(s)
        for m in (1, 4, 8):
            for d in (m * G - 1, m * G, m * G + 1):
                add(d, "rows_b")
    for cap in CAPS:  # c)
        for d in (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1):
            add(d, "rows_c")
    filler0 = len(deg)
    for i in range(13_700):
        add(FILLER[i % len(FILLER)])
    filler1 = len(deg)
    add(LONG)
    plan["unit64_row0"] = len(deg)  # d) [0, 1 x 62, 0] between two long rows
    for d in [0] + [1] * 62 + [0]:
        add(d)
    add(LONG)
    plan["empty_unit_row0"] = len(deg)  # e) two empty rows between two long rows
    add(0)
    add(0)
    add(LONG)
    for cap in sorted(CAPS):  # f) just after a long row: [cap / 2, cap / 2] closes at n == cap, then a row of 1
        plan["full_unit_row0"][cap] = len(deg)
        add(cap // 2)
        add(cap // 2)
        add(1)
        add(LONG)
    add(LONG)  # g) two adjacent long rows, the second at row V - 1
    indeg = np.array(deg, np.int64)
    V = len(indeg)
    u64, e0 = plan["unit64_row0"], plan["empty_unit_row0"]
    filler = np.arange(filler0, filler1)
    nonempty = filler[indeg[filler] > 0]
    # h) SINK: in-links and never a source -- rows of 1, 2, 9 and 10 in-links, of cap + 1 in-links
    # (a CHUNK row at one stride, a PACK row at the others), a LONG row, a row inside the 64-row unit,
    # and every 11th non-empty filler row
    by_deg = {d: r for r, d in plan["rows_a"] + plan["rows_c"]}
    sinks = [by_deg[1], by_deg[2], by_deg[9], by_deg[10], by_deg[257], by_deg[4097], plan["long_rows"][2], u64 + 5]
    sinks += nonempty[::11].tolist()
    # (v, -1) records: the first row of the 64-row unit and of the empty unit (no in-link either), and
    # every 13th non-empty filler row that is no sink (in-links, no out-link, but a key: no dangling mass)
    nolinks = [u64, e0] + [int(v) for v in nonempty[5::13] if int(v) not in set(sinks)]
    plan["sinks"], plan["nolinks"] = sorted(sinks), sorted(nolinks)
    # the other empty rows are sources: keys without an in-link
    plan["indeg0_keys"] = sorted(set(np.nonzero(indeg == 0)[0].tolist()) - set(nolinks))
    plan["indeg"] = indeg
    src, dst = _edges(indeg, plan["sinks"] + plan["nolinks"], plan["nolinks"])
    return V, src, dst, plan


MANY_V = 655_000
MANY_CYCLE = (1, 0, 9, 2)
MANY_HUBS = ((0, 4097), (MANY_V // 2, 9000), (MANY_V - 1, 300))


def many_units_graph():
    """Returns (V, src, dst, plan): in-degrees cycling through (1, 0, 9, 2), three hubs, a sink set.
    64 rows of the cycle hold 192 in-links, below every stride's capacity, so the row limit closes the
    units and n_units ~ V / 64 + the hubs' chunks: more than the 8192 waves of k_batch_units' grid."""
    V = MANY_V
    indeg = np.tile(np.array(MANY_CYCLE, np.int64), V // len(MANY_CYCLE) + 1)[:V]
    for row, d in MANY_HUBS:
        indeg[row] = d
    nonempty = np.nonzero(indeg > 0)[0]
    sinks = sorted(set(nonempty[::97].tolist()) | {MANY_HUBS[1][0]})
    src, dst = _edges(indeg, sinks, [])
    return V, src, dst, dict(indeg=indeg, sinks=sinks)


def teleport_columns(V, width, seed):
    """One teleport vector per column, by j % 4: 0 dense with negative entries (the ranks change sign
    and the row sums cancel), 1 sparse with rest = 0.0 as (ids, values), 2 scalar (None), 3 dense and
    positive.  Returns (specs, terms): what to set on the batch, and the float64[V] term vectors."""
    rng = np.random.default_rng(seed)
    specs, terms = [], []
    for j in range(width):
        kind = j % 4
        if kind == 0:
            t = rng.uniform(-2.0, 2.0, V)
            specs.append(("dense", t))
        elif kind == 1:
            ids = rng.permutation(V)[:max(1, V // 50)].astype(np.int32)
            values = rng.uniform(0.5, 40.0, len(ids))
            t = np.zeros(V)
            t[ids] = values
            specs.append(("sparse", ids, values))
        elif kind == 2:
            t = np.full(V, 0.15)
            specs.append(("scalar",))
        else:
            t = rng.uniform(0.01, 0.3, V)
            specs.append(("dense", t))
        t.setflags(write=False)
        terms.append(t)
    return specs, terms
