"""pr_batch_reset_column, pr_batch_step_until_any and pr_batch_run_queue on the GPU, through
PageRankBatch.reset_column / step_until_any / run_queue.

Reference: tests/test_gpu_batch_until.py's numpy Reference over export_csr(), re-stated -- c = r /
out_deg where out_deg > 0, S[v] = sum of c over the row's columns (S[v] = r_old[v] for an empty
row), dc = sum of r over the PR_VF_SINK vertices, r' = t + 0.85 (S + dc / N); a run stops after the
first iteration whose L1 delta is <= TOL.  Bound on the ranks: |got - want| <= 1e-9 max(1, |want|).
Iteration counts must match the reference exactly; so that this is a fair demand the reference's own
L1 is asserted to stay more than 1e-6 (relative) away from TOL on both sides of every crossing (and,
for a run that hits the cap, above TOL by that margin in its last iteration).  Where two runs must
agree exactly they are compared as uint64 views.

Graphs, as in tests/test_gpu_batch_until.py: the 6-vertex KAT; V = 300 / E = 2500 (PACK units with
short and medium rows); V = 6000 / E = 60000 with 30 % of the links at vertex 0 (CHUNK units and
k_batch_long at every stride).

The queue's queries (make_queries) are sparse vectors of one to three seeds whose masses span two and a
half decades around the V that the initial ranks hold, a quarter of them with rest != 0, so that their
iteration counts spread (91 .. 153 on the two random graphs); query 1 carries a mass of 1e12 V and
does not converge within MAXIT."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KAT = ["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"]  # tests/test_cli_gpu.py
PR_VF_SINK = 2
WIDTHS = [1, 3, 8, 16]
TOL = 1e-6
CAP = 400    # of the step_until / step_until_any tests: never reached
MAXIT = 200  # of the queue: query 1 hits it
N_QUERIES = 40


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def random_edges(rng, V, E, hub_frac=0.0):
    src = rng.integers(0, V, E, dtype=np.int64)
    dst = rng.integers(0, V, E, dtype=np.int64)
    if hub_frac > 0:
        dst[rng.random(E) < hub_frac] = 0
    dst[rng.random(E) < 0.05] = -1
    seen = np.zeros(V, bool)  # every ID appears: one record per missing vertex
    seen[src] = True
    seen[dst[dst >= 0]] = True
    miss = np.nonzero(~seen)[0]
    src = np.concatenate([src, miss])
    dst = np.concatenate([dst, np.full(miss.shape, -1)])
    return src.astype(np.int32), dst.astype(np.int32)


def graph_edges(name):
    """(V, src, dst) of the three graphs."""
    if name == "kat":
        from sparky_hip.driver import read_edge_list

        urls, src, dst = read_edge_list(KAT)
        return len(urls), src, dst
    if name == "pack":
        return (300,) + random_edges(np.random.default_rng(7), 300, 2500)
    return (6000,) + random_edges(np.random.default_rng(11), 6000, 60000, hub_frac=0.3)


class Reference:
    """The iteration in numpy over a canonical CSR (rows = dst, columns = src)."""

    def __init__(self, csr):
        self.V = len(csr.out_deg)
        self.deg = csr.out_deg.astype(np.float64)
        self.col = csr.col_idx.astype(np.int64)
        self.row = np.repeat(np.arange(self.V), np.diff(csr.row_ptr))
        self.empty = np.diff(csr.row_ptr) == 0
        self.sink = (csr.vflags & PR_VF_SINK) != 0
        self._until = {}

    def dc(self, r):
        return float(np.sum(r[self.sink]))

    def step(self, r, t, damping=0.85):
        c = np.zeros(self.V)
        nz = self.deg > 0
        c[nz] = r[nz] / self.deg[nz]
        S = np.bincount(self.row, weights=c[self.col], minlength=self.V)
        S[self.empty] = r[self.empty]
        return t + damping * (S + self.dc(r) / self.V)

    def until(self, key, t, cap=CAP, may_hit_cap=False):
        """(n, ranks after n iterations, converged): the first n <= cap whose L1 delta is <= TOL.
        Computed once per teleport vector (`key`) and shared, read-only.  Asserts that no crossing is
        borderline: the L1 of iteration n and that of iteration n - 1 (for a run that stops at the
        cap: that of iteration cap) are more than 1e-6 (relative) away from TOL."""
        if key not in self._until:
            r, before = np.ones(self.V), np.inf
            for n in range(1, cap + 1):
                new = self.step(r, t)
                l1 = float(np.abs(new - r).sum())
                r = new
                if l1 <= TOL:
                    break
                before = l1
            conv = l1 <= TOL
            assert conv or may_hit_cap, f"vector {key}: the reference needs more than {cap} iterations"
            if conv:
                assert (TOL - l1) / TOL > 1e-6 and (before - TOL) / TOL > 1e-6, (key, n, l1, before)
            else:
                assert (l1 - TOL) / TOL > 1e-6, (key, n, l1)
            r.setflags(write=False)
            self._until[key] = (n, r, conv)
        return self._until[key]


def assert_close(got, want):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-9, f"max error {err.max():.3e} at index {int(err.argmax())}"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def vectors(V, width):
    """tests/test_gpu_batch_until.py's staggered teleport vectors: columns j % 3 == 0 put the mass
    0.15 * 10^(j // 3) on the single seed (7 j + 1) % V, the others are dense; the last column of a
    batch wider than 1 stays scalar (None)."""
    ts = []
    for j in range(width):
        if j % 3 == 0:
            t = np.zeros(V)
            t[(7 * j + 1) % V] = 0.15 * 10.0 ** (j // 3)
        else:
            t = 0.02 * (j + 1) + 1e-4 * ((np.arange(V) * (2 * j + 1)) % V)
        ts.append(t)
    if width > 1:
        ts[-1] = None
    return ts


def term(t, V):
    return np.full(V, 0.15) if t is None else t


def make_queries(V, n=N_QUERIES, seed=3):
    """(ids, values, rest) per query, from a fixed RNG.  The seed is one for which the reference's L1
    stays more than 2e-3 (relative) from TOL at every crossing on all three graphs -- a thousand
    times the margin Reference.until asserts, and well above the rounding noise of an L1 over ranks
    that sum to at most 32 V."""
    rng = np.random.default_rng(seed)
    qs = []
    for q in range(n):
        k = int(rng.integers(1, min(3, V) + 1))
        ids = rng.choice(V, k, replace=False).astype(np.int32)
        mass = 0.15 * V * 10.0 ** rng.uniform(-1.0, 1.5)  # against the V that the initial ranks hold
        values = mass * (1.0 + np.arange(k)) / k
        qs.append((ids, values, (0.0, 0.0, 0.0, 1e-3)[q % 4]))
    qs[1] = (np.array([V // 2], np.int32), np.array([1e12 * V]), 0.0)  # hits MAXIT
    return qs


def dense(q, V):
    t = np.full(V, float(q[2]))
    t[q[0]] = q[1]
    return t


def model(need, width, cap):
    """tests/test_batch_queue_cpu.py's schedule model: need[q] is the iteration in which query q
    converges (> cap: never).  Returns (column per query, completion order)."""
    Q = len(need)
    slot, age, nxt = [None] * width, [0] * width, 0
    col, order = [None] * Q, []
    while len(order) < Q:
        for j in range(width):
            if slot[j] is None and nxt < Q:
                slot[j], age[j], col[nxt] = nxt, 0, j
                nxt += 1
        occ = [j for j in range(width) if slot[j] is not None]
        n = min(min(cap - age[j] for j in occ), min(need[slot[j]] - age[j] for j in occ))
        for j in occ:
            age[j] += n
            if age[j] == need[slot[j]] or age[j] >= cap:
                order.append(slot[j])
                slot[j] = None
    return col, order


def new_batch(hip, g, ts, init=None):
    b = hip.PageRankBatch(g, len(ts))
    for j, t in enumerate(ts):
        if t is not None:
            b.set_teleport(j, t)
    b.reset(init_ranks=init)
    return b


def snapshot(b):
    """Per column the rank bits, and the (dc, l1) bits."""
    d, l = b.norms()
    return [bits(b.ranks(j)).copy() for j in range(b.width)], bits(d).copy(), bits(l).copy()


def same_column(a, b, j, jb=None):
    """Column j of snapshot a against column jb (default j) of snapshot b: ranks and both norms."""
    jb = j if jb is None else jb
    return np.array_equal(a[0][j], b[0][jb]) and a[1][j] == b[1][jb] and a[2][j] == b[2][jb]


class Case:
    def __init__(self, hip, g, name):
        self.hip, self.g, self.name, self.ref = hip, g, name, Reference(g.export_csr())
        self.V = self.ref.V
        self.queries = make_queries(self.V)
        self._solo = {}

    def want(self, q):
        """(iterations, reference ranks, converged) of query q."""
        return self.ref.until(("q", q), dense(self.queries[q], self.V), cap=MAXIT, may_hit_cap=True)

    def solo(self, width, q, k, exclude=None):
        """Query q alone in column 0 of a fresh batch of `width`, stepped by its reference count:
        (rank bits, top-k ids, top-k rank bits)."""
        key = (width, q, k, None if exclude is None else tuple(exclude))
        if key not in self._solo:
            n = self.want(q)[0]
            with self.hip.PageRankBatch(self.g, width) as b:
                ids, values, rest = self.queries[q]
                b.set_teleport_sparse(0, ids, values, rest)
                if exclude is not None:
                    b.set_exclude(0, exclude)
                b.reset()
                b.step(n)
                ti, tr = b.topk(0, k)
                self._solo[key] = (bits(b.ranks(0)).copy(), ti.copy(), bits(tr).copy())
        return self._solo[key]

    def staggered(self, width):
        """(ts, counts) of the staggered batch; from width 3 on columns 0 and 1 hold the same vector."""
        ts = vectors(self.V, width)
        if width >= 3:
            ts[1] = ts[0].copy()
        keys = ["scalar" if t is None else ("v", 0 if (width >= 3 and j == 1) else j) for j, t in enumerate(ts)]
        counts = np.array([self.ref.until(k, term(t, self.V))[0] for k, t in zip(keys, ts)], np.int32)
        return ts, counts


@pytest.fixture(scope="module", params=["kat", "pack", "hub"])
def case(hip, request):
    V, src, dst = graph_edges(request.param)
    with hip.PageRankGraph(V, src, dst) as g:
        if request.param == "hub":
            with hip.PageRankBatch(g, 16) as b:
                assert b.info()["n_long_rows"] >= 1  # CHUNK units and k_batch_long run
        yield Case(hip, g, request.param)


# ---- 1: reset_column -----------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_reset_column(hip, case, width):
    ts, counts = case.staggered(width)
    mid = width // 2
    und = {}  # the undisturbed batch after 4, 5, 8 and 9 steps
    with new_batch(hip, case.g, ts) as u:
        done = 0
        for n in (4, 5, 8, 9):
            u.step(n - done)
            done = n
            und[n] = snapshot(u)
    with new_batch(hip, case.g, ts) as b2:  # step_until, then 4 steps, never disturbed
        assert np.array_equal(b2.step_until(CAP, TOL), counts)
        und["until"] = snapshot(b2)
        b2.step(4)
        und["until+4"] = snapshot(b2)
    rnd = 0.5 + np.random.default_rng(3).random(case.V)
    for init in (None, rnd):
        with new_batch(hip, case.g, ts, init=init) as f:  # the fresh batch the column must equal
            f0 = snapshot(f)
            f.step(4)
            f4 = snapshot(f)
        want_dc = case.ref.dc(np.ones(case.V) if init is None else init)
        assert_close(f0[1].view(np.float64)[mid], want_dc)
        assert f0[2][mid] == 0  # an L1 of +0.0
        for before in (5, 4, "until"):  # odd parity, even parity, columns at different counts
            with new_batch(hip, case.g, ts) as b:
                if before == "until":
                    b.step_until(CAP, TOL)
                else:
                    b.step(before)
                iters0 = b.info()["iters"]
                b.reset_column(mid, init)
                assert b.info()["iters"] == iters0
                s = snapshot(b)
                assert same_column(s, f0, mid), (before, "the column after reset_column")
                for j in range(width):
                    if j != mid:
                        assert same_column(s, und[before], j), (before, j, "another column, right after")
                b.step(4)
                s = snapshot(b)
                assert same_column(s, f4, mid), (before, "the column 4 steps later")
                after = "until+4" if before == "until" else before + 4
                for j in range(width):
                    if j != mid:
                        assert same_column(s, und[after], j), (before, j, "another column, 4 steps later")


def test_reset_column_then_frozen(hip, case):
    """A column restarted at odd parity and frozen in the very next iterations keeps both of its
    buffers valid: whenever it is released it continues like the fresh batch."""
    width = 3
    ts, _ = case.staggered(width)
    with new_batch(hip, case.g, ts) as f:
        f0 = snapshot(f)
        f.step(3)
        f3 = snapshot(f)
    for frozen_for in (1, 2):
        with new_batch(hip, case.g, ts) as b:
            b.step(5)
            b.reset_column(1)
            assert b.step_until_any(0b101, frozen_for, TOL) == (frozen_for, 0)  # column 1 outside the mask
            assert same_column(snapshot(b), f0, 1)
            b.step(3)
            assert same_column(snapshot(b), f3, 1)


@pytest.mark.parametrize("steps", [5, 4])
def test_frozen_column_keeps_norms_after_step(hip, case, steps):
    """step_until_any right after step(): a column outside the mask that was never restarted keeps
    its ranks and the norms of its last iteration (the dc that iteration used, at either parity)."""
    ts, counts = case.staggered(3)
    assert counts.min() > steps + 3
    with new_batch(hip, case.g, ts) as u:
        u.step(steps)
        und = snapshot(u)
        u.step(3)
        und3 = snapshot(u)
    with new_batch(hip, case.g, ts) as b:
        b.step(steps)
        assert b.step_until_any(0b011, 3, TOL) == (3, 0)
        s = snapshot(b)
        assert same_column(s, und, 2)
        assert same_column(s, und3, 0) and same_column(s, und3, 1)


# ---- 2: step_until_any ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_step_until_any(hip, case, width):
    ts, counts = case.staggered(width)
    # from width 8 on one column stays outside `active` throughout (at width 3 that would leave only
    # the identical pair; test_reset_column_then_frozen freezes a column at that width)
    frozen = 2 if width >= 8 else None
    act = [j for j in range(width) if j != frozen]
    stages = sorted(set(int(counts[j]) for j in act))
    if width >= 3:
        assert counts[0] == counts[1] and len(stages) >= 2, counts
    fixed = {}
    with new_batch(hip, case.g, ts) as f:
        start = snapshot(f)
        done = 0
        for n in sorted(set(stages + [5])):
            f.step(n - done)
            done = n
            fixed[n] = snapshot(f)
    with new_batch(hip, case.g, ts) as b:
        assert b.step_until_any(0, 10, TOL) == (0, 0) and b.step_until_any(0b1, 0, TOL) == (0, 0)  # no-ops
        s = snapshot(b)
        assert all(same_column(s, start, j) for j in range(width)) and b.info()["iters"] == 0
        mask, total = sum(1 << j for j in act), 0
        for n in stages:
            executed, conv = b.step_until_any(mask, CAP, TOL)
            want = sum(1 << j for j in act if counts[j] == n)
            assert (executed, conv) == (n - total, want), (n, executed, bin(conv), bin(want))
            total = n
            s = snapshot(b)
            for j in act:
                if (mask >> j) & 1:  # active in this call: where step(n) leaves it
                    assert same_column(s, fixed[n], j), (n, j)
                else:  # converged in an earlier call: frozen there
                    assert same_column(s, fixed[int(counts[j])], j), (n, j)
            if frozen is not None:
                assert same_column(s, start, frozen), n
            assert b.info()["iters"] == n
            mask &= ~conv
        assert mask == 0
    with new_batch(hip, case.g, ts) as b:  # the cap: nothing converges within 5
        assert stages[0] > 5
        mask = sum(1 << j for j in act)
        assert b.step_until_any(mask, 5, TOL) == (5, 0)
        s = snapshot(b)
        assert all(same_column(s, fixed[5], j) for j in act)
        if frozen is not None:
            assert same_column(s, start, frozen)


@pytest.mark.parametrize("width", [3, 16])
def test_step_until_any_block_independence(hip, case, width):
    ts, counts = case.staggered(width)
    first = int(counts.min())
    assert first % 32 != 0  # so that a block of 32 enqueues more than it executes
    want = sum(1 << j for j in range(width) if counts[j] == first)
    snaps = []
    for block in (1, 3, 32):
        with new_batch(hip, case.g, ts) as b:
            executed, conv, (enq, ex) = b._step_until_any_ex((1 << width) - 1, CAP, TOL, block)
            assert (executed, conv, ex) == (first, want, first)
            assert enq == -(-first // block) * block
            if block == 32:
                assert enq > ex
            snaps.append(snapshot(b))
            b.step(2)  # the mask word is restored: the batch goes on as usual
            snaps.append(snapshot(b))
    for s in snaps[2::2]:
        assert all(same_column(s, snaps[0], j) for j in range(width))
    for s in snaps[3::2]:
        assert all(same_column(s, snaps[1], j) for j in range(width))


# ---- 3: run_queue --------------------------------------------------------------------------------
def run_and_check(case, width, order, k):
    """The queries `order` (indices into case.queries) through a batch of `width`: every check of a
    single run.  Returns per query (rank bits, record)."""
    qs = [case.queries[q] for q in order]
    got = {}
    with case.hip.PageRankBatch(case.g, width) as b:
        b.reset()
        calls = []

        def on_done(i, column, rec):
            calls.append(i)
            got[order[i]] = (bits(b.ranks(column)).copy(), rec)

        recs = b.run_queue(qs, MAXIT, TOL, k=k, on_done=on_done)
        b.step(1)  # an ordinary state afterwards
    need = []
    for i, q in enumerate(order):
        n, ranks, conv = case.want(q)
        rec = recs[i]
        assert (rec["iterations"], rec["converged"]) == (n, conv), (q, rec, n, conv)
        assert (rec["l1"] <= TOL) == conv
        assert_close(got[q][0].view(np.float64), ranks)
        sb, si, sr = case.solo(width, q, k)
        assert np.array_equal(got[q][0], sb), q  # bitwise the solo run
        assert np.array_equal(rec["topk"][0], si) and np.array_equal(bits(rec["topk"][1]), sr), q
        need.append(n if conv else MAXIT + 1)
    col, done_order = model(need, width, MAXIT)
    assert [r["column"] for r in recs] == col
    assert calls == done_order
    return got


@pytest.mark.parametrize("Q,width", [(40, 16), (7, 3), (5, 1), (2, 8)])
def test_run_queue(hip, case, Q, width):
    k = min(case.V, 10)
    fwd = run_and_check(case, width, list(range(Q)), k)
    assert not case.want(1)[2]  # query 1 hits MAXIT (on the slowly converging KAT others do, too)
    if Q >= 7:  # others converge, at counts that spread
        assert len(set(case.want(q)[0] for q in range(Q) if case.want(q)[2])) >= 2
    rev = run_and_check(case, width, list(range(Q))[::-1], k)
    for q in range(Q):
        assert np.array_equal(fwd[q][0], rev[q][0]), q
        assert fwd[q][1]["iterations"] == rev[q][1]["iterations"]


def test_run_queue_without_callback(hip, case):
    """done == NULL: the queue runs all the same; with as many queries as columns every column is left
    holding its query's result."""
    import ctypes

    from sparky_hip import _lib

    order = [0, 2, 3]
    keep = [(np.ascontiguousarray(i), np.ascontiguousarray(v)) for i, v, _ in (case.queries[q] for q in order)]
    arr = (_lib.BatchQuery * 3)()
    for n, (i, v) in enumerate(keep):
        arr[n] = _lib.BatchQuery(len(i), i.ctypes.data, v.ctypes.data, float(case.queries[order[n]][2]), 0, None)
    with hip.PageRankBatch(case.g, 3) as b:
        b.reset()
        rc = _lib.load().pr_batch_run_queue(b._h, 3, ctypes.cast(arr, ctypes.c_void_p), MAXIT, TOL, None, None, None)
        assert rc == _lib.PR_OK
        assert b.info()["iters"] == max(case.want(q)[0] for q in order)
        for j, q in enumerate(order):
            assert np.array_equal(bits(b.ranks(j)), case.solo(3, q, min(case.V, 10))[0]), q


def test_run_queue_exclusions(hip, case):
    """Every list leaves out exactly its own query's set -- also when the query before it in the same
    column had another set, or the query itself has none."""
    V, width, Q = case.V, 3, 7
    rng = np.random.default_rng(9)
    qs, sets = [], []
    for q in range(Q):
        ids, values, rest = case.queries[q if q != 1 else Q]  # without the query that hits MAXIT
        ex = np.zeros(0, np.int32) if q % 3 == 2 else np.union1d(ids, rng.choice(V, min(2, V), replace=False)).astype(np.int32)
        qs.append((ids, values, rest, ex))
        sets.append(set(ex.tolist()))
    with hip.PageRankBatch(case.g, width) as b:
        b.reset()
        recs = b.run_queue(qs, MAXIT, TOL, k=V)
        cols = [r["column"] for r in recs]
        assert len(set(cols)) == width and len(cols) > width  # columns are reused
        for q, rec in enumerate(recs):
            ids, ranks = rec["topk"]
            assert set(ids.tolist()) == set(range(V)) - sets[q], q
            assert len(ids) == V - len(sets[q])
            assert np.all(np.diff(ranks) <= 0)
        # afterwards a column keeps the set of the last query it served
        last = {c: q for q, c in enumerate(cols)}
        for c, q in last.items():
            assert set(b.topk(c, V)[0].tolist()) == set(range(V)) - sets[q]


# ---- 4: the sparse teleport vector, set on the device ---------------------------------------------
@pytest.mark.parametrize("width", [3, 16])
def test_sparse_teleport_on_device(hip, case, width):
    """With damping 0 an iteration leaves r = t + 0 * (...) = t: the ranks read T back."""
    V = case.V
    qs = case.queries[:2 * width + 2]
    with hip.PageRankBatch(case.g, width) as b:
        b.reset(damping=0.0)
        recs = b.run_queue(qs, 5, TOL)
        assert all(r["iterations"] == 2 and r["converged"] for r in recs)  # r = t twice: an L1 of 0
        last = {r["column"]: q for q, r in enumerate(recs)}
        assert sorted(last) == list(range(width))
        assert any(qs[q][2] != 0 for q in last.values())  # a rest != 0 among them
        b.step(1)
        for c, q in last.items():
            assert np.array_equal(bits(b.ranks(c)), bits(dense(qs[q], V))), (c, q)


# ---- 5: errors -----------------------------------------------------------------------------------
def test_errors(hip, case):
    import ctypes

    from sparky_hip import _lib

    def raises(code, fn, *args, **kw):
        with pytest.raises(hip.PageRankError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, ei.value

    V = case.V
    INV, ST = _lib.PR_ERR_INVALID, _lib.PR_ERR_STATE
    good = case.queries[0]
    with hip.PageRankBatch(case.g, 3) as b:
        L = _lib.load()
        ex, conv = ctypes.c_int32(0), ctypes.c_uint32(0)
        # before reset
        raises(ST, b.reset_column, 0)
        raises(ST, b.step_until_any, 0b1, 10, TOL)
        raises(ST, b.run_queue, [good], 10, TOL)
        # argument errors win over the state error
        for col in (-1, 3, 16):
            raises(INV, b.reset_column, col)
        raises(INV, b.step_until_any, 0b1000, 10, TOL)
        b.reset()
        for col in (-1, 3, 16):
            raises(INV, b.reset_column, col)
        for bad in (np.nan, -1.0, np.inf, -np.inf):
            raises(INV, b.step_until_any, 0b1, 10, bad)
            raises(INV, b.run_queue, [good], 10, bad)
        raises(INV, b.step_until_any, 0b1, -1, TOL)
        raises(INV, b.step_until_any, 0b1000, 10, TOL)  # a bit at width
        raises(INV, b.step_until_any, 1 << 16, 10, TOL)
        raises(INV, b._step_until_any_ex, 0b1, 10, TOL, 0)
        assert L.pr_batch_step_until_any(b._h, 1, 10, TOL, None, ctypes.byref(conv)) == INV
        assert L.pr_batch_step_until_any(b._h, 1, 10, TOL, ctypes.byref(ex), None) == INV
        raises(INV, b.run_queue, [good], 0, TOL)
        raises(INV, b.run_queue, [good], -1, TOL)
        assert L.pr_batch_run_queue(b._h, -1, None, 10, TOL, None, None, None) == INV
        assert L.pr_batch_run_queue(b._h, 1, None, 10, TOL, None, None, None) == INV
        assert L.pr_batch_run_queue(b._h, 0, None, 10, TOL, None, None, None) == _lib.PR_OK
        assert b.run_queue([], 10, TOL) == []
        # a bad query anywhere in the list changes nothing
        b.step(3)
        before = snapshot(b)
        one = np.array([0], np.int32)
        bad_queries = [
            (np.array([V], np.int32), np.array([1.0])),                      # ID outside [0, V)
            (np.array([-1], np.int32), np.array([1.0])),
            (np.array([0, 0], np.int32), np.array([1.0, 2.0])),              # a duplicate
            (one, np.array([np.nan])),                                       # a non-finite value
            (one, np.array([1.0]), np.inf),                                  # a non-finite rest
            (one, np.array([1.0]), 0.0, np.array([V], np.int32)),            # exclusion outside [0, V)
            (one, np.array([1.0]), 0.0, np.array([0, 0], np.int32)),         # a duplicate exclusion
        ]
        for bad in bad_queries:
            for queue in ([bad], [good, good, good, good, bad], [good, bad, good]):
                raises(INV, b.run_queue, queue, 10, TOL)
        after = snapshot(b)
        assert all(same_column(after, before, j) for j in range(3)) and b.info()["iters"] == 3
        assert L.pr_batch_run_queue(b._h, 1, None, 10, TOL, None, None, None) == INV
        # inside the callback only the three getters run
        seen, internal = [], []

        def on_done(q, column, rec):
            b.ranks(column), b.topk(column, 2), b.norms()
            ns = ctypes.c_int64(0)
            internal.append(L.pr_batch_topk_all_kernel_ns(b._h, ctypes.byref(ns)))  # the internal entry points, too
            for fn, args in ((b.step, (1,)), (b.reset, ()), (b.reset_column, (0,)), (b.set_teleport, (0, None)),
                             (b.set_teleport_sparse, (0, one, np.array([1.0]))), (b.set_exclude, (0, one)),
                             (b.step_until, (1, TOL)), (b.step_until_any, (1, 1, TOL)), (b.topk_all, (1,)),
                             (b.run_queue, ([good], 1, TOL)), (b.sync, ())):
                try:
                    fn(*args)
                    seen.append(None)
                except hip.PageRankError as e:
                    seen.append(e.code)

        recs = b.run_queue([good], MAXIT, TOL, on_done=on_done)
        assert seen == [ST] * 11 and internal == [ST]
        assert recs[0]["iterations"] == case.want(0)[0]
        b.step(1)  # and outside the callback everything runs again
        b.sync()
        with pytest.raises(RuntimeError, match="boom"):  # an exception of on_done surfaces after the run

            def boom(q, column, rec):
                raise RuntimeError("boom")

            b.run_queue([good, good], MAXIT, TOL, on_done=boom)


# ---- 6: both CLIs --------------------------------------------------------------------------------
def run_cli(runner, args):
    import os
    import subprocess
    import sys

    from conftest import PKG_DIR

    base = [os.path.join(PKG_DIR, "build", "pagerank")] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    res = subprocess.run(base + args, capture_output=True, env=dict(os.environ, PYTHONPATH=PKG_DIR), timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout.decode()


def blocks(text):
    """The output cut at its '# seed set' lines: [(header, [lines])]; nothing may come before the first."""
    out = []
    for ln in text.splitlines():
        if ln.startswith("# seed set "):
            out.append((ln, []))
        else:
            out[-1][1].append(ln)
    return out


def test_cli_seed_queue(tmp_path):
    """The KAT with a queue of 20 seed files through 3 slots.  The files cycle through five contents
    (the solo runs they are compared with are one process each)."""
    contents = ["A\n", "C 2\nA\n", "# one seed\nF\n", "B 3\nE\nD 0.5\n", "D\n"]
    seeds = [{"A"}, {"C", "A"}, {"F"}, {"B", "E", "D"}, {"D"}]
    inp = tmp_path / "edges.txt"
    inp.write_text("\n".join(KAT) + "\n")
    files = []
    for q in range(20):
        f = tmp_path / f"set{q:02d}.txt"
        f.write_text(contents[q % 5])
        files.append(str(f))
    lst = tmp_path / "queue.txt"
    lst.write_text("# the queue\n" + "\n".join(files[:7]) + "\n\n" + "\n".join(files[7:]) + "\n")
    common = [str(inp), str(CAP), "--tol", "1e-6", "--top", "4"]
    solo = {}
    for c in range(5):  # what --seed-set prints for the file alone, after the iteration lines
        text = run_cli("cpp", common + ["--seed-set", files[c]])
        lines = [ln for ln in text.splitlines() if not ln.startswith("Starting iter")]
        assert lines[0] == f"# seed set 0: {files[c]}" and lines[1].endswith("(converged)")
        solo[c] = lines[1:]
    out = {}
    for variant in ([], ["--exclude-seeds"]):
        queue = common + ["--seed-queue", str(lst), "--slots", "3"] + variant
        got = run_cli("cpp", queue)
        assert got == run_cli("python", queue)  # identical bytes
        assert "Starting iter" not in got
        out[bool(variant)] = bl = blocks(got)
        assert [h for h, _ in bl] == [f"# seed set {q}: {files[q]}" for q in range(20)]  # queue order
    for q, (_, lines) in enumerate(out[False]):
        assert lines == solo[q % 5], q
    for q, (_, lines) in enumerate(out[True]):
        assert lines[0] == solo[q % 5][0]  # the exclusions do not touch the iteration
        urls = [ln.split(" has rank: ")[0] for ln in lines[1:]]
        assert len(urls) == min(4, 6 - len(seeds[q % 5])) and not set(urls) & seeds[q % 5], (q, urls)
        # the listing without the seeds: the plain one's order with them taken out
        plain = [ln for ln in out[False][q][1][1:] if ln.split(" has rank: ")[0] not in seeds[q % 5]]
        assert lines[1:1 + len(plain)] == plain
