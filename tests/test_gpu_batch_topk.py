"""Batch top-K on the GPU: pr_batch_get_topk_all and pr_batch_set_exclude through
PageRankBatch.topk_all / set_exclude, and both CLIs' --exclude-seeds.

Main statement: for every column, topk_all(k)[j] equals topk(j, k) in IDs and rank bits, and both
equal the numpy reference computed from ranks(j): np.lexsort((ids, -key)) over the vertices the
column does not exclude, key = the order-preserving u64 image of the rank's bits (rank descending,
-0.0 just below +0.0, ties by ID ascending).  IDs compare for equality, ranks bitwise.

Exact rank bits are planted without a hook: reset(init_ranks=x) with no iteration gives every column
x (with -0.0 and subnormals); reset(damping=0.0), set_teleport(j, t), step(1) gives column j exactly
t (the update is t + 0 * (...); a -0.0 comes back as +0.0).

The one strategy switch -- histogram passes over the matrix until the active columns' candidates are
at most V * width / narrow_div together, then over the compacted candidates -- is a parameter of the
internal entry point (PageRankBatch._topk_all_ex): narrow_div = 0 never compacts, 8 is what topk_all
uses; the tests assert from the returned pass counts that each side ran."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "build", "pagerank")
KAT = ["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"]  # tests/test_cli_gpu.py
WIDTHS = [1, 3, 5, 8, 11, 16]


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def rank_keys(x):
    b = bits(x)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def reference(full, k, excluded=()):
    own = np.setdiff1d(np.arange(len(full)), np.asarray(excluded, np.int64))
    o = own[np.lexsort((own, ~rank_keys(full[own])))][: max(k, 0)]
    return o.astype(np.int32), full[o]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def check_all(b, ks, excluded=None, fulls=None):
    """topk_all(k)[j] == topk(j, k) == the reference from ranks(j), for every column and k."""
    W = b.width
    fulls = [b.ranks(j).copy() for j in range(W)] if fulls is None else fulls  # once, shared by every k
    for k in ks:
        lists = b.topk_all(k)
        assert len(lists) == W
        for j in range(W):
            want = reference(fulls[j], k, excluded[j] if excluded else ())
            assert same(lists[j], want), (k, j)
            assert same(b.topk(j, k), want), (k, j)
    return fulls


def ring(hip, V):
    """v -> v + 1 (V = 1: a self-loop)."""
    v = np.arange(V, dtype=np.int32)
    return hip.PageRankGraph(V, v, ((v + 1) % V).astype(np.int32))


def patterns(V, rng):
    """Rank columns that finish at different passes of the select."""
    low = (np.full(V, 0.15).view(np.uint64) & ~np.uint64(0xFF)) | rng.integers(0, 256, V).astype(np.uint64)
    mixed = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, 2.5, -2.5, 1e-310]), V)
    ties = rng.choice(np.array([0.15, 1.0, 3.0]), V, p=[0.6, 0.3, 0.1])
    return [np.full(V, 0.15),  # all equal: ID order, all 12 digits
            rng.random(V) * 3.0, low.view(np.float64),  # differ in the lowest mantissa byte only
            mixed, ties, -rng.random(V), np.arange(V) * 1.0]


def plant(b, cols):
    """Column j holds cols[j] exactly (a -0.0 as +0.0)."""
    for j, t in enumerate(cols):
        b.set_teleport(j, t)
    b.reset(damping=0.0)
    b.step(1)


# ---- tiny graphs, planted patterns -------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65])
def test_tiny_graphs_planted(hip, V):
    rng = np.random.default_rng(V)
    pats = patterns(V, rng)
    ks = sorted({1, 7, 64, 65, max(V - 1, 0), V, V + 5})
    with ring(hip, V) as g:
        for W in WIDTHS:
            with hip.PageRankBatch(g, W) as b:
                cols = [pats[(j + W) % len(pats)] for j in range(W)]  # a different pattern in every column
                plant(b, cols)
                fulls = check_all(b, ks)
                for j in range(W):
                    assert np.array_equal(bits(fulls[j]), bits(cols[j] + 0.0))
                assert all(len(i) == 0 for i, _ in b.topk_all(0))
        with hip.PageRankBatch(g, 3) as b:  # init_ranks: every column the same bits, -0.0 and subnormals kept
            x = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e300]), V)
            b.reset(init_ranks=x)
            fulls = check_all(b, ks)
            assert all(np.array_equal(bits(f), bits(x)) for f in fulls)


def test_tie_class_straddles_k(hip):
    """V = 65: 41 vertices share the rank at position K; the low IDs of the class are selected."""
    V, W = 65, 5
    with ring(hip, V) as g, hip.PageRankBatch(g, W) as b:
        t = np.full(V, 0.5)
        t[[3, 17, 40, 64]] = [9.0, 8.0, 7.0, 7.0]
        t[44:] = np.where(np.arange(44, V) == 64, 7.0, 0.25)
        plant(b, [t] * W)
        check_all(b, [4, 5, 10, 43, 44, 45])
        ids, _ = b.topk_all(10)[2]
        assert list(ids) == [3, 17, 40, 64, 0, 1, 2, 4, 5, 6]
        tie = [v for v in range(44) if v not in (3, 17, 40)]
        b.set_exclude(2, tie[:20])  # the low-ID half of the tie class at K
        excl = [(), (), tie[:20], (), ()]
        check_all(b, [4, 5, 10, 24, 25, V], excluded=excl)
        assert list(b.topk_all(6)[2][0]) == [3, 17, 40, 64, tie[20], tie[21]]


# ---- R-MAT -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,width", [(10, 5), (11, 8), (12, 16)])
def test_rmat(hip, scale, width):
    from sparky_hip.workloads import generate

    wl = generate("rmat", scale=scale, edge_factor=16, device=0)
    V = wl.n_vertices
    rng = np.random.default_rng(scale)
    with hip.PageRankGraph(V, wl.src.data_ptr(), wl.dst.data_ptr(), device=0, device_input=True,
                           n_edges=wl.n_edges) as g, hip.PageRankBatch(g, width) as b:
        for j in range(width - 2):  # seed-set columns; the last but one stays scalar
            seeds = rng.permutation(V)[: 1 + 3 * j].astype(np.int32)
            b.set_teleport_sparse(j, seeds, np.full(len(seeds), 0.15 * V / len(seeds)))
        b.set_teleport(width - 1, 0.15 - 0.4 * rng.random(V))  # negative teleport terms: negative ranks appear
        b.reset()
        done = 0
        for iters in (0, 3, 20):
            b.step(iters - done)
            done = iters
            fulls = check_all(b, [1, 7, 64, 65, 1000, V - 1, V, V + 5] if iters == 3 else [10, 1000])
        assert (fulls[width - 1] < 0).any()
        lists, info = b._topk_all_ex(100, 8)
        assert info["passes"] == info["matrix_passes"] + info["cand_passes"] <= 12


# ---- both sides of the narrowing switch --------------------------------------------------------
@pytest.mark.parametrize("V", [3000, 300_000])
def test_narrowing(hip, V):
    W = 16
    rng = np.random.default_rng(V)
    pats = patterns(V, rng)
    with ring(hip, V) as g, hip.PageRankBatch(g, W) as b:
        cols = [pats[j % len(pats)] if j % 4 else rng.random(V) for j in range(W)]
        cols[7] = rng.random(V) - 0.5
        cols[5] = np.full(V, 0.15)  # the one all-equal column: needs all 12 digits, V candidates until the ID digits
        plant(b, cols)
        fulls = [b.ranks(j).copy() for j in range(W)]
        orders = [reference(f, V)[0] for f in fulls]  # once; a prefix of it is every k's reference
        for k in (1, 100, 2000):
            want = [(orders[j][:k], fulls[j][orders[j][:k]]) for j in range(W)]
            sides = {}
            for div in (0, 8, 1):
                lists, info = b._topk_all_ex(k, div)
                assert all(same(lists[j], want[j]) for j in range(W)), (k, div)
                assert info["passes"] == info["matrix_passes"] + info["cand_passes"] == 12
                sides[div] = info
            assert sides[0]["cand_passes"] == 0 and sides[0]["narrowed_at"] == -1  # never compacted
            assert sides[8]["cand_passes"] > 0 and sides[8]["narrowed_at"] >= 1  # compacted, then candidate passes
            assert sides[1]["narrowed_at"] == 1 and sides[1]["cand_passes"] == 11
            assert all(same(b.topk_all(k)[j], want[j]) for j in (0, 5, 15))
        for j in (0, 5, 15):
            assert same(b.topk(j, 100), (orders[j][:100], fulls[j][orders[j][:100]]))


# ---- exclusions --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(hip):
    """V = 3000, E = 20000, 5 % no-link records (tests/test_gpu_batch.py's graph)."""
    V = 3000
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, V, 20000), rng.integers(0, V, 20000)
    dst[rng.random(20000) < 0.05] = -1
    src = np.concatenate([src, np.arange(V)]).astype(np.int32)
    dst = np.concatenate([dst, np.full(V, -1)]).astype(np.int32)
    with hip.PageRankGraph(V, src, dst) as g:
        yield g, V


def vectors(V, width):
    return [0.02 * (j + 1) + 1e-4 * ((np.arange(V) * (2 * j + 1)) % V) for j in range(width)]


def run_plain(hip, g, V, W, steps):
    """Per entry of `steps`: the ranks, norms and top-50 lists of a batch that never sets an exclusion."""
    with hip.PageRankBatch(g, W) as b:
        for j, t in enumerate(vectors(V, W)):
            b.set_teleport(j, t)
        b.reset()
        out = []
        for n in steps:
            b.step(n)
            out.append(([bits(b.ranks(j)).copy() for j in range(W)], [bits(x).copy() for x in b.norms()],
                        [b.topk(j, 50) for j in range(W)]))
        return out


def test_exclusions(hip, small):
    g, V = small
    W = 5
    plain = run_plain(hip, g, V, W, [4, 3])
    everyone = np.arange(V, dtype=np.int32)
    with hip.PageRankBatch(g, W) as b:
        for j, t in enumerate(vectors(V, W)):
            b.set_teleport(j, t)
        b.set_exclude(3, everyone[2:])  # valid any time after create: all but two vertices
        b.reset()
        b.step(4)
        fulls = [b.ranks(j).copy() for j in range(W)]
        top0 = int(reference(fulls[0], 1)[0][0])
        b.set_exclude(0, [top0])  # the top vertex
        b.set_exclude(1, everyone)  # every vertex
        excl = [[top0], everyone, (), everyone[2:], ()]
        check_all(b, [1, 7, 50, V, V + 5], excluded=excl, fulls=fulls)
        lists = b.topk_all(50)
        assert top0 not in lists[0][0] and len(lists[0][0]) == 50
        assert len(lists[1][0]) == 0 and len(b.topk(1, 50)[0]) == 0  # n_out == 0, PR_OK
        assert list(lists[3][0]) == list(reference(fulls[3], 50, everyone[2:])[0]) and len(lists[3][0]) == 2  # n_out == 2 < k
        for j in (2, 4):  # a column without a set: bitwise what a batch without any set returns
            assert same(lists[j], plain[0][2][j]) and same(b.topk(j, 50), plain[0][2][j])
        # ranks and norms never see a set
        for j in range(W):
            assert np.array_equal(bits(b.ranks(j)), plain[0][0][j])
        assert all(np.array_equal(bits(x), y) for x, y in zip(b.norms(), plain[0][1]))
        # replacing and clearing
        second = [int(v) for v in reference(fulls[0], 3)[0][1:]]
        b.set_exclude(0, second)
        excl[0] = second
        check_all(b, [1, 5], excluded=excl, fulls=fulls)
        assert b.topk_all(1)[0][0][0] == top0
        b.set_exclude(1, None)
        excl[1] = ()
        check_all(b, [5, V], excluded=excl, fulls=fulls)
        # further steps are those of a batch without sets; the sets survive reset
        b.step(3)
        for j in range(W):
            assert np.array_equal(bits(b.ranks(j)), plain[1][0][j])
        assert all(np.array_equal(bits(x), y) for x, y in zip(b.norms(), plain[1][1]))
        for j in (1, 2, 4):
            assert same(b.topk_all(50)[j], plain[1][2][j])
        b.reset()
        b.step(2)
        check_all(b, [3, 50], excluded=excl)
        assert len(b.topk_all(50)[3][0]) == 2


# ---- errors, states, memory --------------------------------------------------------------------
def test_errors_and_memory(hip, small):
    from sparky_hip import _lib

    g, V = small
    lib = _lib.load()

    def raises(code, fn, *args, **kw):
        with pytest.raises(hip.PageRankError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, ei.value

    bytes_g = g.info()["device_bytes"]
    with hip.PageRankBatch(g, 3) as b:
        bytes0 = b.info()["device_bytes"]
        raises(_lib.PR_ERR_STATE, b.topk_all, 5)  # before reset
        raises(_lib.PR_ERR_INVALID, b.set_exclude, 3, [1])  # bad column
        raises(_lib.PR_ERR_INVALID, b.set_exclude, -1, [1])
        raises(_lib.PR_ERR_INVALID, b.set_exclude, 0, [1, V])  # out of range
        raises(_lib.PR_ERR_INVALID, b.set_exclude, 0, [-1])
        raises(_lib.PR_ERR_INVALID, b.set_exclude, 0, [4, 7, 4])  # duplicate
        assert lib.pr_batch_set_exclude(b._h, 0, -1, None) == _lib.PR_ERR_INVALID
        assert lib.pr_batch_set_exclude(b._h, 0, 2, None) == _lib.PR_ERR_INVALID
        b.set_exclude(0, [])  # clearing an empty set allocates nothing
        assert b.info()["device_bytes"] == bytes0
        b.reset()
        b.step(2)
        b.ranks(0), b.norms(), b.topk(0, 5)
        bytes1 = b.info()["device_bytes"]  # the single select's scratch only
        n = np.zeros(3, np.int32)
        ids, rk = np.zeros(30, np.int32), np.zeros(30, np.float64)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        assert lib.pr_batch_get_topk_all(b._h, -1, p(ids), p(rk), p(n)) == _lib.PR_ERR_INVALID
        assert lib.pr_batch_get_topk_all(b._h, 5, p(ids), p(rk), None) == _lib.PR_ERR_INVALID
        assert lib.pr_batch_get_topk_all(b._h, 5, None, p(rk), p(n)) == _lib.PR_ERR_INVALID
        assert lib.pr_batch_get_topk_all(b._h, 5, p(ids), None, p(n)) == _lib.PR_ERR_INVALID
        n[:] = 9
        assert lib.pr_batch_get_topk_all(b._h, 0, None, None, p(n)) == _lib.PR_OK and (n == 0).all()
        assert b.info()["device_bytes"] == bytes1  # nothing allocated so far
        want = [b.topk(j, 5) for j in range(3)]
        assert all(same(x, w) for x, w in zip(b.topk_all(5), want))
        bytes2 = b.info()["device_bytes"]
        assert bytes2 > bytes1  # the select's scratch, from its first use on
        b.set_exclude(1, [int(want[1][0][0])])
        bytes3 = b.info()["device_bytes"]
        assert bytes3 == bytes2 + 2 * V  # the mask: one uint16 per vertex
        assert b.topk_all(5)[1][0][0] == want[1][0][1]
        bytes4 = b.info()["device_bytes"]
        assert b.topk(1, 5)[0][0] == want[1][0][1]
        assert b.info()["device_bytes"] >= bytes4 + 4 * V  # the single query's ID array, with its first need
        assert all(same(x, w) for x, w in zip(b.topk_all(5)[::2], want[::2]))
        assert g.info()["device_bytes"] == bytes_g  # the graph's own figure never moves
    assert g.info()["device_bytes"] == bytes_g


# ---- both CLIs -----------------------------------------------------------------------------------
def run_cli(runner, args):
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    res = subprocess.run(base + args, capture_output=True, env=dict(os.environ, PYTHONPATH=PKG_DIR), timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_cli_exclude_seeds(hip, tmp_path):
    from sparky_hip._host import HostEdges, seed_teleport

    inp, a, b = tmp_path / "edges.txt", tmp_path / "a.txt", tmp_path / "b.txt"
    inp.write_text("\n".join(KAT) + "\n")
    a.write_text("C 2\nA\n")
    b.write_text("# one seed\nF\n")
    sets = [str(a), str(b)]
    args = [str(inp), "10", "--seed-set", sets[0], "--seed-set", sets[1], "--top", "3"]
    out = {r: run_cli(r, args + ["--exclude-seeds", "--out", str(tmp_path / ("out_" + r))]) for r in ("cpp", "python")}
    assert out["cpp"] == out["python"]  # identical bytes
    lines = out["cpp"].decode().splitlines()
    assert lines[:10] == [f"Starting iter{i}" for i in range(10)] and len(lines) == 10 + 2 * 4
    listed = [[ln.rsplit(" has rank: ", 1)[0] for ln in lines[11 + 4 * j:14 + 4 * j]] for j in range(2)]
    assert not set(listed[0]) & {"A", "C"} and "F" not in listed[1]  # no seed of the set's own file
    for r in ("cpp", "python"):  # part files stay complete
        for j in range(2):
            rows = open(tmp_path / ("out_" + r) / f"seedset{j}" / "PageRank9" / "part-00000").read().splitlines()
            assert len(rows) == 6
    # without the flag: the per-column listing
    plain = {r: run_cli(r, args) for r in ("cpp", "python")}
    assert plain["cpp"] == plain["python"] and plain["cpp"] != out["cpp"]
    edges = HostEdges.read(str(inp), "edges")
    V = edges.n_vertices
    want = b"".join(f"Starting iter{i}\n".encode() for i in range(10))
    with hip.PageRankGraph(V, edges.src, edges.dst) as g, hip.PageRankBatch(g, 2) as bt:
        for j, path in enumerate(sets):
            ids, weights = edges.read_seeds(path)
            bt.set_teleport_sparse(j, ids, seed_teleport(weights, V))
        bt.reset()
        bt.step(10)
        for j in range(2):
            listing = tmp_path / f"listing{j}.txt"
            edges.write_has_rank_ids(str(listing), *bt.topk(j, 3))
            want += f"# seed set {j}: {sets[j]}\n".encode() + listing.read_bytes()
    edges.close()
    assert plain["cpp"] == want
