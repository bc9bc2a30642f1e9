"""Batch mixes on the GPU: pr_batch_mix_topk / pr_batch_mix_get through PageRankBatch.mix_topk / mix /
_mix_topk_ex, and both CLIs' --mix.

Main statements: a one-hot mix is its column (IDs and bits of topk / topk_all / ranks); any mix
equals the numpy model of tests/batch_mix_model.py bit for bit -- separate `*` and `+`, columns
ascending, zero weights skipped -- in the dense blend, in the listing and between the two; the bits
do not depend on the kernel's grid, on the select's narrowing, on the number of mixes in the call
or on what a column of weight 0 holds.

Exact column bits are planted as tests/test_gpu_batch_topk.py does: reset(damping=0.0),
set_teleport(j, t), step(1) leaves column j exactly t; reset(init_ranks=x) leaves every column x
(-0.0 and subnormals kept).  The planted vectors are exact_model.grid_vector's multiples of 1/16, so
tie classes are large and, under dyadic weights, every blend is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_mix_model as bmm
import exact_model as em
from conftest import PKG_DIR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
CLI = os.path.join(PKG_DIR, "build", "pagerank")
KAT = ["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"]  # tests/test_cli_gpu.py
bits, same = bmm.bits, bmm.same


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def ring(hip, V):
    """v -> v + 1 (V = 1: a self-loop)."""
    v = np.arange(V, dtype=np.int32)
    return hip.PageRankGraph(V, v, ((v + 1) % V).astype(np.int32))


def plant(b, cols):
    """Column j holds cols[j] exactly (a -0.0 as +0.0)."""
    for j, t in enumerate(cols):
        b.set_teleport(j, t)
    b.reset(damping=0.0)
    b.step(1)


def columns(V, width, seed):
    """Grid vectors (large exact tie classes) and, in every third column, random doubles with negative ones."""
    rng = np.random.default_rng(seed)
    return [em.grid_vector(V, seed + j) if j % 3 else rng.standard_normal(V) for j in range(width)]


def weight_rows(width, n_mixes, seed):
    """Random finite weights; among them negative ones, zeros of both signs and dyadic ones."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((n_mixes, width))
    for i in range(n_mixes):
        if i % 4 == 1:
            w[i] = rng.choice(np.array([0.25, -0.5, 0.75, 2.0, 0.0, -0.0]), width)
        elif i % 4 == 2:
            w[i, rng.random(width) < 0.5] = 0.0
        elif i % 4 == 3:
            w[i] = 0.0  # no participating column: +0.0 everywhere, the listing is ID order
            if i % 8 == 3:
                w[i, rng.integers(0, width)] = -1.0
    return w


def check_model(b, w, ks, excluded=None, fulls=None):
    """mix == the model's bits; mix_topk == the model's listing; the listing's scores are mix's bits."""
    w = np.atleast_2d(w)
    fulls = [b.ranks(j).copy() for j in range(b.width)] if fulls is None else fulls
    want = [bmm.blend(row, fulls) for row in w]
    dense = [b.mix(row) for row in w]
    for i in range(len(w)):
        assert np.array_equal(bits(dense[i]), bits(want[i])), i
    for k in ks:
        lists = b.mix_topk(w, k, excluded)
        assert len(lists) == len(w)
        for i in range(len(w)):
            ex = () if excluded is None or excluded[i] is None else excluded[i]
            assert same(lists[i], bmm.listing(want[i], k, ex)), (k, i)
            assert np.array_equal(bits(lists[i][1]), bits(dense[i][lists[i][0]])), (k, i)
    return fulls, want


# ---- 1. identity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 5, 16])
def test_one_hot_is_the_column(hip, width):
    V = 300
    with ring(hip, V) as g, hip.PageRankBatch(g, width) as b:
        plant(b, [em.grid_vector(V, 40 + j) for j in range(width)])
        fulls = [b.ranks(j).copy() for j in range(width)]
        s = np.sort(fulls[0])[::-1]
        k_tie = next(k for k in range(2, V) if s[k - 1] == s[k])  # column 0's list is cut inside a tie class
        eye = np.eye(width)
        for k in (1, k_tie, V + 7):
            mixes, every = b.mix_topk(eye, k), b.topk_all(k)
            for j in range(width):
                assert same(mixes[j], every[j]) and same(mixes[j], b.topk(j, k)), (k, j)
                assert len(mixes[j][0]) == min(k, V)
                assert same(b.mix_topk(eye[j], k)[0], every[j])  # a (width,) vector is one mix
        for j in range(width):
            assert np.array_equal(bits(b.mix(eye[j])), bits(fulls[j]))
    with ring(hip, 65) as g, hip.PageRankBatch(g, 3) as b:  # -0.0 and subnormals, kept by init_ranks
        x = np.random.default_rng(1).choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e300]), 65)
        b.reset(init_ranks=x)
        for j in range(3):
            assert np.array_equal(bits(b.mix(np.eye(3)[j])), bits(x))
            assert same(b.mix_topk(np.eye(3)[j], 70)[0], b.topk(j, 70))


# ---- 2. the model --------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 2), (5, 3), (16, 1), (16, 16), (2, 16)]  # (width, n_mixes)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1000])
def test_model(hip, V):
    with ring(hip, V) as g:
        for width, n_mixes in SHAPES:
            with hip.PageRankBatch(g, width) as b:
                plant(b, columns(V, width, 7 * V + width))
                check_model(b, weight_rows(width, n_mixes, V + n_mixes), sorted({1, min(7, V), V + 5}))


# ---- 3. kernel boundaries ------------------------------------------------------------------------
@pytest.mark.parametrize("width,n_mixes", [(5, 3), (16, 16), (16, 1), (1, 16)])
def test_grid_cap_and_narrowing(hip, width, n_mixes):
    V, k = 1000, 50
    with ring(hip, V) as g, hip.PageRankBatch(g, width) as b:
        plant(b, [np.random.default_rng(j).random(V) for j in range(width)])
        w = np.random.default_rng(9).standard_normal((n_mixes, width))
        plain = b.mix_topk(w, k)
        fulls = [b.ranks(j) for j in range(width)]
        for i in range(n_mixes):
            assert same(plain[i], bmm.listing(bmm.blend(w[i], fulls), k))
        for cap in (1, 2):  # 256 vertices per workgroup and trip: four and two trips of the grid-stride loop
            lists, info = b._mix_topk_ex(w, k, grid_cap=cap)
            assert all(same(x, y) for x, y in zip(lists, plain)), cap
            assert info["mix_ns"] >= 0
        sides = {}
        for div in (0, 1, 8):
            lists, info = b._mix_topk_ex(w, k, narrow_div=div)
            assert all(same(x, y) for x, y in zip(lists, plain)), div
            sides[div] = info
        assert sides[0]["cand_passes"] == 0 and sides[0]["matrix_passes"] >= 2  # never narrowed
        assert sides[1]["cand_passes"] >= 1 and sides[1]["matrix_passes"] == 1  # narrowed at once
        assert sides[8]["matrix_passes"] >= 1 and sides[8]["select_ns"] >= 0


# ---- 4. exclusions -------------------------------------------------------------------------------
def test_exclusions(hip):
    V, W = 300, 3
    with ring(hip, V) as g, hip.PageRankBatch(g, W) as b:
        plant(b, [em.grid_vector(V, 60 + j) for j in range(W)])
        w = np.array([[0.5, 0.25, 0.0], [0.5, 0.25, 0.0], [0.0, 1.0, -0.5], [1.0, 0.0, 0.0]])
        fulls, want = check_model(b, w, [5])
        everyone = np.arange(V, dtype=np.int32)
        order = bmm.listing(want[0], V)[0]
        k = next(k for k in range(4, V) if want[0][order[k - 1]] == want[0][order[k]])  # a tie class straddles k
        tie = [int(v) for v in order if want[0][v] == want[0][order[k]]]
        cut = tie[: len(tie) // 2 + 1]  # the low IDs of that class: the listing moves on to its higher IDs
        excl = [cut, None, everyone, [int(order[0])]]
        before = b.topk_all(10)
        for kk in (1, k, V + 3):
            lists = b.mix_topk(w, kk, excl)
            for i, ex in enumerate(excl):
                n_i = 0 if ex is None else len(ex)
                assert len(lists[i][0]) == min(kk, V - n_i), (kk, i)
                assert same(lists[i], bmm.listing(want[i], kk, () if ex is None else ex)), (kk, i)
        lists = b.mix_topk(w, k, excl)
        assert not set(lists[0][0]) & set(cut) and same(lists[1], bmm.listing(want[1], k))  # the same weights, no set
        assert len(lists[2][0]) == 0 and int(order[0]) not in lists[3][0]
        # the columns' own sets play no part in a mix, and a mix changes nothing for them
        b.set_exclude(0, order[:20])
        b.set_exclude(1, everyone)
        with_sets = b.topk_all(10)
        assert len(with_sets[1][0]) == 0 and not set(with_sets[0][0]) & set(order[:20].tolist())
        assert all(same(x, y) for x, y in zip(b.mix_topk(w, k, excl), lists))
        assert all(same(x, bmm.listing(y, 10)) for x, y in zip(b.mix_topk(w, 10), want))
        assert all(same(x, y) for x, y in zip(b.topk_all(10), with_sets))
        b.set_exclude(0, None)
        b.set_exclude(1, None)
        assert all(same(x, y) for x, y in zip(b.topk_all(10), before))


# ---- 5. independence -----------------------------------------------------------------------------
def test_independence(hip):
    V, W = 300, 4
    rng = np.random.default_rng(11)
    src = np.concatenate([np.arange(V), rng.integers(0, V, 4 * V)]).astype(np.int32)  # every vertex has an out-link
    dst = np.concatenate([(np.arange(V) + 1) % V, rng.integers(0, V, 4 * V)]).astype(np.int32)
    huge = np.where(np.arange(V) % 2 == 0, 1.7e308, -1.7e308)
    w = np.array([[0.375, -1.25, 0.0, 0.0], [1.0 / 3.0, 0.7, -0.0, 0.0]])
    with hip.PageRankGraph(V, src, dst) as g:
        out = []
        for poisoned in (False, True):
            with hip.PageRankBatch(g, W) as b:
                b.set_teleport(0, em.grid_vector(V, 70))
                b.set_teleport(1, np.full(V, 0.1))
                if poisoned:
                    b.set_teleport(2, huge)  # overflows to +-inf within two iterations, then inf - inf = NaN
                b.reset()
                b.step(6)
                if poisoned:
                    bad = np.where(np.arange(V) % 3 == 0, np.inf, np.where(np.arange(V) % 3 == 1, -np.inf, np.nan))
                    b.reset_column(3, init_ranks=bad)
                    r2 = b.ranks(2)
                    assert np.isnan(r2).any() and not np.isfinite(r2).any()
                    assert np.array_equal(np.isnan(b.ranks(3)), np.isnan(bad))
                dense = [b.mix(row).copy() for row in w]
                lists = b.mix_topk(w, 40)
                again = b.mix_topk(w, 40)  # two runs agree
                assert all(same(x, y) for x, y in zip(lists, again))
                assert all(np.array_equal(bits(b.mix(row)), bits(d)) for row, d in zip(w, dense))
                # the same weights as mix 0 of 1 and as mix 15 of 16
                many = np.vstack([rng.standard_normal((15, W)) * [1, 1, 0, 0], w[1]])
                assert same(b.mix_topk(w[1], 40)[0], lists[1]) and same(b.mix_topk(many, 40)[15], lists[1])
                assert np.array_equal(bits(b.mix(w[1])), bits(dense[1]))
                assert np.isfinite(dense[0]).all() and np.isfinite(dense[1]).all()
                out.append((dense, lists))
        for i in range(2):  # what columns 2 and 3 hold does not reach a mix that gives them weight 0
            assert np.array_equal(bits(out[0][0][i]), bits(out[1][0][i]))
            assert same(out[0][1][i], out[1][1][i])


# ---- 6. linearity --------------------------------------------------------------------------------
def test_linearity_uniform_mode(hip):
    """After the same 20 iterations from the same initial ranks, the column that carries the teleport
    vector 0.25 t_0 + 0.75 t_1 and the mix 0.25 r_0 + 0.75 r_1 differ only by the order of summation:
    within the project's parity bound between orders, 1e-9 relative (README).
    Measured on an MI355X: 5.99e-16 (profiles/batch_mix/README.md)."""
    inp = em.dyadic_graph("mix_linearity", 512, 7, 300, n_sinks=3, n_indeg0=30)
    t0, t1 = em.grid_vector(inp.V, 80), em.grid_vector(inp.V, 81)
    t2 = 0.25 * t0 + 0.75 * t1  # exact: dyadic weights on the grid
    with hip.PageRankGraph(inp.V, inp.src, inp.dst) as g, hip.PageRankBatch(g, 3) as b:
        for j, t in enumerate((t0, t1, t2)):
            b.set_teleport(j, t)
        assert b.dangling == "uniform"
        b.reset()
        b.step(20)
        m, r2 = b.mix([0.25, 0.75, 0.0]), b.ranks(2)
        assert r2.min() > 0.0
        rel = float(np.max(np.abs(m - r2) / r2))
        print(f"linearity: max relative difference {rel:.3e} over {inp.V} vertices")
        assert rel <= 1e-9


# ---- 7. state, errors, memory --------------------------------------------------------------------
def test_errors_state_and_memory(hip):
    from sparky_hip import _lib

    lib = _lib.load()
    V, W = 300, 3
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    w = np.array([[0.5, 0.5, 0.0], [1.0, -0.25, 2.0]])
    with ring(hip, V) as g, hip.PageRankBatch(g, W) as b:
        for fn in (lambda: b.mix_topk(w, 5), lambda: b.mix(w[0]), lambda: b._mix_topk_ex(w, 5)):  # before reset
            with pytest.raises(hip.PageRankError) as ei:
                fn()
            assert ei.value.code == _lib.PR_ERR_STATE
        plant(b, columns(V, W, 90))
        ref = b.topk_all(8)
        bytes0 = b.info()["device_bytes"]
        ids, sc, n = np.zeros(40, np.int32), np.zeros(40, np.float64), np.full(2, 9, np.int32)
        ne, ex0 = np.array([2, 0], np.int32), np.array([3, 4], np.int32)

        def call(n_mixes=2, weights=w, n_excl=None, sets=None, k=5, ids_=ids, sc_=sc, n_=n):
            arr = None
            if sets is not None:
                arr = (ctypes.c_void_p * len(sets))(*[None if s is None else s.ctypes.data for s in sets])
            return lib.pr_batch_mix_topk(b._h, n_mixes, None if weights is None else p(weights),
                                         None if n_excl is None else p(n_excl),
                                         None if arr is None else ctypes.cast(arr, ctypes.c_void_p), k,
                                         None if ids_ is None else p(ids_), None if sc_ is None else p(sc_),
                                         None if n_ is None else p(n_))

        bad = [dict(weights=None), dict(n_=None), dict(n_mixes=0), dict(n_mixes=17), dict(n_mixes=-1),
               dict(weights=np.array([[0.5, np.nan, 0.0], [1.0, 0.0, 0.0]])),
               dict(weights=np.array([[0.5, 0.0, 0.0], [1.0, 0.0, -np.inf]])),
               dict(k=-1), dict(ids_=None), dict(sc_=None),
               dict(n_excl=ne), dict(sets=[ex0, None]),  # exactly one of the two
               dict(n_excl=np.array([2, -1], np.int32), sets=[ex0, None]),
               dict(n_excl=np.array([2, 1], np.int32), sets=[ex0, None]),  # NULL set with n > 0
               dict(n_excl=ne, sets=[np.array([3, V], np.int32), None]),
               dict(n_excl=ne, sets=[np.array([-1, 3], np.int32), None]),
               dict(n_excl=ne, sets=[np.array([7, 7], np.int32), None])]
        out = np.zeros(V)

        def every_bad_call(held):
            """Each is PR_ERR_INVALID, writes no n_out and leaves the batch's device bytes at `held`."""
            for kw in bad:
                n[:] = 9
                assert call(**kw) == _lib.PR_ERR_INVALID, kw
                assert lib.pr_last_error()
                assert list(n) == [9, 9] and b.info()["device_bytes"] == held, kw
            assert lib.pr_batch_mix_get(b._h, None, p(out)) == _lib.PR_ERR_INVALID
            assert lib.pr_batch_mix_get(b._h, p(w), None) == _lib.PR_ERR_INVALID
            assert lib.pr_batch_mix_get(b._h, p(np.array([1.0, np.inf, 0.0])), p(out)) == _lib.PR_ERR_INVALID
            assert b.info()["device_bytes"] == held

        # on a batch that has never mixed: a bad call that got as far as the blend matrix, the mask or the
        # select's scratch before it was rejected would show in the bytes
        every_bad_call(bytes0)
        assert all(same(x, y) for x, y in zip(b.topk_all(8), ref))
        assert call(n_excl=ne, sets=[ex0, None]) == _lib.PR_OK and list(n) == [5, 5]  # the call itself is sound
        bytes1 = b.info()["device_bytes"]
        assert bytes1 > bytes0  # the blends, the mask, the select's scratch
        every_bad_call(bytes1)  # and once the state exists: nothing grows (n_mixes = 17 would widen the matrix)
        assert all(same(x, y) for x, y in zip(b.topk_all(8), ref))
        assert call(k=0, ids_=None, sc_=None) == _lib.PR_OK and list(n) == [0, 0]  # k == 0
        assert all(len(i) == 0 for i, _ in b.mix_topk(w, 0))
    # memory: grows with the first mix, stays put on a second, grows with a wider n_mixes
    with ring(hip, V) as g, hip.PageRankBatch(g, W) as b:
        plant(b, columns(V, W, 91))
        b.topk_all(5), b.topk(0, 5), b.ranks(0)
        base = b.info()["device_bytes"]
        b.mix_topk(w[0], 5)
        first = b.info()["device_bytes"]
        assert first >= base + 8 * V  # V x 1 doubles at least
        b.mix_topk(w[0], 5)
        b.mix(w[0])
        assert b.info()["device_bytes"] == first
        three = np.vstack([w, w[:1]])  # three mixes: stride 4
        b.mix_topk(three, 5)
        wider = b.info()["device_bytes"]
        assert wider >= first + 8 * V * 3
        b.mix_topk(three, 5)
        b.mix(w[1])  # one mix in the wider matrix: the stride stays at the largest seen
        assert b.info()["device_bytes"] == wider
        b.mix_topk(three, 5, [[1, 2], None, None])
        assert b.info()["device_bytes"] >= wider + 2 * V  # the mask: one uint16 per vertex, with the first set


def test_after_every_way_to_iterate(hip):
    V, W = 400, 3
    rng = np.random.default_rng(13)
    src, dst = rng.integers(0, V, 2000), rng.integers(0, V, 2000)
    dst[rng.random(2000) < 0.05] = -1
    src = np.concatenate([src, np.arange(V)]).astype(np.int32)
    dst = np.concatenate([dst, np.full(V, -1)]).astype(np.int32)
    w = np.array([[0.5, 0.5, 0.0], [1.0, -0.25, 0.125]])
    seeds = [(np.array([3 * q, 3 * q + 1], np.int32), np.array([0.15 * V / 2] * 2)) for q in range(5)]
    with hip.PageRankGraph(V, src, dst) as g, hip.PageRankBatch(g, W) as b:
        for j in range(W):
            b.set_teleport_sparse(j, *seeds[j])
        for mode in ("uniform", "teleport"):  # the mix does not care how the columns were produced
            b.set_dangling(mode)
            b.reset()
            b.step(3)
            check_model(b, w, [10])
            b.step_until(50, 1e-6)
            check_model(b, w, [10])
        b.set_dangling("uniform")
        inside = []

        def on_done(q, column, rec):
            try:
                b.mix_topk(w, 3)
            except hip.PageRankError as e:
                inside.append(e.code)
            try:
                b.mix(w[0])
            except hip.PageRankError as e:
                inside.append(e.code)

        from sparky_hip import _lib

        recs = b.run_queue(seeds, 40, 1e-6, on_done=on_done)
        assert len(recs) == 5 and inside == [_lib.PR_ERR_STATE] * 10  # inside the callback: PR_ERR_STATE
        check_model(b, w, [10])


# ---- 8. both CLIs ----------------------------------------------------------------------------------
def run_cli(runner, args):
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    res = subprocess.run(base + args, capture_output=True, env=dict(os.environ, PYTHONPATH=PKG_DIR), timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_cli_mix(hip, tmp_path):
    from sparky_hip._host import HostEdges, seed_teleport

    inp, fa, fb = tmp_path / "edges.txt", tmp_path / "a.txt", tmp_path / "b.txt"
    inp.write_text("\n".join(KAT) + "\n")
    fa.write_text("C 2\nA\n")
    fb.write_text("# one seed\nF\n")
    sets = [str(fa), str(fb)]
    base = [str(inp), "10", "--seed-set", sets[0], "--seed-set", sets[1], "--top", "3"]
    given = ["0.5,0.5", "1,-0.25"]
    # with --exclude-seeds; a weight of 0 takes its set's seeds out of a mix's exclusion, and a value
    # that starts with '-' is a value
    given_x = ["0.5,0.5", "-1,0"]
    args = base + ["--mix", given[0], "--mix", given[1]]
    args_x = base + ["--exclude-seeds", "--mix", given_x[0], "--mix", given_x[1]]
    out = {r: run_cli(r, args) for r in ("cpp", "python")}
    outx = {r: run_cli(r, args_x) for r in ("cpp", "python")}
    assert out["cpp"] == out["python"] and outx["cpp"] == outx["python"]  # identical bytes
    plain, plainx = run_cli("cpp", base), run_cli("cpp", base + ["--exclude-seeds"])
    # the per-set part is the run without --mix, byte for byte
    assert out["cpp"].startswith(plain) and len(out["cpp"]) > len(plain)
    assert outx["cpp"].startswith(plainx) and len(outx["cpp"]) > len(plainx)
    edges = HostEdges.read(str(inp), "edges")
    V = edges.n_vertices

    def listings(bt, weights, excl, texts, tag):
        lists = bt.mix_topk(np.array(weights), 3, excl)
        want = b""
        for i, text in enumerate(texts):
            path = tmp_path / f"mix{tag}{i}.txt"
            edges.write_has_rank_ids(str(path), *lists[i])
            want += f"# mix {i}: {text}\n".encode() + path.read_bytes()
        return want

    with hip.PageRankGraph(V, edges.src, edges.dst) as g, hip.PageRankBatch(g, 2) as bt:
        seed_ids = []
        for j, path in enumerate(sets):
            ids, weights = edges.read_seeds(path)
            seed_ids.append(ids)
            bt.set_teleport_sparse(j, ids, seed_teleport(weights, V))
        bt.reset()
        bt.step(10)
        want = listings(bt, [[0.5, 0.5], [1.0, -0.25]], None, given, "")
        both = np.unique(np.concatenate(seed_ids))
        want_x = listings(bt, [[0.5, 0.5], [-1.0, 0.0]], [both, seed_ids[0]], given_x, "x")
    edges.close()
    assert out["cpp"][len(plain):] == want and outx["cpp"][len(plainx):] == want_x  # the Python API's listings
    tail = outx["cpp"][len(plainx):].decode().splitlines()
    assert tail[0] == "# mix 0: 0.5,0.5" and tail[4] == "# mix 1: -1,0" and len(tail) == 8
    names = [[ln.rsplit(" has rank: ", 1)[0] for ln in tail[1 + 4 * i: 4 + 4 * i]] for i in range(2)]
    assert not set(names[0]) & {"A", "C", "F"} and not set(names[1]) & {"A", "C"}
