"""Batch top-K without a GPU: the two pr_batch_* symbols and their NULL-argument errors, the
per-column state of the lockstep select (csrc/pr_batch_topk.h) through host/batch_topk_shim.cpp, and
the --exclude-seeds usage errors of both CLIs (raised before any GPU work).

The shim's host model runs the library's own driver (btopk_select_thresholds) with the pass
structure of csrc/pr_batch_topk.hip over a V x stride array and an exclusion mask.  Reference for
every column: np.lexsort((ids, -key)) over the vertices the mask does not exclude, key = the
order-preserving u64 image of the rank's bits (so -0.0 sorts just below +0.0) -- rank descending, ties
by ID ascending; IDs compare for equality, ranks bitwise.  Every column's threshold
is also compared with the one topk_select_threshold (the single select's driver) finds for the same
keys."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

CLI = os.path.join(PKG_DIR, "build", "pagerank")
SHIM = os.path.join(PKG_DIR, "build", "libpr_batch_topk_shim.so")
SHAPES = [(1, 1), (2, 2), (4, 3), (8, 5), (8, 7), (16, 11), (16, 13), (16, 16)]  # (stride, width)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_symbols_and_null_arguments():
    import sparky_hip._lib as L

    lib = L.load()
    for name in ("pr_batch_set_exclude", "pr_batch_get_topk_all"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED
    assert hasattr(lib, "pr_batch_topk_all_ex") and "pr_batch_topk_all_ex" not in L.EXPORTED  # internal
    ids, rk, n = np.zeros(4, np.int32), np.zeros(4, np.float64), np.zeros(16, np.int32)
    assert lib.pr_batch_set_exclude(None, 0, 1, _p(ids)) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_get_topk_all(None, 2, _p(ids), _p(rk), _p(n)) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_topk_all_ex(None, 2, 8, _p(ids), _p(rk), _p(n), None) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()


def test_python_methods_exist():
    import sparky_hip

    for m in ("set_exclude", "topk_all", "_topk_all_ex"):
        assert callable(getattr(sparky_hip.PageRankBatch, m))


# ---- the shim ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    # always: make's dependency on the headers rebuilds a stale shim after an edit
    subprocess.run(["make", "-s", "-C", os.path.join(PKG_DIR, "host")], check=True)
    lib = ctypes.CDLL(SHIM)
    P, u64, i64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int
    lib.prbt_begin.argtypes = [P, u64, u64]
    lib.prbt_begin.restype = None
    lib.prbt_advance.argtypes = [P, ci, P]
    lib.prbt_advance.restype = None
    lib.prbt_threshold_ref.argtypes = [P, P, i64, u64, P, P]
    lib.prbt_select.argtypes = [P, i64, ci, ci, P, i64, i64, P, P, P, P, P, P, P]
    return lib


def rank_keys(x):
    b = bits(x)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def order(x, own):
    """The query's order of the vertices `own` under the ranks x[own]."""
    return own[np.lexsort((own, ~rank_keys(x[own])))]


def digit(hi, lo, p):
    if p < 8:
        return ((hi >> np.uint64(56 - 8 * p)) & np.uint64(0xFF)).astype(np.int64)
    return ((lo >> np.uint32(24 - 8 * (p - 8))) & np.uint32(0xFF)).astype(np.int64)


def threshold_ref(shim, hi, lo, k):
    thi, tlo = ctypes.c_uint64(), ctypes.c_uint32()
    hi, lo = np.ascontiguousarray(hi), np.ascontiguousarray(lo)
    passes = shim.prbt_threshold_ref(_p(hi), _p(lo), len(hi), k, ctypes.byref(thi), ctypes.byref(tlo))
    assert passes >= 1
    return thi.value, tlo.value, passes


def patterns(V, rng):
    """Rank columns that finish at different passes."""
    tiny = (np.full(V, 0.15).view(np.uint64) & ~np.uint64(0xFF)) | rng.integers(0, 256, V).astype(np.uint64)  # lowest mantissa byte only
    mixed = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, 2.5, -2.5, 1e-310]), V)
    ties = rng.choice(np.array([0.15, 1.0, 3.0]), V, p=[0.6, 0.3, 0.1])
    return [np.full(V, 0.15),  # all equal: the ID digits decide, all 12 passes
            rng.random(V) * 3.0, tiny.view(np.float64), mixed, ties, -rng.random(V), np.arange(V) * 1.0]


def test_advance_reaches_the_single_selects_threshold(shim):
    """btopk_begin / btopk_advance driven from numpy histograms, one column at a time."""
    rng = np.random.default_rng(2)
    V = 3000
    lo = (~np.arange(V, dtype=np.uint32)).astype(np.uint32)
    seen_passes = set()
    for x in patterns(V, rng):
        hi = rank_keys(x)
        for k in (1, 7, 256, 257, V - 1):
            st = np.zeros(5, np.uint64)
            shim.prbt_begin(_p(st), k, V)
            assert list(st) == [0, 0, k, V, 0]
            live = np.ones(V, bool)
            passes = 0
            while not st[4]:
                d = digit(hi, lo, passes)
                h = np.bincount(d[live], minlength=256).astype(np.uint32)
                shim.prbt_advance(_p(st), passes, _p(h))
                b = digit(np.array([st[0]], np.uint64), np.array([st[1]], np.uint32), passes)[0]
                live &= d == b
                passes += 1
                assert st[3] == live.sum() and 1 <= st[2] <= st[3]
            thi, tlo, ref_passes = threshold_ref(shim, hi, lo, k)
            assert (int(st[0]), int(st[1]), passes) == (thi, tlo, ref_passes)
            seen_passes.add(passes)
    assert 12 in seen_passes and min(seen_passes) <= 3
    for k, avail in ((0, 5), (5, 5), (9, 5), (0, 0)):  # nothing to select, or everything available: done, threshold 0
        st = np.ones(5, np.uint64)
        shim.prbt_begin(_p(st), k, avail)
        assert st[4] == 1 and st[0] == 0 and st[1] == 0


def model(shim, R, V, S, W, mask, k, div):
    kk = max(k, 1)
    ids, rk = np.zeros(W * kk, np.int32), np.zeros(W * kk, np.float64)
    n, cp, info = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(4, np.int32)
    thi, tlo = np.zeros(W, np.uint64), np.zeros(W, np.uint32)
    rc = shim.prbt_select(_p(R), V, S, W, _p(mask), k, div, _p(ids), _p(rk), _p(n), _p(thi), _p(tlo), _p(cp), _p(info))
    assert rc == 0
    return [(ids[j * k: j * k + n[j]], rk[j * k: j * k + n[j]]) for j in range(W)], thi, tlo, cp, info


@pytest.mark.parametrize("S,W", SHAPES)
def test_lockstep_model_equals_lexsort(shim, S, W):
    rng = np.random.default_rng(100 * S + W)
    V = 700
    pats = patterns(V, rng)
    R = np.zeros((V, S))
    R[:, W:] = 7.0  # padding columns never count, whatever they hold
    for j in range(W):
        R[:, j] = pats[j % len(pats)]
    mask = np.zeros(V, np.uint16)
    for j in range(W):
        if j % 3 == 1:  # a random set; the top vertex among it
            mask[rng.random(V) < 0.2] |= np.uint16(1 << j)
            mask[order(R[:, j], np.arange(V))[0]] |= np.uint16(1 << j)
        if j == 4:  # all but two vertices
            mask[2:] |= np.uint16(1 << j)
    everyone = np.arange(V, dtype=np.int32)
    for k, div in ((1, 8), (7, 8), (64, 0), (65, 1), (V - 1, 8), (V, 8), (V + 5, 8), (0, 8)):
        lists, thi, tlo, cp, info = model(shim, R, V, S, W, mask, k, div)
        assert info[0] == info[1] + info[2] <= 12 and info[0] == (cp.max() if W else 0)
        if div == 0:
            assert info[2] == 0 and info[3] == -1
        if div == 1 and info[0] > 1:
            assert info[3] == 1 and info[2] == info[0] - 1  # compacted after the first pass
        for j in range(W):
            own = np.nonzero(((mask >> np.uint16(j)) & np.uint16(1)) == 0)[0]
            o = order(np.ascontiguousarray(R[:, j]), own)[:k]
            gi, gr = lists[j]
            assert len(gi) == min(k, len(own))
            assert np.array_equal(gi, everyone[o]) and np.array_equal(bits(gr), bits(R[o, j]))
            if 0 < k < len(own):
                want = threshold_ref(shim, rank_keys(R[own, j]), (~own.astype(np.uint32)).astype(np.uint32), k)
                assert (int(thi[j]), int(tlo[j]), int(cp[j])) == want
            else:
                assert (thi[j], tlo[j], cp[j]) == (0, 0, 0)  # takes part in no pass
        if k == 7 and W >= 3:
            assert cp[0] == 12 and len(set(cp.tolist())) >= 2  # columns finish at different passes


def test_lockstep_model_without_a_mask(shim):
    rng = np.random.default_rng(9)
    V, S, W = 1000, 4, 3
    R = rng.random((V, S))
    with_zero_mask = model(shim, R, V, S, W, np.zeros(V, np.uint16), 10, 8)
    without = model(shim, R, V, S, W, None, 10, 8)
    for a, b in zip(with_zero_mask[0], without[0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- CLI usage errors (before any GPU work) ----------------------------------------------------
@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_exclude_seeds_usage_errors(tmp_path, runner):
    inp, seeds = tmp_path / "edges.txt", tmp_path / "seeds.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    for extra in (["--exclude-seeds"], ["--exclude-seeds", "--top", "3"], ["--exclude-seeds", "--seed-set", str(seeds)],
                  ["--exclude-seeds", "--seeds", str(seeds), "--top", "3"]):
        res = subprocess.run(base + [str(inp), "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert "--exclude-seeds needs --seed-set and --top" in res.stderr and res.stdout == ""
