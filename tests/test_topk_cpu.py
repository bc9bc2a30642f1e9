"""CPU checks of the top-K rank query (pr_get_topk): everything that needs no GPU.

The arithmetic of the device select lives in csrc/pr_topk.h, which the library and this test's
shim (host/topk_shim.cpp) compile alike: the order-preserving map of a rank's IEEE-754 bits to a
u64, the digits of the composite key (rank key, ~original ID), the bin choice, and the driver of
the MSD radix select.  The shim's host model runs that driver with the pass structure of
csrc/pr_topk.hip (histogram passes over the rows, then over the compacted candidates, then the
emit pass).  Reference for every selection: np.lexsort((ids, -ranks))[:k] -- rank descending,
ties by original ID ascending.  pr_topk_merge and the argument checks of pr_get_topk /
pr_group_topk run in libpagerank_hip itself, which loads without a GPU; the writer of the
listing runs in libpagerank_host.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pagerank-using-apache-spark_amd")
SHIM = os.path.join(PKG, "build", "libpr_topk_shim.so")


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def shim():
    # always: make's dependency on pr_topk.h rebuilds a stale shim after an edit
    subprocess.run(["make", "-s", "-C", os.path.join(PKG, "host")], check=True)
    lib = ctypes.CDLL(SHIM)
    P_, u64, u32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
    lib.prt_rank_key.argtypes = [u64]
    lib.prt_rank_key.restype = u64
    lib.prt_rank_bits.argtypes = [u64]
    lib.prt_rank_bits.restype = u64
    lib.prt_rank_keys.argtypes = [P_, i64, P_]
    lib.prt_rank_keys.restype = None
    lib.prt_digit.argtypes = [u64, u32, ctypes.c_int]
    lib.prt_digit.restype = u32
    lib.prt_match.argtypes = [u64, u32, u64, u32, ctypes.c_int]
    lib.prt_choose_bin.argtypes = [P_, u64, P_]
    lib.prt_select.argtypes = [P_, P_, i64, i64, i64, P_, P_, P_]
    lib.prt_select.restype = i64
    return lib


def keys_of(shim, x):
    bits = np.ascontiguousarray(x, np.float64).view(np.uint64)
    out = np.zeros(bits.shape, np.uint64)
    shim.prt_rank_keys(_p(bits), bits.shape[0], _p(out))
    return out


EDGE = [0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, np.nextafter(1.0, 2.0), 1.797e308, -1.797e308, np.inf, -np.inf]


def test_key_map_orders_like_the_numbers(shim):
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2**64, 100_000, dtype=np.uint64).view(np.float64)
    x = np.concatenate([x[~np.isnan(x)], np.array(EDGE)])
    k = keys_of(shim, x)
    # key order == numeric order: equal keys only for equal bits, and sorting by key sorts the values
    o = np.argsort(k, kind="stable")
    xs = x[o]
    assert np.all(xs[:-1] <= xs[1:])
    assert len(np.unique(k)) == len(np.unique(x.view(np.uint64)))  # distinct bits, distinct keys
    # strictly: a < b  =>  key(a) < key(b), on the edge values against everything
    e = np.array(EDGE)
    ke = keys_of(shim, e)
    for i in range(len(e)):
        assert np.all(k[x < e[i]] < ke[i]) and np.all(k[x > e[i]] > ke[i])
    # -0.0 sorts just below +0.0: adjacent keys
    assert shim.prt_rank_key(0x8000000000000000) + 1 == shim.prt_rank_key(0)
    # the map is a bijection: the returned ranks are the bits that went in
    bits = x.view(np.uint64)
    back = np.array([shim.prt_rank_bits(int(v)) for v in k[:2000]], np.uint64)
    assert np.array_equal(back, bits[:2000])


def test_digits_and_prefix(shim):
    hi, lo = 0x0123456789ABCDEF, 0xA1B2C3D4
    want = [0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF, 0xA1, 0xB2, 0xC3, 0xD4]
    assert [shim.prt_digit(hi, lo, p) for p in range(12)] == want
    for p in range(13):
        assert shim.prt_match(hi, lo, hi, lo, p)
    for p in range(12):  # a difference in digit p shows from prefix length p + 1 on
        if p < 8:
            h2, l2 = hi ^ (1 << (56 - 8 * p)), lo
        else:
            h2, l2 = hi, lo ^ (1 << (24 - 8 * (p - 8)))
        assert [bool(shim.prt_match(h2, l2, hi, lo, q)) for q in range(13)] == [q <= p for q in range(13)]
    hist = np.zeros(256, np.uint32)
    hist[[3, 200, 255]] = [10, 5, 2]
    above = ctypes.c_uint64()
    for need, b, ab in [(1, 255, 0), (2, 255, 0), (3, 200, 2), (7, 200, 2), (8, 3, 7), (17, 3, 7)]:
        assert shim.prt_choose_bin(_p(hist), need, ctypes.byref(above)) == b and above.value == ab


def tie_heavy(n, seed, holes=True):
    rng = np.random.default_rng(seed)
    r = rng.random(n) * 3.0
    u = rng.random(n)
    r[u < 0.4] = 0.15
    r[(u >= 0.4) & (u < 0.6)] = 1.0
    r[rng.integers(0, n, 20)] = -rng.random(20)  # a few negatives below every tie class
    ids = rng.permutation(n).astype(np.int32)
    if holes:
        h = rng.random(n) < 0.03
        ids[h] = -1
        r[h] = 0.0  # what a hole row holds
    return r, ids


def lexsort_ref(r, ids, k):
    own = np.nonzero(ids >= 0)[0]
    o = own[np.lexsort((ids[own], -r[own]))][: max(k, 0)]
    return ids[o], r[o]


@pytest.mark.parametrize("narrow_div", [8, 0, 1])
def test_host_model_equals_lexsort(shim, narrow_div):
    n = 50_000
    r, ids = tie_heavy(n, 7)
    seen = set()
    for k in [0, 1, 63, 64, 65, 1000, n - 1, n, n + 5]:
        oi, orr = np.zeros(n + 8, np.int32), np.zeros(n + 8, np.float64)
        info = np.zeros(4, np.int32)
        m = shim.prt_select(_p(r), _p(ids), n, k, narrow_div, _p(oi), _p(orr), _p(info))
        wi, wr = lexsort_ref(r, ids, k)
        assert m == len(wi) == min(k, int(np.sum(ids >= 0)))
        assert np.array_equal(oi[:m], wi) and -1 not in oi[:m]
        assert np.array_equal(orr[:m].view(np.uint64), wr.view(np.uint64))
        assert info[0] == info[1] + info[2] and info[0] <= 12
        if narrow_div == 0:
            assert info[2] == 0 and info[3] == -1
        seen.add(int(info[3]) >= 0)
    if narrow_div:
        assert True in seen  # the compacted-candidate passes ran for some k


def test_host_model_threshold_deep_in_a_tie_class(shim):
    """All ranks equal: the K-th key is decided by the ID digits alone (passes 8..11)."""
    n = 5000
    r = np.full(n, 0.15)
    ids = np.random.default_rng(3).permutation(n).astype(np.int32)
    for k in [1, 255, 256, 257, 4999]:
        oi, orr, info = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(4, np.int32)
        assert shim.prt_select(_p(r), _p(ids), n, k, 8, _p(oi), _p(orr), _p(info)) == k
        assert np.array_equal(oi[:k], np.arange(k, dtype=np.int32)) and info[0] > 8


# ---- libpagerank_hip without a GPU: the merge and the argument checks -------------------------------

def test_merge_equals_lexsort_of_the_union():
    import sparky_hip

    rng = np.random.default_rng(11)
    for n_lists in (1, 3, 8):
        V = 4000
        r = rng.random(V)
        r[rng.random(V) < 0.5] = 0.15  # ties across lists resolve by ID
        owner = rng.integers(0, n_lists, V)
        owner[owner == 1] = 0  # list 1 (when there is one) stays empty
        lists = []
        for l in range(n_lists):
            ids = np.nonzero(owner == l)[0].astype(np.int32)
            o = np.lexsort((ids, -r[ids]))
            lists.append((ids[o], r[ids][o]))
        allid = np.arange(V, dtype=np.int32)
        for k in (0, 1, 100, V, V + 7):
            gi, gr = sparky_hip.merge_topk(lists, k)
            o = np.lexsort((allid, -r))[:k]
            assert np.array_equal(gi, allid[o]) and np.array_equal(gr.view(np.uint64), r[o].view(np.uint64))
    gi, gr = sparky_hip.merge_topk([], 5)
    assert len(gi) == 0 and len(gr) == 0


def test_merge_and_query_argument_errors():
    import sparky_hip
    import sparky_hip._lib as L

    lib = L.load()
    n = ctypes.c_int32(-7)
    ids, rk = np.zeros(4, np.int32), np.zeros(4, np.float64)
    a, b = np.array([1, 2], np.int32), np.array([0.5, 0.25])
    pid, prk = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_void_p * 1)(b.ctypes.data)
    cnt = np.array([2], np.int32)
    ok = lib.pr_topk_merge(1, pid, prk, _p(cnt), 4, _p(ids), _p(rk), ctypes.byref(n))
    assert ok == L.PR_OK and n.value == 2 and list(ids[:2]) == [1, 2]
    assert lib.pr_topk_merge(1, pid, prk, _p(cnt), -1, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(-1, pid, prk, _p(cnt), 4, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(1, None, prk, _p(cnt), 4, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(1, pid, prk, None, 4, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(1, pid, prk, _p(cnt), 4, None, _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(1, pid, prk, _p(cnt), 4, _p(ids), _p(rk), None) == L.PR_ERR_INVALID
    bad = np.array([-2], np.int32)
    assert lib.pr_topk_merge(1, pid, prk, _p(bad), 4, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    nul = (ctypes.c_void_p * 1)(None)
    assert lib.pr_topk_merge(1, nul, prk, _p(cnt), 4, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_merge(1, pid, prk, _p(cnt), 0, None, None, ctypes.byref(n)) == L.PR_OK and n.value == 0
    # no GPU needed: a NULL handle / group is rejected before any device work
    assert lib.pr_get_topk(None, 3, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_group_topk(None, 2, 3, _p(ids), _p(rk), ctypes.byref(n)) == L.PR_ERR_INVALID
    assert lib.pr_topk_select_ex(None, 3, 8, _p(ids), _p(rk), ctypes.byref(n), None) == L.PR_ERR_INVALID
    with pytest.raises(ValueError):
        sparky_hip.merge_topk([(a, b[:1])], 2)


# ---- libpagerank_host: the listing of a top-K list ---------------------------------------------------

def test_write_has_rank_ids(tmp_path):
    import sparky_hip

    e = sparky_hip.HostEdges.parse(b"A B\nA C\nB C\nD\n")
    assert e.names() == ["A", "B", "C", "D"]
    ids = np.array([2, 0, 3, 0], np.int32)
    ranks = np.array([1.9916666666666665, 1.0, 5e-324, 1e7])
    path = tmp_path / "top.txt"
    e.write_has_rank_ids(str(path), ids, ranks)
    want = ["C has rank: 1.9916666666666665.", "A has rank: 1.0.", "D has rank: 4.9E-324.", "A has rank: 1.0E7."]
    assert path.read_text().splitlines() == want
    assert [f"{u} has rank: {sparky_hip.java_double_to_string(float(r))}." for u, r in zip("CADA", ranks)] == want
    e.write_has_rank_ids(str(path), ids[:0], ranks[:0])
    assert path.read_text() == ""
    for bad in (4, -1, 2**31 - 1):
        path.write_text("kept")
        with pytest.raises(sparky_hip.HostError) as ei:
            e.write_has_rank_ids(str(path), np.array([1, bad], np.int32), ranks[:2])
        assert "out of range" in str(ei.value) and path.read_text() == "kept"
    with pytest.raises(ValueError):
        e.write_has_rank_ids(str(path), ids, ranks[:2])
    e.close()
