"""The device-side top-K rank query on the GPU: pr_get_topk / pr_group_topk / pr_topk_merge through
PageRankGraph.topk, PartGroup.topk, merge_topk and both CLIs' --top.

Reference for every selection: np.lexsort((ids, -ranks))[:k] over the full vector that the existing
pr_get_ranks returns for the same handle -- rank descending, ties by original ID ascending; IDs
compare for equality, ranks bitwise.  The one strategy switch of the implementation -- histogram
passes over the rows until the candidates are at most rows / narrow_div, then over the compacted
candidates -- is a parameter of the library's internal entry point (PageRankGraph._topk_ex), so
both sides run here at small sizes: narrow_div = 0 never compacts (row passes only), 1 compacts
after the first pass, 8 is what topk() uses; the tests assert from the returned pass counts that
each side was taken (one workgroup: test_selection_on_chosen_values; many workgroups and a
multi-tile grid-stride loop: test_many_workgroups).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "build", "pagerank")
KAT = ["A B", "A C", "A B", "B C", "C A", "C C", "D", "E A", "E F"]  # tests/test_cli_gpu.py


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


def reference(ranks, k, ids=None):
    ids = np.arange(len(ranks), dtype=np.int32) if ids is None else ids
    o = np.lexsort((ids, -ranks[ids]))[: max(k, 0)]
    return ids[o], ranks[ids[o]]


def check(got, want, n_expect):
    gi, gr = got[0], got[1]
    wi, wr = want
    assert len(gi) == len(gr) == n_expect == len(wi)
    assert -1 not in gi and len(np.unique(gi)) == len(gi)
    assert np.array_equal(gi, wi)
    assert np.array_equal(gr.view(np.uint64), wr.view(np.uint64))


def layout_kw(layout):
    return dict(layout="split", options={"classes": 8}) if layout == "split" else dict(layout="fused")


@pytest.mark.parametrize("layout", ["fused", "split"])
def test_selection_on_chosen_values(hip, layout):
    """No iteration: reset(init_ranks=x) with negatives, +0.0, the smallest subnormal, 1e308,
    nextafter(1, 2) and two big tie classes.  The split case (8 classes, 3000 rows) has hole rows,
    which hold 0.0: with negative ranks present and k = V a leaked hole would displace one."""
    V = 3000
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, V, 20000)
    x = rng.random(V) * 4.0
    u = rng.random(V)
    x[u < 0.4] = 0.15
    x[(u >= 0.4) & (u < 0.6)] = 1.0
    sp = rng.permutation(V)[:60]
    x[sp[:20]] = -rng.random(20) * 3.0
    x[sp[20:30]] = 0.0
    x[sp[30:40]] = 5e-324
    x[sp[40:50]] = 1e308
    x[sp[50:60]] = np.nextafter(1.0, 2.0)
    with hip.PageRankGraph(V, src, dst, **layout_kw(layout)) as g:
        inf = g.info()
        if layout == "split":
            assert inf["layout"] == 1 and inf["classes"] == 8
        g.reset(init_ranks=x)
        full = g.ranks().copy()
        assert np.array_equal(full.view(np.uint64), x.view(np.uint64))
        sides = set()
        for k in [0, 1, 2, 63, 64, 65, 1000, V - 1, V, V + 5]:
            want = reference(full, k)
            check(g.topk(k), want, min(k, V))
            for div in (0, 1):
                gi, gr, info = g._topk_ex(k, div)
                check((gi, gr), want, min(k, V))
                assert info["passes"] == info["row_passes"] + info["cand_passes"] <= 12
                if div == 0:
                    assert info["cand_passes"] == 0 and info["narrowed_at"] == -1
                sides.add((div, info["cand_passes"] > 0))
        assert (1, True) in sides and (0, False) in sides


@pytest.mark.parametrize("layout", ["fused", "split"])
def test_threshold_inside_a_tie_class(hip, layout):
    """64 hubs in a ring, every other vertex links to hub i % 64: after 10 iterations the 4096
    vertices without in-links tie bit-exactly, and the K-th vertex falls inside that class."""
    V = 4160
    hubs = np.arange(64)
    rest = np.arange(64, V)
    src = np.concatenate([hubs, rest]).astype(np.int32)
    dst = np.concatenate([(hubs + 1) % 64, rest % 64]).astype(np.int32)
    with hip.PageRankGraph(V, src, dst, **layout_kw(layout)) as g:
        g.reset()
        g.step(10)
        full = g.ranks().copy()
        assert len(np.unique(full[64:].view(np.uint64))) == 1
        for k in [1, 64, 65, 1000, 4159]:
            want = reference(full, k)
            got = g.topk(k)
            check(got, want, k)
            if k == 1000:  # more vertices share the K-th value than were selected
                kth = got[1][-1]
                assert np.sum(full == kth) > np.sum(got[1] == kth) > 0
            check(g._topk_ex(k, 0)[:2], want, k)
            check(g._topk_ex(k, 1)[:2], want, k)


def test_many_workgroups(hip):
    """V = 300 000 (split layout): hundreds of workgroups, several grid-stride tiles with the
    compacted candidates on both sides of the switch."""
    V, E = 300_000, 2_000_000
    rng = np.random.default_rng(9)
    src, dst = random_edges(rng, V, E, hub_frac=0.02)
    with hip.PageRankGraph(V, src, dst, layout="split") as g:
        assert g.info()["layout"] == 1
        g.reset()
        g.step(5)
        full = g.ranks().copy()
        sides = set()
        for k in [1, 100, 100_000, V]:
            want = reference(full, k)
            check(g.topk(k), want, k)
            for div in (0, 1, 8):
                gi, gr, info = g._topk_ex(k, div)
                check((gi, gr), want, k)
                sides.add((div > 0, info["cand_passes"] > 0))
                if k < V:
                    assert info["row_passes"] >= 1
        assert (True, True) in sides and (False, False) in sides


def test_parts(hip):
    """Three parts on one device: a part answers for the rows it owns; the group call and the
    host merge of the three lists answer for the graph."""
    V, P = 50_000, 3
    rng = np.random.default_rng(13)
    src, dst = random_edges(rng, V, 400_000, hub_frac=0.01)
    parts = [hip.PageRankGraph(V, src, dst, part=p, n_parts=P, keep_canonical=False) for p in range(P)]
    try:
        grp = hip.PartGroup(parts)
        grp.reset()
        grp.step(4)
        grp.sync()
        full = grp.ranks().copy()
        assert not np.isnan(full).any()
        owned = []
        for g in parts:
            mine = np.full(V, np.nan)
            g.ranks(mine)
            owned.append(np.nonzero(~np.isnan(mine))[0].astype(np.int32))
        assert sum(len(o) for o in owned) == V
        for k in [1, 100, 20_000, V]:
            lists = []
            for g, ids in zip(parts, owned):
                got = g.topk(k)
                check(got, reference(full, k, ids), min(k, len(ids)))
                lists.append(got)
            want = reference(full, k)
            check(grp.topk(k), want, k)
            check(hip.merge_topk(lists, k), want, k)
    finally:
        for g in parts:
            g.close()


def test_no_side_effect(hip):
    V = 20_000
    rng = np.random.default_rng(17)
    src, dst = random_edges(rng, V, 150_000, hub_frac=0.01)
    with hip.PageRankGraph(V, src, dst) as a, hip.PageRankGraph(V, src, dst) as b:
        bytes0 = a.info()["device_bytes"]
        a.reset()
        a.step(3)
        assert a.info()["device_bytes"] == bytes0
        t1 = a.topk(100)
        bytes1 = a.info()["device_bytes"]
        assert bytes1 > bytes0
        check(t1, reference(a.ranks().copy(), 100), 100)
        t2 = a.topk(100)
        assert a.info()["device_bytes"] == bytes1
        assert np.array_equal(t1[0], t2[0]) and np.array_equal(t1[1].view(np.uint64), t2[1].view(np.uint64))
        a.step(3)
        b.reset()
        b.step(6)
        assert np.array_equal(a.ranks().view(np.uint64), b.ranks().view(np.uint64))
        assert a.stats()["iters"] == 6
        assert b.info()["device_bytes"] == bytes0


def test_state_and_argument_errors(hip):
    from sparky_hip import _lib

    with hip.PageRankGraph(3, np.array([0, 1], np.int32), np.array([1, 2], np.int32)) as g:
        with pytest.raises(hip.PageRankError) as ei:
            g.topk(2)
        assert ei.value.code == _lib.PR_ERR_STATE
        g.reset()
        with pytest.raises(hip.PageRankError) as ei:
            g.topk(-1)
        assert ei.value.code == _lib.PR_ERR_INVALID
        ids, ranks = g.topk(0)
        assert len(ids) == 0 and len(ranks) == 0
        ids, ranks = g.topk(5)
        assert list(ids) == [0, 1, 2] and list(ranks) == [1.0, 1.0, 1.0]


TOP3 = ["C has rank: 1.9916666666666665.", "A has rank: 1.1416666666666666.", "D has rank: 1.1416666666666666."]


def _base(runner):
    return [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_top(tmp_path, runner):
    """The known-answer edge list, 1 iteration, --top 3: A, D and E tie, first appearance wins."""
    inp = tmp_path / "edges.txt"
    inp.write_text("\n".join(KAT) + "\n")
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    res = subprocess.run(_base(runner) + [str(inp), "1", "--top", "3"], capture_output=True, text=True, env=env,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.splitlines() == ["Starting iter0"] + TOP3
    out_dir = tmp_path / "out"
    res = subprocess.run(_base(runner) + [str(inp), "1", "--top", "3", "--out", str(out_dir)], capture_output=True,
                         text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.splitlines() == ["Starting iter0"] + TOP3
    part = (out_dir / "PageRank0" / "part-00000").read_text().splitlines()
    assert sorted(ln[1:].split(",")[0] for ln in part) == ["A", "B", "C", "D", "E", "F"]
    if runner == "cpp":  # --quiet still suppresses the listing (one host is enough: keeps the case short)
        res = subprocess.run(_base(runner) + [str(inp), "1", "--top", "3", "--quiet"], capture_output=True, text=True,
                             env=env, timeout=120)
        assert res.returncode == 0 and res.stdout.splitlines() == ["Starting iter0"]
    res = subprocess.run(_base(runner) + [str(inp), "1", "--top", "0"], capture_output=True, text=True, env=env,
                         timeout=120)
    assert res.returncode == 2 and "--top" in res.stderr


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_top_devices_group(tmp_path, runner):
    inp = tmp_path / "edges.txt"
    inp.write_text("\n".join(KAT) + "\n")
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    res = subprocess.run(_base(runner) + [str(inp), "1", "--devices", "0,0", "--top", "3"], capture_output=True,
                         text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "Starting iter0" and len(lines) == 4
    for got, want in zip(lines[1:], TOP3):
        gu, gr = got.rsplit(" has rank: ", 1)
        wu, wr = want.rsplit(" has rank: ", 1)
        assert gu == wu and abs(float(gr[:-1]) - float(wr[:-1])) <= 1e-9
