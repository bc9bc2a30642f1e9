"""Batched personalised PageRank without a GPU: the pr_batch_* symbols and their NULL-argument
errors, the planner of csrc/pr_batch.h through host/batch_shim.cpp on hand-made row_ptr arrays,
and the --seed-set usage errors of both CLIs (they are raised before any GPU work)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

CLI = os.path.join(PKG_DIR, "build", "pagerank")
STRIDES = [1, 2, 4, 8, 16]
BATCH_FUNCTIONS = ["pr_batch_create", "pr_batch_set_teleport", "pr_batch_set_teleport_sparse", "pr_batch_reset",
                   "pr_batch_step", "pr_batch_sync", "pr_batch_get_ranks", "pr_batch_get_norms", "pr_batch_get_topk",
                   "pr_batch_info", "pr_batch_destroy"]


def test_symbols_and_null_arguments():
    import sparky_hip._lib as L

    lib = L.load()
    for name in BATCH_FUNCTIONS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED
    h = ctypes.c_void_p()
    assert lib.pr_batch_create(None, 4, ctypes.byref(h)) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error() and not h.value
    assert lib.pr_batch_step(None, 1) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    info = np.zeros(6, np.int64)
    assert lib.pr_batch_info(None, ctypes.c_void_p(info.ctypes.data), 6) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    lib.pr_batch_destroy(None)  # no-op


def test_python_class_is_exported():
    import sparky_hip

    assert sparky_hip.PageRankBatch.__name__ == "PageRankBatch"
    for m in ("set_teleport", "set_teleport_sparse", "reset", "step", "ranks", "norms", "topk", "info"):
        assert callable(getattr(sparky_hip.PageRankBatch, m))


# ---- the planner -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_shim.so"))
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.prb_stride.argtypes = [ctypes.c_int]
    lib.prb_unit_cap.argtypes = [ctypes.c_int]
    lib.prb_plan.argtypes = [P, i64, ctypes.c_int, i64, P, P, P, P, P, P, P]
    lib.prb_plan.restype = i64
    return lib


def plan(shim, row_ptr, stride):
    rp = np.ascontiguousarray(row_ptr, np.int64)
    V = len(rp) - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    n_long, n_slots = np.zeros(1, np.int64), np.zeros(1, np.int64)
    cap_units = V + int(rp[-1]) + 1  # never more units than rows + in-links
    e0 = np.zeros(cap_units, np.int64)
    row0, rows, n, slot = (np.zeros(cap_units, np.int32) for _ in range(4))
    nu = shim.prb_plan(p(rp), V, stride, cap_units, p(e0), p(row0), p(rows), p(n), p(slot), p(n_long), p(n_slots))
    assert 0 <= nu <= cap_units
    return dict(e0=e0[:nu], row0=row0[:nu], rows=rows[:nu], n=n[:nu], slot=slot[:nu], n_long=int(n_long[0]),
                n_slots=int(n_slots[0]))


def check_plan(shim, row_ptr, stride):
    """Every in-link exactly once, every row exactly once, chunks consecutive and in order, no
    unit above its capacity.  Returns the plan."""
    rp = np.asarray(row_ptr, np.int64)
    V = len(rp) - 1
    cap = shim.prb_unit_cap(stride)
    max_rows = shim.prb_unit_rows()
    assert cap == (64 // stride) * 64
    pl = plan(shim, rp, stride)
    covered = np.zeros(int(rp[-1]), np.int32)
    row_seen = np.zeros(V, np.int32)
    next_chunk = {}  # long row -> (next chunk index, next in-link, next slot)
    next_row = 0
    for e0, row0, rows, n, slot in zip(pl["e0"], pl["row0"], pl["rows"], pl["n"], pl["slot"]):
        e0, row0, rows, n, slot = int(e0), int(row0), int(rows), int(n), int(slot)
        assert 0 <= n <= cap
        covered[e0:e0 + n] += 1
        if rows > 0:  # PACK: whole consecutive rows
            assert rows <= max_rows and row0 == next_row
            assert e0 == rp[row0] and e0 + n == rp[row0 + rows]
            row_seen[row0:row0 + rows] += 1
            next_row = row0 + rows
        else:  # CHUNK -(k + 1) of a long row
            k = -rows - 1
            deg = int(rp[row0 + 1] - rp[row0])
            assert deg > cap
            if k == 0:
                assert row0 == next_row and row0 not in next_chunk
                next_chunk[row0] = (0, int(rp[row0]), slot)
                row_seen[row0] += 1
                next_row = row0 + 1
            want_k, want_e0, want_slot = next_chunk[row0]
            assert (k, e0, slot) == (want_k, want_e0, want_slot)  # consecutive, in order, slots too
            last = e0 + n == rp[row0 + 1]
            assert n == cap or last  # only the last chunk is short
            next_chunk[row0] = (k + 1, e0 + n, slot + 1)
    assert next_row == V
    assert (covered == 1).all() and (row_seen == 1).all()
    for row, (_, e_end, _) in next_chunk.items():
        assert e_end == rp[row + 1]
    assert pl["n_long"] == len(next_chunk)
    assert pl["n_slots"] == sum(k for k, _, _ in next_chunk.values())
    return pl


@pytest.mark.parametrize("stride", STRIDES)
def test_plan_empty_rows(shim, stride):
    pl = check_plan(shim, np.zeros(1001, np.int64), stride)
    assert len(pl["rows"]) == -(-1000 // shim.prb_unit_rows())  # packed to the row limit
    assert pl["n_long"] == 0
    check_plan(shim, np.zeros(1, np.int64), stride)  # V = 0: no unit
    assert len(plan(shim, np.zeros(1, np.int64), stride)["rows"]) == 0


@pytest.mark.parametrize("stride", STRIDES)
def test_plan_rows_of_one(shim, stride):
    pl = check_plan(shim, np.arange(5001, dtype=np.int64), stride)
    assert (pl["rows"][:-1] > 1).all()  # short rows are packed
    assert len(pl["rows"]) == -(-5000 // min(shim.prb_unit_rows(), shim.prb_unit_cap(stride)))


@pytest.mark.parametrize("stride", STRIDES)
def test_plan_single_long_row(shim, stride):
    pl = check_plan(shim, np.array([0, 100_000], np.int64), stride)
    cap = shim.prb_unit_cap(stride)
    assert pl["n_long"] == 1 and len(pl["rows"]) == -(-100_000 // cap) == pl["n_slots"]
    assert (pl["rows"] < 0).all()
    # exactly the capacity is still one PACK unit; one more in-link splits
    assert check_plan(shim, np.array([0, cap], np.int64), stride)["n_long"] == 0
    assert check_plan(shim, np.array([0, cap + 1], np.int64), stride)["n_slots"] == 2


@pytest.mark.parametrize("stride", STRIDES)
def test_plan_mix(shim, stride):
    rng = np.random.default_rng(7 + stride)
    deg = rng.integers(0, 9, 4000)  # power-law-ish: mostly short rows ...
    deg[rng.integers(0, 4000, 40)] = rng.integers(100, 3000, 40)  # ... some medium ...
    deg[[0, 1999, 3999]] = [70_000, 4097, 12_345]  # ... and hubs at the first, a middle and the last row
    deg[1000:1200] = 0
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    pl = check_plan(shim, rp, stride)
    cap = shim.prb_unit_cap(stride)
    assert pl["n_long"] == int((deg > cap).sum()) >= 3
    packs = pl["rows"][pl["rows"] > 0]
    assert packs.mean() > 4  # many short rows per unit
    # greedy packing: a unit is closed only because the next row would not fit
    pack_i = np.nonzero(pl["rows"] > 0)[0]
    for u in pack_i:
        nxt = int(pl["row0"][u] + pl["rows"][u])
        if nxt < len(deg) and deg[nxt] <= cap:
            assert pl["rows"][u] == shim.prb_unit_rows() or pl["n"][u] + deg[nxt] > cap


def test_stride(shim):
    assert [shim.prb_stride(w) for w in range(1, 17)] == [1, 2, 4, 4, 8, 8, 8, 8] + [16] * 8


# ---- CLI usage errors (before any GPU work) ----------------------------------------------------
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("seedsets")
    inp, seeds = d / "edges.txt", d / "seeds.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    return str(inp), str(seeds)


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_usage_errors(cli_files, runner):
    inp, seeds = cli_files
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    cases = [(["--seeds", seeds, "--seed-set", seeds], "--seeds and --seed-set are exclusive"),
             (["--seed-set", seeds] * 17, "at most 16 seed sets"),
             (["--seed-set", seeds, "--devices", "0,0"], "--seed-set does not combine with --devices"),
             (["--seed-set", seeds, "--resume", "nowhere/PageRank3"], "--seed-set does not combine with"),
             (["--seed-set", seeds, "--save-every-iter", "--out", "nowhere"], "--seed-set does not combine with")]
    for extra, msg in cases:
        res = subprocess.run(base + [inp, "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert msg in res.stderr and res.stdout == ""
