"""pr_batch_step_until_any / pr_batch_run_queue without a GPU: the symbols and their host-side
argument checks, the stop rule and the scheduler of csrc/pr_batch_queue.h through
host/batch_queue_shim.cpp.

The scheduler is checked against a short Python model (model() below) for random per-query iteration
counts: the column of every query, the completion order, every pr_batch_step_until_any call it
issues (mask and cap) and the total of the iterations."""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG_DIR


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_symbols_and_null_batch():
    import sparky_hip._lib as L

    lib = L.load()
    for name in ("pr_batch_reset_column", "pr_batch_step_until_any", "pr_batch_run_queue"):
        assert hasattr(lib, name) and name in L.EXPORTED
    assert hasattr(lib, "pr_batch_step_until_any_ex") and "pr_batch_step_until_any_ex" not in L.EXPORTED
    ex, conv = ctypes.c_int32(7), ctypes.c_uint32(7)
    assert lib.pr_batch_reset_column(None, 0, None) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_step_until_any(None, 1, 10, 1e-6, ctypes.byref(ex), ctypes.byref(conv)) == L.PR_ERR_INVALID
    info = np.zeros(2, np.int32)
    assert lib.pr_batch_step_until_any_ex(None, 1, 10, 1e-6, 4, ctypes.byref(ex), ctypes.byref(conv),
                                          _p(info)) == L.PR_ERR_INVALID
    assert lib.pr_batch_run_queue(None, 0, None, 10, 1e-6, None, None, None) == L.PR_ERR_INVALID


def test_python_methods():
    import sparky_hip

    for m in ("reset_column", "step_until_any", "_step_until_any_ex", "run_queue"):
        assert callable(getattr(sparky_hip.PageRankBatch, m))


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_queue_shim.so"))
    lib.prq_decide.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                               ctypes.c_void_p]
    lib.prq_decide.restype = ctypes.c_uint32
    i32, P = ctypes.c_int32, ctypes.c_void_p
    lib.prq_simulate.argtypes = [i32, P, i32, i32, P, P, P, P, P, i32, P]
    lib.prq_simulate.restype = ctypes.c_int
    return lib


def decide(shim, mask, l1, tol, width):
    """(mask of the next launch, saved, converged)"""
    a = np.zeros(16, np.float64)
    a[:len(l1)] = l1
    saved, conv = ctypes.c_uint32(0), ctypes.c_uint32(0)
    nxt = shim.prq_decide(mask, _p(a), tol, width, ctypes.byref(saved), ctypes.byref(conv))
    return nxt, saved.value, conv.value


# ---- the stop rule -----------------------------------------------------------------------------
def test_state(shim):
    assert shim.prq_state_bytes() == 8 and shim.prq_block() >= 1


def test_any_converged_stops(shim):
    tol = 1e-6
    # nothing within tol: the mask stays, nothing is recorded
    assert decide(shim, 0b111, [1.0, 2e-6, np.nextafter(1e-6, 1.0)], tol, 3) == (0b111, 0, 0)
    # one column: stop, the mask is parked
    assert decide(shim, 0b111, [1.0, 1e-6, 1.0], tol, 3) == (0, 0b111, 0b010)
    # several in the same iteration
    assert decide(shim, 0b1111, [0.0, 1.0, 5e-7, 1e-6], tol, 4) == (0, 0b1111, 0b1101)
    assert decide(shim, 0, [0.0] * 16, tol, 16) == (0, 0, 0)


def test_nan_never_converges(shim):
    for tol in (0.0, 1e-6, 1e300):
        assert decide(shim, 0b11, [np.nan, -np.nan], tol, 2) == (0b11, 0, 0)
    assert decide(shim, 0b111, [np.nan, np.inf, 0.0], 1e300, 3) == (0, 0b111, 0b100)


def test_tol_zero_needs_exact_zero(shim):
    tiny = np.nextafter(0.0, 1.0)
    assert decide(shim, 0b11, [tiny, 1e-300], 0.0, 2) == (0b11, 0, 0)
    assert decide(shim, 0b1111, [0.0, tiny, -0.0, 1e-300], 0.0, 4) == (0, 0b1111, 0b0101)


def test_bits_outside_active_never_appear(shim):
    # columns 1 and 3 are not active: their L1 (stale, tiny) cannot stop the call or show up
    assert decide(shim, 0b0101, [1.0, 0.0, 1.0, 0.0], 1e-6, 4) == (0b0101, 0, 0)
    assert decide(shim, 0b0101, [1.0, 0.0, 1e-9, 0.0], 1e-6, 4) == (0, 0b0101, 0b0100)
    rng = np.random.default_rng(5)
    for _ in range(300):
        mask = int(rng.integers(0, 1 << 16))
        width = int(rng.integers(1, 17))
        l1 = rng.choice([0.0, 1e-9, 1e-6, 1e-3, np.nan, np.inf], 16)
        nxt, saved, conv = decide(shim, mask, l1, 1e-6, width)
        want = sum(1 << j for j in range(width) if (mask >> j) & 1 and l1[j] <= 1e-6)
        assert conv == want and conv & ~mask == 0 and conv >> width == 0
        assert (nxt, saved) == ((0, mask) if want else (mask, 0))


@pytest.mark.parametrize("width", [1, 3, 8, 16])
def test_bits_at_or_above_width_never_appear(shim, width):
    nxt, saved, conv = decide(shim, 0xffffffff, [0.0] * 16, 1e-6, width)
    assert conv == (1 << width) - 1 and nxt == 0
    # only columns at or above width are within tol: no stop
    l1 = [1.0] * width + [0.0] * (16 - width)
    assert decide(shim, 0xffffffff, l1, 1e-6, width) == (0xffffffff, 0, 0)


# ---- the scheduler -----------------------------------------------------------------------------
def model(need, width, cap):
    """The schedule in Python.  need[q]: the iteration in which query q converges (> cap: never).
    Returns (column per query, iterations per query, converged per query, completion order,
    [(mask, cap, executed)], total iterations)."""
    Q = len(need)
    slot, age, nxt = [None] * width, [0] * width, 0
    col, its, conv, order, calls = [None] * Q, [None] * Q, [None] * Q, [], []
    while len(order) < Q:
        for j in range(width):  # free columns take the next queries, in column order
            if slot[j] is None and nxt < Q:
                slot[j], age[j], col[nxt] = nxt, 0, j
                nxt += 1
        occ = [j for j in range(width) if slot[j] is not None]
        c = min(cap - age[j] for j in occ)
        n = min(c, min(need[slot[j]] - age[j] for j in occ))
        calls.append((sum(1 << j for j in occ), c, n))
        for j in occ:  # ascending column order
            age[j] += n
            q = slot[j]
            if age[j] == need[q] or age[j] >= cap:
                its[q], conv[q] = age[j], int(age[j] == need[q])
                order.append(q)
                slot[j] = None
    return col, its, conv, order, calls, sum(n for _, _, n in calls)


@pytest.mark.parametrize("width", [1, 3, 16])
@pytest.mark.parametrize("Q", [0, 1, 5, 16, 17, 40])
def test_schedule_matches_model(shim, Q, width):
    rng = np.random.default_rng(100 * Q + width)
    hit = 0
    for trial in range(6):
        cap = int(rng.integers(1, 60))
        need = rng.integers(1, 80, Q).astype(np.int32)  # some above the cap: those queries hit it
        if Q and trial == 0:
            need[rng.integers(0, Q)] = cap  # converges exactly at the cap
        if Q > 1 and trial == 1:
            need[:] = need[0]  # everything finishes together
        col, its, conv, order = (np.full(max(Q, 1), -1, np.int32) for _ in range(4))
        calls = np.zeros(3 * (Q + 1), np.int32)
        total = ctypes.c_int64(-1)
        n_calls = shim.prq_simulate(Q, _p(need), width, cap, _p(col), _p(its), _p(conv), _p(order), _p(calls), Q + 1,
                                    ctypes.byref(total))
        w_col, w_its, w_conv, w_order, w_calls, w_total = model(need.tolist(), width, cap)
        assert n_calls == len(w_calls)  # at least one query leaves per call: never more than Q calls
        assert col[:Q].tolist() == w_col and its[:Q].tolist() == w_its and conv[:Q].tolist() == w_conv
        assert order[:Q].tolist() == w_order
        assert [tuple(calls[3 * i:3 * i + 3].tolist()) for i in range(n_calls)] == w_calls
        assert total.value == w_total
        # what the contract promises, independent of the model
        assert col[:min(Q, width)].tolist() == list(range(min(Q, width)))  # query q starts in column q
        want_its = np.minimum(need, cap)
        assert its[:Q].tolist() == want_its.tolist() and conv[:Q].tolist() == (need <= cap).astype(int).tolist()
        for mask, c, n in w_calls:
            assert 1 <= n <= c <= cap and mask >> width == 0 and mask != 0
        hit += int((need > cap).sum())
    assert Q < 5 or hit > 0  # some queries did hit the cap


def test_schedule_caps_are_hit(shim):
    """A query that never converges leaves at exactly max_iterations, whatever ran beside it, and
    the queries beside it are not cut short by its cap."""
    need = np.array([100, 3, 7, 100, 2], np.int32)
    Q, width, cap = 5, 2, 10
    col, its, conv, order = (np.zeros(Q, np.int32) for _ in range(4))
    calls = np.zeros(3 * (Q + 1), np.int32)
    total = ctypes.c_int64(0)
    n = shim.prq_simulate(Q, _p(need), width, cap, _p(col), _p(its), _p(conv), _p(order), _p(calls), Q + 1,
                          ctypes.byref(total))
    assert its.tolist() == [10, 3, 7, 10, 2] and conv.tolist() == [0, 1, 1, 0, 1]
    assert col.tolist() == [0, 1, 1, 0, 1]
    assert order.tolist() == [1, 0, 2, 4, 3]
    got = [tuple(calls[3 * i:3 * i + 3].tolist()) for i in range(n)]
    # (mask, cap, executed): q1 done at 3; q0 at its cap 10 (q2 then has 7 = converged in the same call);
    # q3 + q4; q3 alone
    assert got == [(3, 10, 3), (3, 7, 7), (3, 10, 2), (1, 8, 8)]
    assert total.value == 20


# ---- CLI usage errors (before any GPU work) ----------------------------------------------------
CLI = os.path.join(PKG_DIR, "build", "pagerank")


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("queue")
    inp, seeds, lst = d / "edges.txt", d / "seeds.txt", d / "queue.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    lst.write_text(f"# two sets\n{seeds}\n\n{seeds}\n")
    return str(inp), str(seeds), str(lst)


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_seed_queue_usage_errors(cli_files, runner):
    import subprocess
    import sys

    inp, seeds, lst = cli_files
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    ok = ["--seed-queue", lst, "--tol", "1e-6", "--top", "2"]
    needs = "--seed-queue needs --tol and --top"
    excl = "--seed-queue does not combine with --seeds, --seed-set, --devices, --resume or --save-every-iter"
    slots = "--slots takes a count W in 1..16"
    cases = [(["--seed-queue", lst], needs),
             (["--seed-queue", lst, "--tol", "1e-6"], needs),
             (["--seed-queue=" + lst, "--top", "2"], needs),
             (ok + ["--seeds", seeds], excl),
             (ok + ["--seed-set", seeds], excl),
             (ok + ["--devices", "0,0"], excl),
             (ok + ["--resume", "x/PageRank3"], excl),
             (ok + ["--save-every-iter"], excl),
             (ok + ["--slots", "0"], slots),
             (ok + ["--slots", "17"], slots),
             (ok + ["--slots=abc"], slots),
             (ok + ["--slots", "-1"], slots),
             (ok + ["--tol", "nan"], "--tol: not a finite number >= 0"),
             (["--slots", "4"], "--slots needs --seed-queue"),
             (["--slots", "4", "--seed-set", seeds], "--slots needs --seed-queue")]
    for extra, msg in cases:
        res = subprocess.run(base + [inp, "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert msg in res.stderr and res.stdout == "", (extra, res.stderr)
    # the cap of every set is at least one iteration
    res = subprocess.run(base + [inp, "0", *ok], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 2 and "--seed-queue: iterations" in res.stderr and res.stdout == ""
    # a list file that does not exist, and one that names a bad seed file: status 2, no GPU work
    res = subprocess.run(base + [inp, "3", "--seed-queue", lst + ".missing", "--tol", "1e-6", "--top", "2"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 2 and "cannot open the list file" in res.stderr and res.stdout == ""
    bad = lst + ".bad"
    with open(bad, "w") as f:
        f.write(f"{seeds}\n{seeds}.missing\n")
    res = subprocess.run(base + [inp, "3", "--seed-queue", bad, "--tol", "1e-6", "--top", "2"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 2 and "--seed-queue " + seeds + ".missing" in res.stderr and res.stdout == ""
    # --seed-set keeps its limit of 16
    res = subprocess.run(base + [inp, "3"] + ["--seed-set", seeds] * 17, capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 2 and "--seed-set: at most 16 seed sets" in res.stderr
