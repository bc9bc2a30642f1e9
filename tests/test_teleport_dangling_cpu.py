"""The engine's teleport dangling mode (pr_set_teleport_dangling) without a GPU: the block-order sum of
csrc/pr_tele_sum.h through host/tele_sum_shim.cpp (built with -ffp-contract=off) against a numpy model
bit for bit, the new symbols and their argument checks on a NULL handle, the --dangling=seeds usage
errors of both CLIs (raised before any GPU work), and the exact model of
tests/exact_dangling_model.py against the same iteration in float64."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exact_dangling_model as edm
import exact_model as em
from conftest import PKG_DIR, ROOT

CLI = os.path.join(PKG_DIR, "build", "pagerank")
BLOCK = 1024
SIZES = [1, 1023, 1024, 1025, 2048, 5000]


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- 1. the block-order sum -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_tele_sum_shim.so"))
    d, ll, p = ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p
    lib.prts_block.argtypes, lib.prts_block.restype = [], ll
    lib.prts_dense.argtypes, lib.prts_dense.restype = [p, ll], d
    lib.prts_sparse.argtypes, lib.prts_sparse.restype = [ll, ll, p, p, d], d
    return lib


def model_sum(t):
    """Blocks of 1024 consecutive IDs, each added in order from +0.0; the block sums added in order."""
    t = np.asarray(t, np.float64)
    ts = np.float64(0.0)
    for b0 in range(0, t.size, BLOCK):
        acc = np.float64(0.0)
        for x in t[b0:b0 + BLOCK]:
            acc = acc + x
        ts = ts + acc
    return ts


def dense(shim, t):
    t = np.ascontiguousarray(t, np.float64)
    return shim.prts_dense(t.ctypes.data, t.size)


def sparse(shim, V, ids, values, rest):
    order = np.argsort(ids)
    ids = np.ascontiguousarray(np.asarray(ids, np.int32)[order])
    values = np.ascontiguousarray(np.asarray(values, np.float64)[order])
    return shim.prts_sparse(V, ids.size, ids.ctypes.data, values.ctypes.data, float(rest))


def test_block_is_1024(shim):
    assert shim.prts_block() == BLOCK


@pytest.mark.parametrize("V", SIZES)
def test_dense_sum_is_the_block_order_sum(shim, V):
    rng = np.random.default_rng(V)
    for t in (rng.uniform(-1.0, 1.0, V), rng.uniform(0.0, 1.0, V) * 10.0 ** rng.integers(-8, 8, V), np.full(V, 0.1),
              np.zeros(V), np.full(V, -0.0)):
        assert bits(dense(shim, t))[0] == bits(model_sum(t))[0], V


def seed_cases(V, rng):
    """Seed sets with seeds in the first, last and partial block, in every block, alone, and none."""
    last_full = (V // BLOCK) * BLOCK  # start of the partial block (== V when there is none)
    cases = [np.array([], np.int64), np.array([0]), np.array([V - 1])]
    cases.append(np.unique(rng.integers(0, min(V, BLOCK), 5)))  # the first block
    if last_full < V:
        cases.append(np.unique(rng.integers(last_full, V, 3)))  # the partial block
    if V > BLOCK:
        cases.append(np.unique(rng.integers(max(0, last_full - BLOCK), last_full, 4)))  # the last full block
        cases.append(np.unique(np.concatenate([[0, BLOCK - 1, BLOCK, V - 1], rng.integers(0, V, 7)])))
        cases.append(np.arange(0, V, BLOCK))  # one seed in every block
    cases.append(np.unique(rng.integers(0, V, min(V, 300))))
    return cases


@pytest.mark.parametrize("V", SIZES)
def test_sparse_sum_has_the_bits_of_the_dense_vector(shim, V):
    rng = np.random.default_rng(100 + V)
    for rest in (0.1, 0.0, 1.0 / 3.0, -0.0, 0.15):  # 0.1 and 1/3: the 1024-fold sum is inexact
        for ids in seed_cases(V, rng):
            values = rng.uniform(-2.0, 2.0, ids.size) * 10.0 ** rng.integers(-6, 6, ids.size)
            t = np.full(V, rest)
            t[ids] = values
            want = model_sum(t)
            perm = rng.permutation(ids.size)  # the shim sorts, as the library does
            got = sparse(shim, V, ids[perm], values[perm], rest)
            assert bits(got)[0] == bits(want)[0] == bits(dense(shim, t))[0], (V, rest, ids[:5])
    acc = np.float64(0.0)
    for _ in range(BLOCK):
        acc = acc + np.float64(0.1)
    assert acc != np.float64(0.1) * BLOCK  # the case the issue names: a repeated sum is not a product


def test_the_exact_tests_vector_sums_to_8(shim):
    for name in em.WITH_SINKS:
        inp = em.DYADIC_BUILDERS[name]()
        g = em.Graph(inp.V, inp.src, inp.dst)
        ids, values, t = edm.seed_vector(g, inp.hub)
        assert dense(shim, t) == 8.0 and sparse(shim, inp.V, ids, values, 0.0) == 8.0
        assert g.sink[ids[1]] and not g.has_in[ids[2]] and not g.sink[ids[2]] and ids[0] == inp.hub
        assert len(set(ids.tolist())) == 8


# ---- 2. the exact model ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", em.WITH_SINKS)
def test_exact_model_against_float64(name):
    """The integer recurrence reproduces the float64 iteration bit for bit for as long as it certifies
    itself, which is at least 5 iterations on the three inputs of the GPU test; totals stay below 2^53."""
    inp = em.DYADIC_BUILDERS[name]()
    g = em.Graph(inp.V, inp.src, inp.dst)
    _, _, t = edm.seed_vector(g, inp.hub)
    init = em.grid_init(inp.V, 7)
    run = edm.dangling_run(g, 5, t, damping=0.5, init=init)
    assert min(run.exact_iters.values()) >= 5, run.exact_iters
    assert max(run.width_bits) <= em.MANT
    ranks, dc, l1 = edm.float_run(g, 5, t, 0.5, 8.0, init=init)
    for k in range(5):
        assert np.array_equal(bits(run.ranks[k]), bits(ranks[k])), (name, k)
    assert np.array_equal(bits(run.dc), bits(dc)) and np.array_equal(bits(run.l1), bits(l1))
    assert (run.dc > 0).all()
    # the mode differs from the uniform term, and the hub's row shows a lost q * t
    uni = em.dyadic_run(g, 1, teleport=t, damping=0.5, init=init)
    assert run.ranks[0][inp.hub] != uni.ranks[0][inp.hub]
    # a vertex with t = 0 and no in-link drains: r' = damping * r
    lonely = np.nonzero(~g.has_in & (t == 0))[0]
    assert lonely.size > 0 and np.array_equal(run.ranks[0][lonely], 0.5 * init[lonely])


def test_exact_model_refuses_inputs_outside_the_family():
    inp = em.sinks3()
    g = em.Graph(inp.V, inp.src, inp.dst)
    _, _, t = edm.seed_vector(g, inp.hub)
    bad = t.copy()
    bad[inp.hub] += 1.0  # ts = 9: not a power of two
    with pytest.raises(ValueError):
        edm.dangling_run(g, 1, bad)
    bad = t.copy()
    bad[inp.hub] = 4.0 + 1.0 / 64.0  # off the 2^-4 grid
    with pytest.raises(ValueError):
        edm.dangling_run(g, 1, bad)
    with pytest.raises(ValueError):
        edm.dangling_run(g, 1, t / 16.0)  # ts = 1/2 < 1
    with pytest.raises(ValueError):
        edm.dangling_run(g, 1, t, damping=0.85)


# ---- 3. symbols and argument checks ---------------------------------------------------------------
NEW = ("pr_set_teleport_dangling", "pr_get_teleport_dangling", "pr_get_teleport_sum")


def test_symbols_and_null_graph():
    import sparky_hip._lib as L

    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTED
    mode = ctypes.c_int32(7)
    ts = ctypes.c_double(3.5)
    assert lib.pr_set_teleport_dangling(None, L.PR_TELEPORT_DANGLING_TELEPORT) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_set_teleport_dangling(None, 5) == L.PR_ERR_INVALID
    assert lib.pr_get_teleport_dangling(None, ctypes.byref(mode)) == L.PR_ERR_INVALID
    assert mode.value == 7
    assert lib.pr_get_teleport_dangling(None, None) == L.PR_ERR_INVALID
    assert lib.pr_get_teleport_sum(None, ctypes.byref(ts)) == L.PR_ERR_INVALID
    assert ts.value == 3.5
    assert lib.pr_get_teleport_sum(None, None) == L.PR_ERR_INVALID
    assert lib.pr_abi_version() == 2


def test_constants_and_header():
    import sparky_hip._lib as L

    text = open(os.path.join(ROOT, "include", "pagerank_hip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PR_TELEPORT_DANGLING_\w+) (\d+)", text)}
    assert got == {"PR_TELEPORT_DANGLING_UNIFORM": 0, "PR_TELEPORT_DANGLING_TELEPORT": 1}
    assert L.TELEPORT_DANGLING_MODES == {"uniform": 0, "teleport": 1}
    for fn in NEW:
        assert re.search(r"\bint " + fn + r"\(", text), fn
    assert re.search(r"#define PR_ABI_VERSION 2\b", text)
    # the header no longer calls the mode out of scope for the engine
    assert "out of scope" not in text and "keeps the uniform term" not in text


def test_python_methods():
    import sparky_hip

    G, P = sparky_hip.PageRankGraph, sparky_hip.PartGroup
    assert callable(G.set_teleport_dangling) and callable(G.teleport_sum) and callable(P.set_teleport_dangling)
    assert isinstance(G.teleport_dangling, property)


# ---- 4. CLI usage errors (before any GPU work) ----------------------------------------------------
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("teleport_dangling")
    inp, seeds, queue = d / "edges.txt", d / "seeds.txt", d / "queue.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    queue.write_text(str(seeds) + "\n")
    return str(inp), str(seeds), str(queue)


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_dangling_seeds_usage_errors(cli_files, runner):
    inp, seeds, queue = cli_files
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    needs = "--dangling=seeds needs --seeds"
    points = "with --seed-set or --seed-queue use --dangling-to-seeds"
    cases = [(["--dangling=seeds"], False),
             (["--dangling=seeds", "--top", "3"], False),
             (["--dangling=seeds", "--devices", "0,0"], False),
             (["--seed-set", seeds, "--dangling=seeds"], True),
             (["--seed-set", seeds, "--dangling=seeds", "--top", "3"], True),
             (["--seed-queue", queue, "--tol", "1e-6", "--top", "3", "--dangling=seeds"], True)]
    for extra, pointed in cases:
        res = subprocess.run(base + [inp, "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert needs in res.stderr and res.stdout == "", (extra, res.stderr)
        assert (points in res.stderr) == pointed, (extra, res.stderr)
    # --dangling-to-seeds keeps its own rule for --seeds
    res = subprocess.run(base + [inp, "3", "--seeds", seeds, "--dangling-to-seeds"], capture_output=True, text=True,
                         env=env, timeout=120)
    assert res.returncode == 2 and "--dangling-to-seeds needs --seed-set or --seed-queue" in res.stderr
    # an unknown value of --dangling is still an error
    res = subprocess.run(base + [inp, "3", "--dangling=seed"], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 2 and res.stdout == ""
    # the usage text names the option, and no longer says that --seeds keeps the uniform term
    res = subprocess.run(base + ["--help"], capture_output=True, text=True, env=env, timeout=120)
    text = res.stdout + res.stderr
    assert "--dangling=seeds" in text and "keeps the uniform term" not in text
