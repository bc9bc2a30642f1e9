"""The batch's teleport dangling mode without a GPU: the symbols and their host-side argument checks,
the per-column rule and the term of csrc/pr_batch_dangling.h through host/batch_dangling_shim.cpp
(built with -ffp-contract=off), the --dangling-to-seeds usage errors of both CLIs (raised before any
GPU work), and the helper model's fallback."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import batch_dangling_model as bdm
import batch_order_model as bom
from conftest import PKG_DIR, ROOT

CLI = os.path.join(PKG_DIR, "build", "pagerank")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- 1. symbols ----------------------------------------------------------------------------------
def test_symbols_and_null_batch():
    import sparky_hip._lib as L

    lib = L.load()
    for name in ("pr_batch_set_dangling", "pr_batch_get_dangling", "pr_batch_get_teleport_sums"):
        assert hasattr(lib, name) and name in L.EXPORTED
    mode = ctypes.c_int32(7)
    sums = np.zeros(16, np.float64)
    p = ctypes.c_void_p(sums.ctypes.data)
    assert lib.pr_batch_set_dangling(None, L.PR_BATCH_DANGLING_TELEPORT) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_set_dangling(None, 5) == L.PR_ERR_INVALID
    assert lib.pr_batch_get_dangling(None, ctypes.byref(mode)) == L.PR_ERR_INVALID
    assert mode.value == 7
    assert lib.pr_batch_get_dangling(None, None) == L.PR_ERR_INVALID
    assert lib.pr_batch_get_teleport_sums(None, p) == L.PR_ERR_INVALID
    assert lib.pr_batch_get_teleport_sums(None, None) == L.PR_ERR_INVALID


def test_constants_match_header():
    import sparky_hip._lib as L

    text = open(os.path.join(ROOT, "include", "pagerank_hip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PR_BATCH_DANGLING_\w+) (\d+)", text)}
    assert got == {"PR_BATCH_DANGLING_UNIFORM": 0, "PR_BATCH_DANGLING_TELEPORT": 1}
    assert (L.PR_BATCH_DANGLING_UNIFORM, L.PR_BATCH_DANGLING_TELEPORT) == (0, 1)
    assert L.BATCH_DANGLING_MODES == {"uniform": 0, "teleport": 1}
    for fn in ("pr_batch_set_dangling", "pr_batch_get_dangling", "pr_batch_get_teleport_sums"):
        assert re.search(r"\bint " + fn + r"\(", text), fn


def test_python_methods():
    import sparky_hip

    B = sparky_hip.PageRankBatch
    assert callable(B.set_dangling) and callable(B.teleport_sums)
    assert isinstance(B.dangling, property)


# ---- 2. the rule and the term --------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_dangling_shim.so"))
    d = ctypes.c_double
    lib.prd_uses_teleport.argtypes, lib.prd_uses_teleport.restype = [d], ctypes.c_int
    lib.prd_term.argtypes, lib.prd_term.restype = [d, d], d
    lib.prd_factor.argtypes, lib.prd_factor.restype = [ctypes.c_int, d, d, d], d
    lib.prd_terms.argtypes, lib.prd_terms.restype = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], None
    return lib


def test_rule(shim):
    for ts in (0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan):
        assert shim.prd_uses_teleport(ts) == 0, ts
        assert not bdm.uses_teleport(ts)
    for ts in (5e-324, -5e-324, -1.0, 1e308, -1e308, 1.0, np.finfo(np.float64).max, 2.2250738585072014e-308):
        assert shim.prd_uses_teleport(ts) == 1, ts
        assert bdm.uses_teleport(ts)


def test_factor_is_a_select(shim):
    dc, n = 123.456, 1000.0
    uni = np.float64(dc) / np.float64(n)
    for ts in (0.0, np.inf, np.nan):  # the quotient not taken must not leak into the result
        assert bits(shim.prd_factor(0, dc, ts, n))[0] == bits(uni)[0]
    for ts in (3.0, -7.5, 5e-324, 1e308):
        with np.errstate(over="ignore"):
            want = np.float64(dc) / np.float64(ts)
        assert bits(shim.prd_factor(1, dc, ts, n))[0] == bits(want)[0]


def test_term_is_one_rounded_multiply(shim):
    rng = np.random.default_rng(11)
    n = 4000
    q = np.concatenate([rng.uniform(-3.0, 3.0, n), rng.uniform(-1.0, 1.0, n) * 1e-300, rng.standard_normal(n) * 1e155,
                        np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1.0 / 3.0])])
    t = np.concatenate([rng.uniform(-40.0, 40.0, n), rng.uniform(-1.0, 1.0, n) * 1e-12, rng.standard_normal(n) * 1e155,
                        np.array([1.0, 2.0, 0.5, -0.5, 1e-3, 3.0, 3.0])])
    t[::17] = 0.0
    out = np.zeros_like(q)
    shim.prd_terms(len(q), q.ctypes.data, t.ctypes.data, out.ctypes.data)
    with np.errstate(over="ignore", under="ignore"):
        want = q * t
    assert np.array_equal(bits(out), bits(want))
    sub = (want != 0.0) & (np.abs(want) < np.finfo(np.float64).tiny)
    assert sub.any() and (want < 0).any() and np.isinf(want).any()  # subnormal, negative and overflowing products
    assert bits(shim.prd_term(1.0 / 3.0, 3.0))[0] == bits(np.float64(1.0 / 3.0) * np.float64(3.0))[0]


# ---- 3. CLI usage errors (before any GPU work) ---------------------------------------------------
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dangling")
    inp, seeds = d / "edges.txt", d / "seeds.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    return str(inp), str(seeds)


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_dangling_to_seeds_usage_errors(cli_files, runner):
    inp, seeds = cli_files
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    needs = "--dangling-to-seeds needs --seed-set or --seed-queue"
    cases = [["--dangling-to-seeds"],
             ["--dangling-to-seeds", "--top", "3"],
             ["--seeds", seeds, "--dangling-to-seeds"],
             ["--dangling-to-seeds", "--dangling=none"]]
    for extra in cases:
        res = subprocess.run(base + [inp, "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert needs in res.stderr and res.stdout == "", (extra, res.stderr)
    # the usage text names the option
    res = subprocess.run(base + ["--help"], capture_output=True, text=True, env=env, timeout=120)
    assert "--dangling-to-seeds" in res.stdout + res.stderr


# ---- 4. the helper model -------------------------------------------------------------------------
def test_model_fallback_is_the_uniform_step(oracle_c):
    rng = np.random.default_rng(5)
    V, E = 400, 3000
    src = rng.integers(0, 300, E).astype(np.int32)  # vertices 300.. are sinks
    dst = rng.integers(0, V, E).astype(np.int32)
    dst[:600] = 7  # a row past stride 16's capacity: chunks
    csr = oracle_c.build_csr(V, src, dst)
    r = rng.uniform(0.5, 1.5, V)
    t = rng.uniform(-1.0, 1.0, V)
    for stride in (1, 16):
        m = bdm.DanglingModel(csr, stride)
        assert m.sink.any()
        dc = float(r[m.sink].sum())
        want = bom.BatchModel(csr, stride).step(r, t, dc)
        for ts in (0.0, -0.0, np.inf, -np.inf, np.nan):
            assert np.array_equal(bits(m.step_teleport(r, t, dc, ts)), bits(want)), (stride, ts)
        ts = float(t.sum())
        got = m.step_teleport(r, t, dc, ts)
        assert not np.array_equal(bits(got), bits(want))
        S = m.row_sums(r)
        q = np.float64(dc) / np.float64(ts)
        assert np.array_equal(bits(got), bits(t + np.float64(0.85) * (S + q * t)))
        # a vertex whose teleport term is 0 receives no dangling mass
        t0 = t.copy()
        t0[:50] = 0.0
        got0 = m.step_teleport(r, t0, dc, float(t0.sum()))
        assert np.array_equal(bits(got0[:50]), bits(np.float64(0.85) * S[:50] + 0.0))
