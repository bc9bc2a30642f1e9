"""pr_batch_step_until without a GPU: the symbols and their host-side argument checks, the per-column
convergence decision of csrc/pr_batch_until.h through host/batch_until_shim.cpp, and the --tol usage
errors of both CLIs (they are raised before any GPU work)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR

CLI = os.path.join(PKG_DIR, "build", "pagerank")


def test_symbols_and_null_batch():
    import sparky_hip._lib as L

    lib = L.load()
    assert hasattr(lib, "pr_batch_step_until") and "pr_batch_step_until" in L.EXPORTED
    assert hasattr(lib, "pr_batch_step_until_ex") and "pr_batch_step_until_ex" not in L.EXPORTED
    iters = np.zeros(16, np.int32)
    p = ctypes.c_void_p(iters.ctypes.data)
    assert lib.pr_batch_step_until(None, 10, 1e-6, p) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_step_until(None, 10, 1e-6, None) == L.PR_ERR_INVALID
    info = np.zeros(2, np.int32)
    assert lib.pr_batch_step_until_ex(None, 10, 1e-6, 8, p, ctypes.c_void_p(info.ctypes.data)) == L.PR_ERR_INVALID


def test_python_methods():
    import sparky_hip

    for m in ("step_until", "_step_until_ex"):
        assert callable(getattr(sparky_hip.PageRankBatch, m))


# ---- the decision ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_until_shim.so"))
    lib.pru_decide.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double, ctypes.c_int]
    lib.pru_decide.restype = ctypes.c_uint32
    lib.pru_all.argtypes = [ctypes.c_int]
    lib.pru_all.restype = ctypes.c_uint32
    return lib


def decide(shim, mask, l1, tol, width):
    a = np.zeros(16, np.float64)
    a[:len(l1)] = l1
    return shim.pru_decide(mask, ctypes.c_void_p(a.ctypes.data), tol, width)


def test_all_mask(shim):
    assert [shim.pru_all(w) for w in (1, 3, 8, 16)] == [0x1, 0x7, 0xff, 0xffff]
    assert shim.pru_block() >= 1
    assert shim.pru_state_bytes() == 8 + 4 * 16  # mask, executed count, 16 per-column counts


def test_threshold_is_inclusive_and_absolute(shim):
    tol = 1e-6
    l1 = [2e-6, 1e-6, np.nextafter(1e-6, 1.0), 0.0, 5e-7, 1e300]
    assert decide(shim, 0x3f, l1, tol, 6) == 0b100101  # <= tol leaves the mask, the next double up stays


def test_nan_never_freezes(shim):
    for tol in (0.0, 1e-6, 1e300):
        assert decide(shim, 0x7, [np.nan, -np.nan, 0.0], tol, 3) == 0b011
    assert decide(shim, 0x3, [np.inf, 1.0], 1e300, 2) == 0b01  # inf is not within any finite tol


def test_tol_zero_needs_exact_zero(shim):
    tiny = np.nextafter(0.0, 1.0)  # the smallest subnormal
    assert decide(shim, 0xf, [0.0, tiny, -0.0, 1e-300], 0.0, 4) == 0b1010


def test_cleared_bit_stays_cleared(shim):
    # column 1 was frozen earlier; its (stale or even large) L1 cannot bring it back
    assert decide(shim, 0b101, [1.0, 1.0, 1.0], 1e-6, 3) == 0b101
    assert decide(shim, 0b101, [1.0, np.nan, 1e-9], 1e-6, 3) == 0b001
    assert decide(shim, 0, [1.0] * 16, 1e-6, 16) == 0
    rng = np.random.default_rng(3)
    for _ in range(200):
        mask = int(rng.integers(0, 1 << 16))
        l1 = rng.choice([0.0, 1e-9, 1e-6, 1e-3, np.nan, np.inf], 16)
        out = decide(shim, mask, l1, 1e-6, 16)
        assert out & ~mask == 0
        for j in range(16):
            want = bool((mask >> j) & 1) and not (l1[j] <= 1e-6)
            assert bool((out >> j) & 1) == want


@pytest.mark.parametrize("width", [1, 3, 8, 16])
def test_bits_at_or_above_width_are_never_set(shim, width):
    # a mask with stray high bits and large L1 everywhere: only columns below width survive
    out = decide(shim, 0xffffffff, [1.0] * 16, 1e-6, width)
    assert out == (1 << width) - 1


# ---- CLI usage errors (before any GPU work) ----------------------------------------------------
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("until")
    inp, seeds = d / "edges.txt", d / "seeds.txt"
    inp.write_text("A B\nB A\n")
    seeds.write_text("A\n")
    return str(inp), str(seeds)


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_tol_usage_errors(cli_files, runner):
    inp, seeds = cli_files
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR)
    needs, bad = "--tol needs --seed-set", "--tol: not a finite number >= 0"
    cases = [(["--tol", "1e-6"], needs),
             (["--tol=1e-6", "--seeds", seeds], needs),
             (["--seed-set", seeds, "--tol", "nan"], bad),
             (["--seed-set", seeds, "--tol", "inf"], bad),
             (["--seed-set", seeds, "--tol=-1"], bad),
             (["--seed-set", seeds, "--tol", "-1"], bad),
             (["--seed-set", seeds, "--tol=-1e-6"], bad),
             (["--seed-set", seeds, "--tol", "abc"], bad),
             (["--seed-set", seeds, "--tol="], bad)]
    for extra, msg in cases:
        res = subprocess.run(base + [inp, "3", *extra], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 2, (extra, res.returncode, res.stderr)
        assert msg in res.stderr and res.stdout == "", (extra, res.stderr)
