"""The batch mixes without a GPU: the numpy model (tests/batch_mix_model.py) against the PR_HD blend
of csrc/pr_batch_mix.h through host/batch_mix_shim.cpp (built with -ffp-contract=off), bit for bit;
the symbols and the host-side argument checks that need no batch; the --mix usage errors of both CLIs
(raised before any GPU work)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import batch_mix_model as bmm
from conftest import PKG_DIR, ROOT

CLI = os.path.join(PKG_DIR, "build", "pagerank")
bits = bmm.bits
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # the inputs overflow and hold NaN on purpose


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "build", "libpr_batch_mix_shim.so"))
    P = ctypes.c_void_p
    lib.prm_stride.argtypes, lib.prm_stride.restype = [ctypes.c_int], ctypes.c_int
    lib.prm_elem.argtypes, lib.prm_elem.restype = [P, P, ctypes.c_int], ctypes.c_double
    lib.prm_blend.argtypes, lib.prm_blend.restype = [ctypes.c_int, ctypes.c_int, P, P, P], None
    return lib


def shim_blend(shim, w, cols):
    w = np.ascontiguousarray(w, np.float64)
    x = np.ascontiguousarray(np.stack(cols, axis=1), np.float64)  # V x width, row-major
    out = np.full(x.shape[0], np.nan)
    shim.prm_blend(x.shape[0], x.shape[1], ctypes.c_void_p(w.ctypes.data), ctypes.c_void_p(x.ctypes.data),
                   ctypes.c_void_p(out.ctypes.data))
    return out


# ---- 1. the model against the shared expression -----------------------------------------------------
SPECIAL = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, 1.0 / 3.0, 0.1, 0.7, 1.0, -1.0,
                    3.0, 1e300, -1e300, 1.7976931348623157e308, 2.0 ** -30, 1.0 + 2.0 ** -52])


def test_stride(shim):
    assert [shim.prm_stride(n) for n in range(1, 17)] == [1, 2, 4, 4] + [8] * 4 + [16] * 8


@pytest.mark.parametrize("width", [1, 2, 3, 5, 8, 16])
def test_model_equals_shim(shim, width):
    rng = np.random.default_rng(width)
    V = 400
    cols = [rng.choice(SPECIAL, V) * rng.choice(np.array([1.0, 1.0 / 3.0, 3.0]), V) for _ in range(width)]
    for trial in range(40):
        w = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 1.0 / 3.0, 0.25, -0.75, 0.1, 1e-300, 3.0]), width)
        if trial % 3 == 0:
            w = rng.standard_normal(width)
        want = bmm.blend(w, cols)
        assert np.array_equal(bits(shim_blend(shim, w, cols)), bits(want)), (width, trial)


def test_rounding_is_two_steps(shim):
    """1/3-type products: a fused multiply-add would give other bits than `*` then `+`."""
    rng = np.random.default_rng(7)
    a, b = rng.random(2000) + 0.5, rng.random(2000) + 0.5
    w = np.array([1.0 / 3.0, 1.0 / 7.0])
    two = (w[0] * a) + (w[1] * b)
    got = shim_blend(shim, w, [a, b])
    assert np.array_equal(bits(got), bits(two)) and np.array_equal(bits(bmm.blend(w, [a, b])), bits(two))
    import math
    fused = np.array([math.fma(w[1], y, w[0] * x) for x, y in zip(a, b)]) if hasattr(math, "fma") else None
    if fused is not None:
        assert (bits(fused) != bits(two)).any()  # the inputs do tell the two apart


def test_zero_weights_one_hot_and_non_finite(shim):
    V = 64
    rng = np.random.default_rng(3)
    x = rng.choice(SPECIAL, V)
    bad = np.where(np.arange(V) % 2 == 0, np.inf, np.nan)
    neg = np.full(V, -np.inf)
    cols = [bad, x, neg, x * 0.5]
    for w in ([0.0, 1.0, 0.0, 0.0], [-0.0, 1.0, -0.0, -0.0]):  # one-hot: the column bit for bit, -0.0 kept
        got = shim_blend(shim, w, cols)
        assert np.array_equal(bits(got), bits(x)) and np.array_equal(bits(bmm.blend(w, cols)), bits(x))
    w = [0.0, 0.25, -0.0, -3.0]  # inf and NaN behind a weight of 0 never enter
    want = (0.25 * x) + (-3.0 * (x * 0.5))
    assert np.array_equal(bits(shim_blend(shim, w, cols)), bits(want))
    assert np.array_equal(bits(bmm.blend(w, cols)), bits(want))
    zero = shim_blend(shim, [0.0, -0.0, 0.0, -0.0], cols)  # no participating column: +0.0
    assert (bits(zero) == 0).all() and (bits(bmm.blend([0.0, -0.0, 0.0, -0.0], cols)) == 0).all()
    # the first participating column is taken as it is: -1 * 0.0 = -0.0 survives, 0.0 + -0.0 would not
    m = shim_blend(shim, [0.0, -1.0, 0.0, 0.0], [bad, np.zeros(V), neg, x])
    assert (bits(m) == bits(np.array([-0.0]))[0]).all()
    # subnormal products and sums
    tiny = np.full(V, 5e-324)
    w2 = [0.5, 3.0, 0.0, 1.0]
    cols2 = [tiny * 3, tiny, bad, -tiny * 2]
    assert np.array_equal(bits(shim_blend(shim, w2, cols2)), bits(bmm.blend(w2, cols2)))


def test_model_listing():
    s = np.array([0.5, -0.0, 0.0, 0.5, 2.0, -1.0, 0.5])
    ids, sc = bmm.listing(s, 5)
    assert list(ids) == [4, 0, 3, 6, 2] and np.array_equal(bits(sc), bits(s[[4, 0, 3, 6, 2]]))
    assert list(bmm.listing(s, 10)[0]) == [4, 0, 3, 6, 2, 1, 5]
    assert list(bmm.listing(s, 3, excluded=[0, 4])[0]) == [3, 6, 2]
    assert len(bmm.listing(s, 0)[0]) == 0


# ---- 2. symbols and the checks that need no batch ---------------------------------------------------
def test_symbols_declared_and_exported():
    import sparky_hip._lib as L

    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "pagerank_hip.h")).read()
    assert re.search(r"#define PR_BATCH_MAX_MIXES 16\b", hdr) and L.BATCH_MAX_MIXES == 16
    assert re.search(r"#define PR_ABI_VERSION 2\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pr_batch_mix_topk", "pr_batch_mix_get"):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert hasattr(lib, name) and name in L.EXPORTED
    assert hasattr(lib, "pr_batch_mix_topk_ex") and "pr_batch_mix_topk_ex" not in code  # internal
    w = np.ones(4)
    out = np.zeros(4)
    n = np.zeros(1, np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.pr_batch_mix_topk(None, 1, p(w), None, None, 0, None, None, p(n)) == L.PR_ERR_INVALID
    assert b"NULL" in lib.pr_last_error()
    assert lib.pr_batch_mix_get(None, p(w), p(out)) == L.PR_ERR_INVALID
    assert lib.pr_batch_mix_topk_ex(None, 1, p(w), None, None, 0, None, None, p(n), 8, 0, None) == L.PR_ERR_INVALID


def test_python_methods_exist():
    from sparky_hip.batch import PageRankBatch

    for name in ("mix", "mix_topk", "_mix_topk_ex"):
        assert callable(getattr(PageRankBatch, name))


# ---- 3. the CLIs' usage errors -----------------------------------------------------------------------
def run_cli(runner, args):
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    return subprocess.run(base + args, capture_output=True, env=dict(os.environ, PYTHONPATH=PKG_DIR), timeout=120)


SETS = ["--seed-set", "a.txt", "--seed-set", "b.txt"]
NEEDS = b"--mix needs --seed-set and --top"
WEIGHTS = b"--mix takes one finite weight per --seed-set, separated by commas"
# case -> (arguments, the message of the check that has to fire)
BAD = {
    "no seed set": (["--top", "3", "--mix", "1"], NEEDS),
    "no top": (SETS + ["--mix", "0.5,0.5"], NEEDS),
    "too few weights": (SETS + ["--top", "3", "--mix", "1"], WEIGHTS),
    "too many weights": (SETS + ["--top", "3", "--mix", "1,2,3"], WEIGHTS),
    "nan": (SETS + ["--top", "3", "--mix", "1,nan"], WEIGHTS),
    "inf": (SETS + ["--top", "3", "--mix", "inf,1"], WEIGHTS),
    "overflow": (SETS + ["--top", "3", "--mix", "1e999,1"], WEIGHTS),
    "abc": (SETS + ["--top", "3", "--mix", "abc,1"], WEIGHTS),
    "empty field": (SETS + ["--top", "3", "--mix", "1,"], WEIGHTS),
    "empty": (SETS + ["--top", "3", "--mix="], WEIGHTS),
    "17 mixes": (SETS + ["--top", "3"] + ["--mix", "1,1"] * 17, b"--mix: at most 16 mixes"),
    "with a queue": (["--seed-queue", "list.txt", "--tol", "1e-6", "--top", "3", "--mix", "1"],
                     b"--mix does not combine with --seed-queue"),
}


@pytest.mark.parametrize("runner", ["cpp", "python"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_cli_usage_errors(runner, case, tmp_path):
    """Status 2, the message of the check the case is there for (both runners word it alike), nothing on
    stdout.  No input file exists: a run that got past the usage checks would fail differently (status 1
    or a traceback); a runner that does not know --mix says "unknown" or "unrecognized", not this."""
    args, message = BAD[case]
    res = run_cli(runner, [str(tmp_path / "missing.txt"), "5"] + args)
    assert res.returncode == 2, (case, res.stderr)
    assert message in res.stderr, (case, res.stderr)
    assert res.stdout == b""


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_help_names_mix(runner):
    res = run_cli(runner, ["--help"])
    assert b"--mix" in res.stdout + res.stderr
