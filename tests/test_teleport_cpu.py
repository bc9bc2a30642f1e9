"""Personalised PageRank, the parts that need no GPU: the seed-file parser and the seeds' teleport
terms of libpagerank_host (prh_parse_seeds, prh_seed_teleport), the argument checks of
pr_set_teleport / pr_set_teleport_sparse that run before any device call, both CLIs' exit status on a
bad --seeds file, and host/seeds_check.cpp under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT

CLI = os.path.join(PKG_DIR, "build", "pagerank")
EDGES = b"A B\nA C\nB C\nC A\nD\nE A\n"  # IDs in first-appearance order: A 0, B 1, C 2, D 3, E 4


@pytest.fixture(scope="module")
def edges():
    from sparky_hip._host import HostEdges

    e = HostEdges.parse(EDGES)
    assert e.names() == ["A", "B", "C", "D", "E"]
    yield e
    e.close()


def test_seed_lines(edges):
    ids, w = edges.parse_seeds(b"C 2\nA\n")
    assert ids.dtype == np.int32 and w.dtype == np.float64
    assert list(ids) == [2, 0] and list(w) == [2.0, 1.0]  # weights default to 1
    ids, w = edges.parse_seeds(b"# seeds of the run\n\nE\t0.25\r\n   \n#D\nB 3e0\nA")
    assert list(ids) == [4, 1, 0] and list(w) == [0.25, 3.0, 1.0]  # file order; no final newline
    ids, w = edges.parse_seeds(b"D 1e-300\n")
    assert list(ids) == [3] and list(w) == [1e-300]


@pytest.mark.parametrize("data,line,word", [
    (b"A\nX 2\n", 2, "not in the edge list"),
    (b"A\n\n# c\nA 3\n", 4, "twice"),
    (b"A 0\n", 1, "weight"),
    (b"B\nA -1\n", 2, "weight"),
    (b"A nan\n", 1, "weight"),
    (b"B 2\nC\nA inf\n", 3, "weight"),
    (b"A 1x\n", 1, "weight"),
    (b"A 1 junk\n", 1, "tokens"),
    (b"", 1, "empty"),
    (b"\n# nothing\n", 3, "empty"),
])
def test_bad_seed_lines_name_the_line(edges, data, line, word):
    from sparky_hip._host import HostError

    with pytest.raises(HostError) as ei:
        edges.parse_seeds(data)
    assert f"line {line}:" in str(ei.value) and word in str(ei.value)


def test_read_seeds_file(edges, tmp_path):
    from sparky_hip._host import HostError

    f = tmp_path / "seeds.txt"
    f.write_text("C 2\nA\n")
    ids, w = edges.read_seeds(str(f))
    assert list(ids) == [2, 0] and list(w) == [2.0, 1.0]
    f.write_text("C 2\nQ\n")
    with pytest.raises(HostError) as ei:
        edges.read_seeds(str(f))
    assert "line 2:" in str(ei.value) and str(f) in str(ei.value)
    with pytest.raises(HostError):
        edges.read_seeds(str(tmp_path / "missing.txt"))


def test_seed_teleport_expression():
    """values[i] = ((teleport * N) * w[i]) / W with W summed left to right: bit for bit the explicit
    loop (Python's sum() compensates since 3.12 and would differ in the last bit), and the terms
    add up to the scalar run's total teleport mass 0.15 N."""
    from sparky_hip._host import seed_teleport

    rng = np.random.default_rng(3)
    w = np.exp(rng.normal(0.0, 3.0, 1000))
    N = 123_457
    got = seed_teleport(w, N)
    W = 0.0
    for x in w.tolist():
        W = W + x
    mass = 0.15 * float(N)
    want = [(mass * x) / W for x in w.tolist()]
    assert [struct.pack("<d", x) for x in got.tolist()] == [struct.pack("<d", x) for x in want]
    total = 0.0
    for x in got.tolist():
        total = total + x
    assert abs(total - 0.15 * N) <= 1e-12 * (0.15 * N)
    one = seed_teleport(np.array([7.0]), 4160)
    assert one[0] == 0.15 * 4160


def test_null_graph_is_invalid():
    from sparky_hip import _lib

    L = _lib.load()
    t = np.full(4, 0.15)
    ids = np.array([0, 1], np.int32)
    assert L.pr_set_teleport(None, ctypes.c_void_p(t.ctypes.data)) == _lib.PR_ERR_INVALID
    assert L.pr_set_teleport(None, None) == _lib.PR_ERR_INVALID
    assert L.pr_set_teleport_sparse(None, 2, ctypes.c_void_p(ids.ctypes.data), ctypes.c_void_p(t.ctypes.data),
                                    0.0) == _lib.PR_ERR_INVALID
    assert L.pr_last_error()


@pytest.mark.parametrize("runner", ["cpp", "python"])
def test_cli_bad_seeds_exit_2_without_a_gpu(tmp_path, runner):
    inp = tmp_path / "edges.txt"
    inp.write_bytes(EDGES)
    seeds = tmp_path / "seeds.txt"
    seeds.write_text("C 2\nnot-a-url\n")
    base = [CLI] if runner == "cpp" else [sys.executable, "-m", "sparky_hip"]
    env = dict(os.environ, PYTHONPATH=PKG_DIR, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run(base + [str(inp), "3", "--seeds", str(seeds), "--top", "2"], capture_output=True, text=True,
                         env=env, timeout=120)
    assert res.returncode == 2, (res.stdout, res.stderr)
    assert "line 2:" in res.stderr and "not-a-url" in res.stderr
    assert res.stdout == ""


def test_seeds_check_under_sanitizers(tmp_path):
    """host/seeds_check.cpp + pr_host.cpp as one stand-alone program under ASan + UBSan: malformed
    seed files and truncated buffers (exact-length heap copies, every prefix) with no report."""
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build host/seeds_check.cpp"
    host = os.path.join(PKG_DIR, "host")
    exe = tmp_path / "seeds_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "seeds_check.cpp"),
           os.path.join(host, "pr_host.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "done, 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
