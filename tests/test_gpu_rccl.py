"""The RCCL transport of the row-partitioned iteration, executed on a one-GPU box.

The multi-GPU path (one process per GPU, per-peer ncclSend/ncclRecv of the contributions each part
reads, Sparky.java:192's re-shuffle) normally needs as many GPUs as ranks, and RCCL refuses two
ranks on one device ("Duplicate GPU detected").  `bench.py --share-device` runs every rank on
GPU 0 and gives each rank its own NCCL_HOSTID, so RCCL treats the ranks as separate hosts and
connects them through its socket transport on loopback: the library's communicator attach, its
exchange agreement check (ncclAllGather of the run records), the grouped send/recv of the
unchunked and chunked exchange and torch's process group around them all execute for real.
The bench then checks every rank's rows, summed on rank 0, against the oracle (Sparky.java:233 after
10 iterations) for both exchange modes.  Throughput of such a run means nothing.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_TOL = 1e-9


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, extra, scale=20, timeout=280, launcher=True, steps=6, warmup=2, share=True):
    """launcher=False: a plain `python bench.py --gpus N`, which starts its N ranks itself.
    share=False: one GPU per rank (no --share-device)."""
    cmd = [sys.executable]
    if launcher:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                f"--master-port={_free_port()}"]
    cmd += [os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(world)] + (["--share-device"] if share else []) + [
            "--scale", str(scale), "--steps",
            str(steps), "--warmup", str(warmup), "--parity-iters", "10", "--stage-timeout", "150"] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-5000:]}"
    line = json.loads(lines[-1])
    print(f"world {world} {extra}: exchange {line['config']['exchange_mode']} "
          f"doubles/iter rank0 {line['config']['exchange_doubles_per_iter_rank0']} "
          f"overlap_ab {line['exchange_overlap_ab']} parity {line['parity']}")
    return line


def _check_ipc(line):
    """The CU-free transport (PR_OPT_XCHG_IPC): its set-up succeeded on every rank, every IPC mode
    passed the pre-timing bitwise check against RCCL on every rank and was timed, and in the parity
    leg each -- unchunked, chunked, chunked with per-chunk publication, each run on its own -- gave
    bitwise the RCCL transport's ranks
    (same runs, same gather-space positions, only the mover differs) within the oracle bar.  The
    timed configuration itself (whatever the calibration picked) was re-run and checked too
    (VERDICT r4 item 1)."""
    ab, par = line["exchange_overlap_ab"], line["parity"]
    assert "ipc_error" not in ab, ab.get("ipc_error")
    assert ab["candidates_bitwise_checked"] is True and not ab.get("rejected"), ab.get("rejected")
    names = ("ipc_unchunked", "ipc_chunked", "ipc_chunked_early", "ipc_blit_unchunked", "ipc_blit_chunked_early",
             "ipc_blit_chunked_early_reserve1", "ipc_blit_chunked_early_reserve2")
    for name in names:  # early: per-chunk publication of the send runs
        assert ab[f"{name}_ms_per_step"] > 0
        assert par[f"{name}_bitwise_equal_rccl"] is True
        assert par["modes"][name]["max_rel"] <= RANK_TOL
    assert par["ipc_bitwise_equal_rccl"] is True
    assert par["max_rel_ipc_exchange"] <= RANK_TOL
    _check_timed_mode(line)


def _check_timed_mode(line):
    par = line["parity"]
    assert par["timed_mode"] == line["config"]["exchange_mode"]
    assert par["max_rel_timed_mode"] <= RANK_TOL
    assert par["timed_mode_bitwise_equal_rccl"] is True
    assert line["value"] is not None and "error" not in line


@pytest.mark.gpu
@pytest.mark.timeout(320)
@pytest.mark.parametrize(
    "world,extra",
    [
        (2, ["--build-option", "classes=16"]),  # sparse runs; calibration of unchunked / chunked (2 chunks)
        (3, ["--build-option", "classes=32"]),  # odd rank count, 4 chunks per run
        (2, ["--build-option", "exchange_allgather=1"]),  # whole-slice ncclAllGather (A/B reference)
        (2, ["--graph", "lj"]),  # BASELINE configs[1] (LiveJournal shape) at its policy, RCCL and IPC
    ],
    ids=["p2-c16-sparse", "p3-c32-sparse", "p2-allgather", "p2-lj"],
)
def test_rccl_exchange_on_shared_device(world, extra):
    line = _run(world, extra)
    assert line["n_gpus"] == world
    assert line["config"]["shared_device_rehearsal"] is True
    par = line["parity"]
    assert par is not None and par["ranks_from"] == f"{world} rank(s)"
    assert par["every_row_owned_once"] is True
    assert par["max_rel"] <= RANK_TOL
    if "exchange_allgather=1" not in extra:
        assert line["config"]["exchange_doubles_per_iter_rank0"] > 0
        ab = line["exchange_overlap_ab"]
        assert ab is not None and ab["chosen"] in ("unchunked", "chunked_reserve0", "chunked_reserve1",
                                                   "chunked_reserve2", "ipc_unchunked", "ipc_chunked",
                                                   "ipc_chunked_early", "ipc_blit_unchunked",
                                                   "ipc_blit_chunked_early", "ipc_blit_chunked_early_reserve1",
                                                   "ipc_blit_chunked_early_reserve2")
        assert par["max_rel_overlapped_exchange"] <= RANK_TOL
        _check_ipc(line)


@pytest.mark.gpu
@pytest.mark.timeout(420)
def test_rccl_and_ipc_eight_ranks_shared_device():
    """The driver's largest rank count: 8 ranks (7 peers per rank) on the one GPU, R-MAT s20 with 32
    classes (4 chunks per run) -- every exchange mode calibrated and checked bitwise against the RCCL
    unchunked exchange, the timed mode and every IPC mode against the oracle."""
    line = _run(8, ["--build-option", "classes=32"], timeout=380)
    assert line["n_gpus"] == 8 and line["config"]["shared_device_rehearsal"] is True
    par = line["parity"]
    assert par["ranks_from"] == "8 rank(s)" and par["every_row_owned_once"] is True
    assert par["max_rel"] <= RANK_TOL and par["max_rel_overlapped_exchange"] <= RANK_TOL
    _check_ipc(line)


@pytest.mark.gpu
@pytest.mark.timeout(320)
def test_ipc_on_distinct_gpus():
    """The IPC transport across physical devices: hipIpcOpenMemHandle with lazy peer
    access, copy-engine pulls over xGMI and interprocess event waits between GPUs -- what the driver's
    N-GPU bench can time.  Needs two GPUs; skips on a one-GPU box (the shared-device tests above run
    the same protocol with every rank on one device)."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two or more physical GPUs")
    line = _run(2, ["--build-option", "classes=16"], share=False)
    assert line["n_gpus"] == 2 and line["config"]["shared_device_rehearsal"] is False
    assert line["parity"]["max_rel"] <= RANK_TOL and line["parity"]["every_row_owned_once"] is True
    _check_ipc(line)


@pytest.mark.gpu
@pytest.mark.timeout(320)
def test_plain_bench_gpus_2_runs_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it (the driver's BENCH command shape) runs two
    ranks -- it starts torch.distributed.run itself -- and reports n_gpus 2 with oracle parity."""
    line = _run(2, [], launcher=False)
    assert line["n_gpus"] == 2 and line["value"] is not None
    assert line["parity"]["ranks_from"] == "2 rank(s)" and line["parity"]["every_row_owned_once"] is True
    assert line["parity"]["max_rel"] <= RANK_TOL
    # the oracle built its own CSR from the raw edges, and the library's canonical CSR equals it
    assert line["parity"]["csr_bit_exact"] is True
    _check_timed_mode(line)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rccl_default_policy_at_baseline_size():
    """BASELINE.json configs[2] (Erdos-Renyi s24) at P = 4 through the RCCL transport with the default
    build policy -- 64 classes, piece codes, the epilogue's fused pack, per-peer runs -- both exchange
    modes checked against the oracle after 10 iterations (Sparky.java:187, :192, :229-233)."""
    line = _run(4, ["--graph", "er", "--serial-build"], scale=24, timeout=560, steps=4, warmup=1)
    assert line["n_gpus"] == 4 and line["config"]["build_options"] is None
    assert line["config"]["exchange_doubles_per_iter_rank0"] > 0
    par = line["parity"]
    assert par["every_row_owned_once"] is True
    assert par["max_rel"] <= RANK_TOL and par["max_rel_overlapped_exchange"] <= RANK_TOL
    _check_ipc(line)
    assert line["roofline"]["classes"] == 64 and line["config"]["code_bits"] in (20, 24)


@pytest.mark.gpu
@pytest.mark.timeout(420)
def test_ipc_modes_long_run_shared_device():
    """The IPC transport past the HIP runtime's 32 records per interprocess event (the 33rd record's
    wait fails and the event stays broken): tools/ipc_modes_probe.py switches between RCCL, IPC and
    IPC with per-chunk publication, chunked and not, copy engines or blit kernel, 32 times with 10
    iterations each (~170 exchanges per buffer, every event recycled several times); every step
    must give bitwise the RCCL unchunked ranks on both ranks."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", f"--master-port={_free_port()}", os.path.join(ROOT, "tools", "ipc_modes_probe.py"),
           "--rounds", "2", "--iters", "10"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    recs, dec = [], json.JSONDecoder()  # two ranks' lines can land on one line of the launcher's stdout
    for line in p.stdout.splitlines():
        i = line.find("{")
        while i >= 0:
            obj, end = dec.raw_decode(line, i)
            recs.append(obj)
            i = line.find("{", end)
    steps = [r for r in recs if "step" in r]
    assert p.returncode == 0 and steps, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    errors = [r for r in steps if "error" in r]
    assert not errors, errors[:4]
    assert len(steps) == 2 * 32 and all(r["bitwise_equal_ref"] for r in steps)


@pytest.mark.gpu
@pytest.mark.timeout(420)
def test_ipc_one_long_step_shared_device():
    """one pr_step of 300 iterations with no sync inside, in IPC mode 2 (per-chunk
    publication, chunked copies; copy engines and blit) and mode 1, on two ranks sharing the device.
    The host enqueues far ahead of its device there; the library bounds that lead (pr_ipc.hip
    bound_lead) so no interprocess event generation is destroyed before the device has passed every
    record and wait on it.  Every run must give bitwise the RCCL unchunked ranks of 300 iterations."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", f"--master-port={_free_port()}", os.path.join(ROOT, "tools", "ipc_modes_probe.py"),
           "--rounds", "0", "--scale", "22", "--long", "300"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    recs, dec = [], json.JSONDecoder()
    for line in p.stdout.splitlines():
        i = line.find("{")
        while i >= 0:
            obj, end = dec.raw_decode(line, i)
            recs.append(obj)
            i = line.find("{", end)
    longs = [r for r in recs if "long" in r]
    assert p.returncode == 0 and longs, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    assert not [r for r in longs if "error" in r], longs
    assert len(longs) == 2 * 3 and all(r["bitwise_equal_ref"] for r in longs)
