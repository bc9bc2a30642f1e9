"""Parity on the BASELINE.json configs the bench numbers are quoted on, at full size, through the
product path with the default policy (no layout or hot-set overrides).

R-MAT scale-26 (configs[3], the headline metric), Erdos-Renyi scale-24 (configs[2]) and the
Twitter-2010-shaped Chung-Lu graph (configs[4], here on one GPU) are generated on the device,
interned on the device (pr_intern_device) and built by libpagerank_hip exactly as bench.py does
(sparky_hip.workloads).  At these sizes the size policy picks 64 column classes with u64 row
masks, the grouped epilogue, the 18,430-slot LDS hot set and, at s26 and Twitter, more than 2^28
partial slots and 32-bit buffer offsets over a gather space of 0.26-0.33 GB -- the configuration
no smaller test reaches.

Against oracle/pagerank_oracle.c (the OpenMP restatement of Sparky.java:98-235) on the same
interned edges:
* canonical CSR, out-degrees and vertex flags: bit-exact;
* ranks after every one of 10 iterations (Sparky.java:187): max relative error <= 1e-9;
* the dangling sum dc (Sparky.java:219-222) and the L1 delta of every iteration: relative 1e-9.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANK_TOL = 1e-9  # north_star: "ranks within 1e-9 max relative error"
ITERS = 10  # Sparky.java:187


@pytest.fixture(scope="module")
def hip():
    import sparky_hip

    assert sparky_hip.device_count() > 0, "no GPU visible: the gpu tests need an MI355X"
    return sparky_hip


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


@pytest.mark.parametrize("graph,scale", [("rmat", 26), ("er", 24), ("twitter", 0)],
                         ids=["rmat-s26", "er-s24", "twitter-full"])
def test_headline_config_parity(hip, oracle_c, graph, scale):
    import torch

    from sparky_hip.workloads import generate

    t0 = time.perf_counter()
    wl = generate(graph, scale=scale)
    torch.cuda.synchronize()
    hs, hd = wl.src.cpu().numpy(), wl.dst.cpu().numpy()
    g = hip.PageRankGraph(wl.n_vertices, wl.src.data_ptr(), wl.dst.data_ptr(), device_input=True,
                          n_edges=wl.n_edges)
    try:
        del wl
        torch.cuda.empty_cache()
        info = g.info()
        # the product configuration of the bench line
        assert info["layout"] == 1 and info["classes"] == 64 and info["epilogue"] == 3, info
        assert info["hot_slots"] == 18429, info
        assert info["hot_gather"] == 1, info  # the dense cold gathers (pr_iter.hip kDenseUnitsPerCU)
        if graph != "er":
            assert info["partial_slots"] > (1 << 28), info
        t_build = time.perf_counter()
        csr = oracle_c.build_csr(info["n_vertices"], hs, hd)
        del hs, hd
        t_orc = time.perf_counter()
        ex = g.export_csr()
        assert info["n_edges"] == csr.n_edges
        assert np.array_equal(ex.row_ptr, csr.row_ptr)
        assert np.array_equal(ex.col_idx, csr.col_idx)
        assert np.array_equal(ex.out_deg, csr.out_deg)
        assert np.array_equal(ex.vflags, csr.vflags)
        del ex
        hist = []
        ranks, stats = g.run(ITERS, want_ranks_in_callback=True, callback=lambda it, r, st: hist.append(r))
    finally:
        g.close()
    t_gpu = time.perf_counter()
    ref = oracle_c.run(csr, ITERS, keep_history=True)
    t_ref = time.perf_counter()
    errs = [max_rel(hist[it], ref["history"][it]) for it in range(ITERS)]
    print(f"\n{graph} s{scale}: V={info['n_vertices']} E'={info['n_edges']} slots={info['partial_slots']} "
          f"max_rel per iteration {['%.1e' % e for e in errs]}; gen+build {t_build - t0:.1f}s "
          f"oracle build {t_orc - t_build:.1f}s gpu run {t_gpu - t_orc:.1f}s oracle run {t_ref - t_gpu:.1f}s")
    for it in range(ITERS):
        assert errs[it] <= RANK_TOL, (it, errs[it])
        assert abs(stats[it].dangling_sum - ref["dc"][it]) <= RANK_TOL * max(abs(ref["dc"][it]), 1.0), it
        assert abs(stats[it].l1_delta - ref["l1"][it]) <= RANK_TOL * max(ref["l1"][it], 1.0), it
    assert np.array_equal(ranks, hist[-1])
