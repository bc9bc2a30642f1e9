"""The boundary-unit input of tests/test_gpu_hot_gather.py, proven on the CPU: built into the
oracle's canonical CSR, with the internal order, the column classes and the (row, class) segment
lengths recomputed in numpy from the documented layout rules (hot_gather_inputs), its long segments
are exactly the listed lengths -- so the GPU tests' claims about the cold count of every last piece
cannot drift from the generator."""
import numpy as np

import hot_gather_inputs as hgi


def test_boundary_graph_segments(oracle_c):
    V, src, dst, plan = hgi.boundary_graph()
    C, H, M = plan["C"], plan["H"], plan["M"]
    assert C == 8 and 39000 <= V <= 41000
    csr = oracle_c.build_csr(V, src, dst)
    assert csr.n_edges == len(src)  # no duplicate edge
    # the members are the only vertices of out-degree 2: ranks 0..M-1 in ID order, class i % C
    assert np.all(csr.out_deg[H:H + M] == 2)
    assert np.all(csr.out_deg[:H] == 1) and np.all(csr.out_deg[H + M:] == 1)
    row, cls, n = hgi.segment_lengths(csr, C)
    # every segment of a wave unit's length or more belongs to a listed hub, one each, of the
    # planned class and length: the multiset is exactly the list
    big = n >= hgi.WAVE_UNIT
    assert sorted(n[big].tolist()) == sorted(hgi.LENGTHS)
    assert sorted(n[n > hgi.WAVE_UNIT].tolist()) == sorted(x for x in hgi.LENGTHS if x > hgi.WAVE_UNIT)
    assert row[big].tolist() == list(range(plan["n_listed"]))
    assert cls[big].tolist() == plan["hub_class"] and n[big].tolist() == plan["hub_len"]
    # a listed hub has no other in-link; the other hubs' segments are short; every other row has
    # ring edges only
    indeg = np.diff(csr.row_ptr)
    assert indeg[:plan["n_listed"]].tolist() == plan["hub_len"]
    spill = (row >= plan["n_listed"]) & (row < H)
    assert spill.any() and n[spill].max() <= hgi.SPILL_MAX
    assert indeg[H:].min() == 1 and indeg[H:].max() == 2  # V ring edges over V - H rows
    # the last piece's cold count of every listed tail, as the GPU test assumes
    tails = sorted((x - 1) % hgi.WAVE_UNIT + 1 for x in n[n > hgi.WAVE_UNIT].tolist())
    assert tails == sorted(hgi.TAILS + [1, 512, 1])


def test_lengths_are_the_issue_list():
    assert len(hgi.TAILS) == 24 and len(hgi.LENGTHS) == 28
    for b in (64, 128, 192, 256, 320, 384, 448):  # both sides of every load, half and round boundary
        assert {b - 1, b, b + 1} <= set(hgi.TAILS)
    assert {1, 8, 511} <= set(hgi.TAILS) and {512, 513, 1024, 1025} <= set(hgi.LENGTHS)
