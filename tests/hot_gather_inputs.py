"""Inputs whose wave units have provable numbers of cold entries (tests of k_spmv_hot's gathers).

boundary_graph() relies on documented layout rules only:

* DESIGN.md §4 with one part: the internal order is (out-degree descending, original ID ascending)
  and the column class of the vertex at internal rank j is j % C.
* plan_chunk (csrc/pr_plan.hip): a (row, class) segment longer than 512 entries becomes PIECE units
  of exactly 512 entries, the remainder last; a segment of exactly 512 stays one STREAM unit.
* With hot_slots = 0 every real entry is cold (gathered from memory); padding entries are not.

Construction: H hub rows at IDs 0..H-1; every vertex has one ring edge into the non-hub rows; the M
vertices after the hubs ("members") each also link to exactly one hub.  The members are the only
vertices of out-degree 2, so they hold the internal ranks 0..M-1 in ID order and member i has class
i % C.  A hub that is given L members of one class x has the single (row, class) segment of length L
and no other in-link.  The hubs of LENGTHS come first; the members that these leave over go, at most
SPILL_MAX per (hub, class), to a few more hubs whose segments therefore all stay short.

So the last PIECE unit of the hub with length 512 + m has exactly m cold entries: on both sides of
every 64-entry load of a dense round, of the 128-value half, of the 256-entry round, a single entry
and a full unit.  tests/test_hot_gather_inputs_cpu.py proves the segment lengths from the oracle's
CSR, without a GPU; tests/test_gpu_hot_gather.py runs the graph.
"""
import numpy as np

CLASSES = 8
WAVE_UNIT = 512  # entries of a wave unit (pr_internal.h kWaveUnit)
TAILS = [1, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385,
         447, 448, 449, 511]
LENGTHS = [WAVE_UNIT + m for m in TAILS] + [512, 513, 1024, 1025]
SPILL_MAX = 300  # members per (spill hub, class): below a wave unit, so these segments stay short
N_VERTICES = 40000
RING_SHIFT = 7


def boundary_graph():
    """Returns (V, src, dst, plan): int32 edge arrays and plan = dict(C, H, M, n_listed,
    hub_class[n_listed], hub_len[n_listed])."""
    C = CLASSES
    # listed hubs -> classes: longest first into the least loaded class
    load = [0] * C
    hub_class = [0] * len(LENGTHS)
    for h in sorted(range(len(LENGTHS)), key=lambda h: (-LENGTHS[h], h)):
        x = min(range(C), key=lambda x: (load[x], x))
        hub_class[h] = x
        load[x] += LENGTHS[h]
    per_class = max(load)
    M = per_class * C
    n_spill = max(-(-(per_class - load[x]) // SPILL_MAX) for x in range(C))
    H = len(LENGTHS) + n_spill
    V = N_VERTICES
    assert H + M < V
    hub_of = np.full(M, -1, np.int64)  # member i -> its hub
    used = [0] * C  # members of class x handed out so far
    for h, (x, L) in enumerate(zip(hub_class, LENGTHS)):
        hub_of[x + C * np.arange(used[x], used[x] + L)] = h
        used[x] += L
    for x in range(C):
        s = 0
        while used[x] < per_class:
            n = min(SPILL_MAX, per_class - used[x])
            hub_of[x + C * np.arange(used[x], used[x] + n)] = len(LENGTHS) + s
            used[x] += n
            s += 1
    assert hub_of.min() >= 0 and hub_of.max() < H
    ids = np.arange(V, dtype=np.int64)
    src = np.concatenate([ids, H + np.arange(M)])
    dst = np.concatenate([H + (ids + RING_SHIFT) % (V - H), hub_of])
    plan = dict(C=C, H=H, M=M, n_listed=len(LENGTHS), hub_class=list(hub_class), hub_len=list(LENGTHS))
    return V, src.astype(np.int32), dst.astype(np.int32), plan


def random_edges(rng, V, E, p_nolink=0.05, hub_frac=0.0):
    """test_gpu_parity.py's random edge list: uniform edges, a hub at vertex 0, records without
    links, and one (v, -1) record for every vertex that would not appear otherwise."""
    src = rng.integers(0, V, E, dtype=np.int64)
    dst = rng.integers(0, V, E, dtype=np.int64)
    if hub_frac > 0:
        dst[rng.random(E) < hub_frac] = 0
    dst[rng.random(E) < p_nolink] = -1
    seen = np.zeros(V, bool)
    seen[src] = True
    seen[dst[dst >= 0]] = True
    miss = np.nonzero(~seen)[0]
    src = np.concatenate([src, miss])
    dst = np.concatenate([dst, np.full(miss.shape, -1)])
    return src.astype(np.int32), dst.astype(np.int32)


def segment_lengths(csr, C):
    """From a canonical CSR (rows = dst, columns = src): (row, class, length) of every (row, class)
    segment of the one-part split layout, recomputed with numpy."""
    V = csr.n_vertices
    rank_of = np.empty(V, np.int64)
    rank_of[np.lexsort((np.arange(V), -csr.out_deg.astype(np.int64)))] = np.arange(V)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(csr.row_ptr))
    key = rows * C + rank_of[csr.col_idx] % C
    seg, n = np.unique(key, return_counts=True)
    return seg // C, seg % C, n
