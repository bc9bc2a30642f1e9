"""A plain model of the row partition (csrc/pr_build.hip order_and_geometry and local_keys, csrc/
pr_exchange.hip): who owns a vertex, what every pair of parts exchanges, and the geometry that
decides which code a part takes (csrc/pr_layout.h, tests/test_layout_policy_cpu.py).  numpy
only; it imports nothing from sparky_hip and loads no shared library.  tests/
test_partition_model_cpu.py checks the model and the inputs below without a GPU, tests/
test_gpu_partition_edges.py holds the library to the model.

The definition:

  owner      vertices sorted by (out-degree descending, ID ascending); sorted index i belongs to
             part i % P and is that part's local index i / P (tests/test_dist_cpu.py layout()).
  rows       part p of V vertices owns (V - p + P - 1) / P rows if V > p, else none.
  pair[p,q]  the number of distinct sources owned by p that the in-links of q's rows read (p != q;
             the diagonal is 0: a part's own slice is not exchanged).
  sparse     part p sends q those pair[p, q] contributions and then its two slots {dangling partial,
             L1 partial}: xchg_send[p] = sum_q pair[p, q] + 2 (P - 1),
             xchg_recv[q] = sum_p pair[p, q] + 2 (P - 1)           (PR_INFO_XCHG_SEND / _RECV).
  all-gather whole slices: every part receives P - 1 times what it sends.
  classes    local index j of a part lies in column class j % C (C = 1: the fused layout), so a part
             with fewer than C rows leaves whole classes empty.
  chunks     the overlapped exchange moves a run in max(1, C / 8) chunks, chunk c = the rows of
             classes [8 c, 8 c + 8); the two slots travel in the last chunk.
  hot set    Kp = hot_slots / P slots per part and class (hot_slots -1: 18429); 0: no hot set.
  codes      piece codes and the fused pack exist for P <= 8 only (kMaxPackParts).

The builders isolated() and one_way() make graphs whose partition is known by construction: every
source has out-degree 2, so the degree order is the ID order and the owner of a vertex is ID % P.
"""
from collections import namedtuple

import numpy as np

from test_dist_cpu import exchange_lists, layout  # noqa: F401  (exchange_lists: the cross-check)
from test_gpu_parity import random_edges  # noqa: F401  (re-exported: the third builder)

K_XCDS = 8  # classes per hot phase = per exchange chunk (pr_internal.h kXcds)
K_MAX_PARTS = 64  # pr_internal.h kMaxParts
K_MAX_PACK_PARTS = 8  # pr_internal.h kMaxPackParts: fused pack and piece codes up to here
K_HOT_SLOTS_DEFAULT = 18429  # pr_internal.h kHotSlotsDefault (PR_BOPT_HOT_SLOTS = -1)


# ---- the partition -------------------------------------------------------------------------------
def owners(csr, P):
    """Owner of every vertex."""
    _, rank_of, _, _ = layout(csr, P)
    return (rank_of % P).astype(np.int64)


def part_rows(V, P):
    """Rows owned by every part, from the sizes alone."""
    return np.array([(V - p + P - 1) // P if V > p else 0 for p in range(P)], np.int64)


def local_rows(csr, P):
    return np.bincount(owners(csr, P), minlength=P).astype(np.int64)


def local_edges(csr, P):
    """In-links of the rows every part owns."""
    own = owners(csr, P)
    return np.bincount(own, weights=np.diff(csr.row_ptr), minlength=P).astype(np.int64)


def pair_counts(csr, P):
    """pair[p, q]: distinct sources owned by p that q's in-links read (p != q)."""
    own = owners(csr, P)
    rows = np.repeat(np.arange(csr.n_vertices, dtype=np.int64), np.diff(csr.row_ptr))
    cols = csr.col_idx.astype(np.int64)
    cross = own[cols] != own[rows]
    reads = np.unique(cols[cross] * P + own[rows[cross]])  # (source, reading part), once each
    src, q = reads // P, reads % P
    return np.bincount(own[src] * P + q, minlength=P * P).reshape(P, P).astype(np.int64)


def sparse_volumes(pair):
    """(xchg_send[P], xchg_recv[P]) of the sparse exchange."""
    P = pair.shape[0]
    return pair.sum(axis=1) + 2 * (P - 1), pair.sum(axis=0) + 2 * (P - 1)


# ---- geometry ------------------------------------------------------------------------------------
def n_chunks(C):
    return max(1, C // K_XCDS)


def classes_with_rows(n_local, C):
    """Column classes that hold at least one of a part's n_local rows (dealt round-robin)."""
    return min(n_local, C)


def chunks_with_rows(n_local, C):
    """Exchange chunks that hold at least one of a part's rows, ascending."""
    return sorted({(j % C) // K_XCDS for j in range(min(n_local, C))}) if C > 1 else ([0] if n_local else [])


def hot_kp(hot_slots, P):
    """Hot-set slots per part and class at P > kMaxPackParts (below, the piece table takes some)."""
    return (K_HOT_SLOTS_DEFAULT if hot_slots < 0 else hot_slots) // P


# ---- graphs whose partition is known by construction ------------------------------------------
def _ring_graph(P, rows, sinks, cross):
    """P * rows sources (IDs 0 .. P rows - 1, ID % P = owner, i = ID / P the index inside the owner)
    and P * sinks sink-only vertices at the highest IDs (again ID % P = owner).  Source i links to
    source (i + 1) % rows of its owner, and to sink i of its owner if i < sinks, else to source
    (i + 2) % rows of its owner -- or, for the sources i >= sinks of part 0 when `cross`, to source
    i of part 1."""
    if rows < 3 or not 1 <= sinks < rows or (cross and P < 2):
        raise ValueError("rows >= 3, 1 <= sinks < rows, and two parts for a cross link")
    n_src = P * rows
    V = n_src + P * sinks
    src, dst = [], []
    for p in range(P):
        for i in range(rows):
            u = p + i * P
            src.append(u)
            dst.append(p + ((i + 1) % rows) * P)
            src.append(u)
            if i < sinks:
                dst.append(n_src + p + i * P)
            elif cross and p == 0:
                dst.append(1 + i * P)
            else:
                dst.append(p + ((i + 2) % rows) * P)
    return V, np.array(src, np.int32), np.array(dst, np.int32)


def isolated(P, rows=6, sinks=1):
    """Every edge stays inside its owner: the parts exchange nothing but the slots."""
    return _ring_graph(P, rows, sinks, False)


def one_way(P, rows=6, sinks=1):
    """isolated(), except that the sources of part 0 that feed no sink link into part 1 instead:
    the only run that carries contributions is 0 -> 1, with rows - sinks entries."""
    return _ring_graph(P, rows, sinks, True)


# ---- the cases of tests/test_gpu_partition_edges.py -------------------------------------------
# Layout = (name for the test ID, PageRankGraph's layout, its classes or None for the fused layout)
FUSED = ("fused", "fused", None)
SPLIT8 = ("c8", "split", 8)
SPLIT16 = ("c16", "split", 16)
SPLIT64 = ("c64", "split", 64)

# Group 1, many parts: one graph (V prime, so the parts' sizes differ by one; a hub row cut into
# pieces) at P = 9 .. 64.  (P, layout, hot_slots or None where the layout has no hot set)
MANY_V, MANY_E, MANY_HUB, MANY_SEED = 20011, 266000, 0.05, 1234  # ~250 000 records after the sinks' are dropped
MANY_SINK_EVERY = 16  # one vertex in 16 is sink-only: every part of 64 owns some, so every slot counts
MANY_CASES = [
    (9, FUSED, None), (9, SPLIT16, -1), (9, SPLIT64, 40),
    (16, SPLIT16, 100), (16, SPLIT64, -1),
    (33, FUSED, None), (33, SPLIT16, 40), (33, SPLIT64, 100),
    (64, FUSED, None), (64, SPLIT16, -1), (64, SPLIT64, 100), (64, SPLIT16, 40), (64, SPLIT64, 40),
]
QUERY_P = 16  # group 5: top-K and the teleport vector on the same graph

# Group 3, tiny and lopsided: (V, P) with random_edges(V, E).  What each is there for:
#   zero   some parts own no row (V < P)
#   classes{C}  n_local < C: whole column classes of the split layout are empty
#   chunks64    at 64 classes, exchange chunks past the part's rows carry nothing (the last: slots)
TinyCase = namedtuple("TinyCase", "V P E seed")
TINY_CASES = [TinyCase(1, 2, 3, 11), TinyCase(2, 2, 4, 12), TinyCase(5, 8, 8, 13), TinyCase(16, 16, 24, 14),
              TinyCase(65, 64, 100, 15), TinyCase(100, 64, 150, 16), TinyCase(2000, 64, 3000, 17)]
TINY_LAYOUTS = [FUSED, SPLIT8, SPLIT64]
TINY_P_NOLINK = 0.2
TINY_NONE = (TinyCase(100, 64, 150, 16), SPLIT8)  # the one run with dangling = "none"
TINY_CHUNKED = (TinyCase(2000, 64, 3000, 17), SPLIT64)  # xchg_chunks 1 against 0


def tiny_edges(case):
    rng = np.random.default_rng(case.seed)
    return random_edges(rng, case.V, case.E, p_nolink=TINY_P_NOLINK)


def many_edges():
    """random_edges, then every record of the vertices ID % MANY_SINK_EVERY == MANY_SINK_EVERY - 1
    dropped: they stay as link targets only (sinks).  With 12 out-links per vertex random_edges alone
    leaves no sink, dc would be 0 and the slots of 63 peers would carry nothing to check."""
    rng = np.random.default_rng(MANY_SEED)
    src, dst = random_edges(rng, MANY_V, MANY_E, hub_frac=MANY_HUB)
    keep = src % MANY_SINK_EVERY != MANY_SINK_EVERY - 1
    return src[keep], dst[keep]


# Group 4, silent peers
SILENT_P = [2, 8, 9, 64]
SILENT_BUILDERS = {"isolated": isolated, "one_way": one_way}
SILENT_LAYOUTS = [FUSED, SPLIT8]
SILENT_ROWS, SILENT_SINKS = 6, 1
