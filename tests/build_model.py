"""A plain numpy model of the canonical graph build, an edge-list builder that lands on exact counts,
and the launch arithmetic of the build's sort and compaction (TEST INFRASTRUCTURE ONLY).

The device build (csrc/pr_build.hip) packs every record into a (dst << b | src) key (its stage
pack_inputs), radix-sorts the keys (csrc/pr_sort.hip) and drops adjacent duplicates with a
two-launch compaction (csrc/pr_compact.h; sort_dedupe), and derives the in-link CSR, the
out-degrees, the vertex flags and five counters (canonical_csr).  `build` below
restates the result with np.unique and np.bincount; it shares no code with the library or with
oracle/pagerank_oracle.c, and tests/test_build_model_cpu.py holds it to that oracle bit for bit.

`edge_list` makes inputs whose raw count E, unique count m and number of records without links are
exact, with duplicate runs at chosen positions of the sorted key array, so that a case can sit on one
loop boundary of the kernels.  `sort_shape` and `compact_shape` say which boundary that is; CASES is
the table tests/test_gpu_build_edges.py runs and tests/test_build_model_cpu.py checks.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

# include/pagerank_hip.h PR_VF_*
PR_VF_KEY, PR_VF_SINK, PR_VF_NOLINK, PR_VF_INDEG0 = 1, 2, 4, 8

# These restate constants of the kernels: kTile = kSortThreads * kSortKPT and kMaxSortWG of
# csrc/pr_sort.hip, kCompactTile = kCompactThreads * kCompactIPT and the 2048-workgroup cap of
# compact_index in csrc/pr_compact.h, and the 8-bit digit of radix_sort_u64.  A one-line comment next
# to each of them points back here: change both sides together.
SORT_TILE = 2048
SORT_WAVE_SLICE = 512  # kSortKPT * 64 keys of one wave inside a tile
SORT_MAX_WG = 2048
SORT_DIGIT_BITS = 8
COMPACT_TILE = 2048
COMPACT_IPT = 8  # consecutive items of one thread
COMPACT_MAX_WG = 2048
SCAN_THREADS = 1024  # k_scan_hist's one workgroup


@dataclass
class Model:
    n_vertices: int
    row_ptr: np.ndarray  # int64[V+1]
    col_idx: np.ndarray  # int32[m]
    out_deg: np.ndarray  # int32[V]
    vflags: np.ndarray  # uint8[V]
    counters: dict  # n_vertices, n_edges, n_sink, n_nolink, n_indeg0, max_indeg (info()'s names)

    @property
    def n_edges(self) -> int:
        return int(self.col_idx.shape[0])


def build(V: int, src, dst) -> Model:
    """The canonical build of (V, src, dst): dst == -1 is a record without links."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    if src.shape != dst.shape or src.ndim != 1:
        raise ValueError("src and dst must be 1-D arrays of the same length")
    if src.size and (src.min() < 0 or src.max() >= V or dst.min() < -1 or dst.max() >= V):
        raise ValueError("an ID outside [0, V) (dst may be -1)")
    real = dst >= 0
    keys = np.unique(dst[real] * V + src[real])  # (dst, src) order, duplicates gone
    d, s = keys // max(V, 1), keys % max(V, 1)
    indeg = np.bincount(d, minlength=V).astype(np.int64)
    row_ptr = np.zeros(V + 1, np.int64)
    row_ptr[1:] = np.cumsum(indeg)
    out_deg = np.bincount(s, minlength=V).astype(np.int32)
    is_key = np.zeros(V, bool)
    is_key[src] = True  # a record without links still makes its src a key
    appears = is_key.copy()
    appears[dst[real]] = True
    if not appears.all():
        raise ValueError("an ID in [0, V) never appears")
    vflags = np.where(is_key, PR_VF_KEY, PR_VF_SINK).astype(np.uint8)
    vflags[is_key & (out_deg == 0)] |= PR_VF_NOLINK
    vflags[indeg == 0] |= PR_VF_INDEG0
    counters = dict(n_vertices=int(V), n_edges=int(keys.shape[0]), n_sink=int((~is_key).sum()),
                    n_nolink=int((is_key & (out_deg == 0)).sum()), n_indeg0=int((indeg == 0).sum()),
                    max_indeg=int(indeg.max()) if V else 0)
    return Model(int(V), row_ptr, s.astype(np.int32), out_deg, vflags, counters)


# ---- launch arithmetic ---------------------------------------------------------------------------
def bits_for(v: int) -> int:
    """pr_internal.h bits_for: the fewest bits b >= 1 with 2^b > v."""
    b = 1
    while (1 << b) <= v:
        b += 1
    return b


def sort_shape(n: int, bits: int) -> dict:
    """radix_sort_u64(keys, tmp, n, 0, bits): the grid and the passes it runs."""
    if n <= 1 or bits <= 0:  # returns before any launch
        return dict(ntiles=0, nwg=0, tiles_per_wg=0, passes=0, last_nbits=0, tail=0, scan_per=0)
    ntiles = -(-n // SORT_TILE)
    nwg = min(ntiles, SORT_MAX_WG)
    tpw = -(-ntiles // nwg)
    nwg = -(-ntiles // tpw)
    passes = -(-bits // SORT_DIGIT_BITS)
    last = bits - SORT_DIGIT_BITS * (passes - 1)
    return dict(ntiles=ntiles, nwg=nwg, tiles_per_wg=tpw, passes=passes, last_nbits=last,
                tail=n % SORT_TILE,  # keys of the partial last tile; 0: the last tile is full
                scan_per=-(-256 * nwg // SCAN_THREADS))  # histogram words per k_scan_hist thread


def compact_shape(n: int) -> dict:
    """compact_index over [0, n): the grid of k_compact_count / k_compact_write."""
    if n <= 0:
        return dict(ntiles=0, nwg=0, tiles_per_wg=0, tail=0)
    ntiles = -(-n // COMPACT_TILE)
    nwg = min(ntiles, COMPACT_MAX_WG)
    tpw = -(-ntiles // nwg)
    nwg = -(-ntiles // tpw)
    return dict(ntiles=ntiles, nwg=nwg, tiles_per_wg=tpw, tail=n % COMPACT_TILE)


# ---- edge lists on exact counts ------------------------------------------------------------------
def _corner_pairs(V: int):
    out = []
    for p in ((0, 0), (V - 1, V - 1), (0, V - 1), (V - 1, 0)):  # (src, dst)
        if p not in out:
            out.append(p)
    return out


def run_copies(m: int, n_real: int, runs: Sequence[Tuple[int, int]], rng) -> np.ndarray:
    """Copies of each unique key, in sorted key order, so that every (start, length) of `runs` is a
    run of equal keys at sorted positions [start, start + length) of the n_real real records.  Keys
    before and between the runs are single; what is left is spread over the keys behind the last run."""
    copies = np.ones(m, np.int64)
    pos = u = 0
    for start, length in sorted(runs):
        if start < pos or length < 1:
            raise ValueError("duplicate runs overlap")
        u += start - pos
        if u >= m:
            raise ValueError("a duplicate run lies beyond the last unique key")
        copies[u] = length
        pos, u = start + length, u + 1
    extra = n_real - pos - (m - u)
    if extra < 0 or (extra > 0 and u == m):
        raise ValueError("the runs do not fit E, m and the number of records without links")
    if extra:
        copies[u:] += rng.multinomial(extra, np.full(m - u, 1.0 / (m - u)))
    assert copies.sum() == n_real
    return copies


def edge_list(V: int, E: int, m: int, n_nolink: int = 0, seed: int = 0, runs: Sequence[Tuple[int, int]] = (),
              order: str = "shuffle", cover: bool = False):
    """(src, dst) int32 of E records: m distinct edges, E - m - n_nolink further copies of them and
    n_nolink records without links, every ID of [0, V) appearing.

    The m pairs are drawn without replacement from V * V after the pairs (0->0), (V-1->V-1), (0->V-1),
    (V-1->0) and, with cover, (v -> v+1 mod V) for every even v, as far as m has room.  `runs` places
    duplicate runs (run_copies).  Records without links go to the IDs no edge mentions first, then to
    random ones; when there are too few of them for that, the builder fails.  order: 'shuffle' (all
    records), 'real_first' or 'real_last' (each group shuffled, the edges before / behind the rest).
    """
    if min(V, E, m, n_nolink) < 0 or V < 1 or m + n_nolink > E or m > V * V or (m == 0) != (E == n_nolink):
        raise ValueError("inconsistent V, E, m, n_nolink")
    rng = np.random.default_rng(seed)
    forced = _corner_pairs(V)
    if cover:
        forced += [p for p in ((v, (v + 1) % V) for v in range(0, V, 2)) if p not in forced]
    fk = np.array([d * V + s for s, d in forced[:m]], np.int64)
    need = m - fk.shape[0]
    if need > 0:
        if V * V <= max(4 * m, 1 << 16):
            cand = rng.permutation(V * V)
        else:  # sparse: draw with replacement, keep the distinct ones in draw order
            cand = rng.integers(0, V * V, size=need + need // 4 + 64 + 2 * fk.shape[0], dtype=np.int64)
            _, first = np.unique(cand, return_index=True)
            cand = cand[np.sort(first)]
        cand = cand[~np.isin(cand, fk)][:need]
        if cand.shape[0] != need:
            raise ValueError("could not draw m distinct pairs")
        fk = np.concatenate([fk, cand])
    keys = np.sort(fk)
    n_real = E - n_nolink
    copies = run_copies(m, n_real, runs, rng) if m else np.zeros(0, np.int64)
    real = np.repeat(keys, copies)
    rs, rd = real % V, real // V
    seen = np.zeros(V, bool)
    seen[rs] = True
    seen[rd] = True
    miss = np.nonzero(~seen)[0]
    if miss.shape[0] > n_nolink:
        raise ValueError(f"{miss.shape[0]} IDs never appear and only {n_nolink} records without links")
    ns = np.concatenate([miss, rng.integers(0, V, size=n_nolink - miss.shape[0], dtype=np.int64)])
    pr, pn = rng.permutation(n_real), rng.permutation(n_nolink)
    rs, rd, ns = rs[pr], rd[pr], ns[pn]
    nd = np.full(n_nolink, -1, np.int64)
    if order == "real_first":
        src, dst = np.concatenate([rs, ns]), np.concatenate([rd, nd])
    elif order == "real_last":
        src, dst = np.concatenate([ns, rs]), np.concatenate([nd, rd])
    elif order == "shuffle":
        p = rng.permutation(E)
        src, dst = np.concatenate([rs, ns])[p], np.concatenate([rd, nd])[p]
    else:
        raise ValueError("order must be 'shuffle', 'real_first' or 'real_last'")
    return src.astype(np.int32), dst.astype(np.int32)


def sorted_real_keys(V: int, src, dst) -> np.ndarray:
    """The real records' keys in the order the first sort leaves them (the sentinels follow)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    real = dst >= 0
    return np.sort(dst[real] * V + src[real])


def run_crosses(keys: np.ndarray, pos: int) -> bool:
    """True when sorted positions pos - 1 and pos hold the same key: a duplicate run straddles pos."""
    return 0 < pos < keys.shape[0] and keys[pos - 1] == keys[pos]


# ---- the cases -----------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    group: str
    V: int
    E: int
    m: int
    n_nolink: int = 0
    runs: tuple = ()
    order: str = "shuffle"
    cover: bool = False
    seed: int = 0
    # what the case is in the table for: facts()[key] == value, checked on the CPU
    expect: dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def big(self) -> bool:  # above 1 M edges: one layout, thinned on the CPU
        return self.E > (1 << 20)


def _tail_cases():
    # sort tile tail: n at tile edges (2048 q +- 1), wave-slice edges inside a tile (512 w +- 1) and
    # ballot-row edges (64 j +- 1).  V = 300 needs 150 edges for every ID to appear, so the counts
    # below that use the largest V they can cover.  (ntiles, tail) are written out, not computed.
    table = {1: (0, 0), 2: (1, 2), 63: (1, 63), 64: (1, 64), 65: (1, 65), 511: (1, 511), 512: (1, 512), 513: (1, 513),
             2047: (1, 2047), 2048: (1, 0), 2049: (2, 1), 4095: (2, 2047), 4096: (2, 0), 4097: (3, 1), 6145: (4, 1)}
    out = []
    for E, (ntiles, tail) in table.items():
        V = 300 if E >= 511 else min(E, 60)
        out.append(Case(f"tail_E{E}", "sort tile tail", V, E, E, cover=True, seed=100 + E,
                        expect=dict(E=E, m=E, ntiles=ntiles, tail=tail, tiles_per_wg=min(ntiles, 1))))
    return out


def _dedupe_cases():
    out = []
    for m in (2047, 2048, 2049, 4096):
        # runs: the smallest key (i == 0 starts a run), one across an 8-item slice edge (807 | 808) and
        # one across the compaction tile edge 2047 | 2048
        out.append(Case(f"dedupe_m{m}", "dedupe tile", 300, 3 * m, m, runs=((0, 3), (806, 3), (2040, 16)), cover=True,
                        seed=200 + m, expect=dict(E=3 * m, m=m, m_tail=m % 2048, run_at_0=True, run_at_808=True,
                                                  run_at_2048=True, compact_ntiles=-(-3 * m // 2048))))
    out.append(Case("dedupe_m1_V1", "dedupe extremes", 1, 5000, 1, seed=1,
                    expect=dict(m=1, E=5000, run_at_0=True, run_at_2048=True, run_at_4096=True, compact_ntiles=3)))
    out.append(Case("dedupe_m1_V2", "dedupe extremes", 2, 5000, 1, n_nolink=1, seed=2,
                    expect=dict(m=1, E=5000, run_at_0=True, run_at_2048=True, run_at_4096=True, first_key=0)))
    out.append(Case("dedupe_m0", "dedupe extremes", 4097, 4097, 0, n_nolink=4097, seed=3,
                    expect=dict(m=0, E=4097, ntiles=3, tail=1, n_nolink=4097, n_indeg0=4097)))
    return out


def _width_cases():
    # V at 2^k - 1, 2^k, 2^k + 1: (2b, passes, last digit's bits) written out.  V = 100 adds the 6-bit
    # last digit (2b = 14) that the powers of two above never give.
    table = {1: (2, 1, 2), 2: (4, 1, 4), 3: (4, 1, 4), 15: (8, 1, 8), 16: (10, 2, 2), 17: (10, 2, 2), 100: (14, 2, 6),
             255: (16, 2, 8), 256: (18, 3, 2), 257: (18, 3, 2), 4095: (24, 3, 8), 4096: (26, 4, 2), 4097: (26, 4, 2),
             65535: (32, 4, 8), 65536: (34, 5, 2), 65537: (34, 5, 2)}
    out = []
    for V, (two_b, passes, last) in table.items():
        E = 4 * V + 1
        if V <= 3:  # every possible pair, plus duplicates
            m, nl = V * V, 1
        else:
            m, nl = 3 * V, V // 2 + 1
        out.append(Case(f"width_V{V}", "key width", V, E, m, n_nolink=nl, seed=300 + V,
                        expect=dict(E=E, m=m, two_b=two_b, passes=passes, last_nbits=last, has_top_key=True)))
    return out


def _sentinel_cases():
    return [Case(f"sentinel_{o}", "sentinel-heavy", 3000, 20000, 1500, n_nolink=18000, order=o, seed=400 + i,
                 expect=dict(E=20000, n_nolink_records=18000, m=1500))
            for i, o in enumerate(("shuffle", "real_first", "real_last"))]


def _big_cases():
    full = 2048 * 2048  # 4 194 304: the most keys with one tile per workgroup
    return [
        Case("tpw1_full", "two tiles per workgroup", 3000, full, 3_000_000, n_nolink=1000, seed=500,
             expect=dict(E=full, tiles_per_wg=1, nwg=2048, tail=0, compact_tpw=1)),
        Case("tpw2_first", "two tiles per workgroup", 3000, full + 1, 3_000_000, n_nolink=1000, seed=501,
             expect=dict(E=full + 1, tiles_per_wg=2, nwg=1025, tail=1, compact_tpw=2, ntiles=2049)),
        Case("tpw2_dedup", "two tiles per workgroup", 4000, 6_000_000, 5_000_000, n_nolink=1000, seed=502,
             expect=dict(E=6_000_000, m=5_000_000, tiles_per_wg=2, compact_tpw=2, m_tpw=2, m_past_full=True)),
    ]


CASES = _tail_cases() + _dedupe_cases() + _width_cases() + _sentinel_cases() + _big_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# (case, P) built as parts of a row partition
PART_CASES = [("dedupe_m2048", 2), ("dedupe_m2048", 3), ("tpw2_dedup", 2), ("tpw2_dedup", 3)]


@functools.lru_cache(maxsize=None)
def case_inputs(name: str):
    """(src, dst, model) of a case, made once per process and shared read-only."""
    c = CASE_BY_NAME[name]
    src, dst = edge_list(c.V, c.E, c.m, c.n_nolink, c.seed, c.runs, c.order, c.cover)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst, build(c.V, src, dst)


def facts(c: Case, src, dst, model: Model) -> dict:
    """What a case's inputs reach, from the launch arithmetic and the inputs themselves."""
    two_b = 2 * bits_for(c.V)
    s1 = sort_shape(int(src.shape[0]), two_b)  # the first sort: every raw record
    c1 = compact_shape(int(src.shape[0]))  # the dedupe reads the sorted raw records
    cm = compact_shape(model.n_edges)  # the per-part filter reads the unique keys
    keys = sorted_real_keys(c.V, src, dst)
    f = dict(E=int(src.shape[0]), m=model.n_edges, n_nolink_records=int((np.asarray(dst) < 0).sum()), two_b=two_b,
             ntiles=s1["ntiles"], nwg=s1["nwg"], tiles_per_wg=s1["tiles_per_wg"], passes=s1["passes"],
             last_nbits=s1["last_nbits"], tail=s1["tail"], scan_per=s1["scan_per"],
             compact_ntiles=c1["ntiles"], compact_tpw=c1["tiles_per_wg"], m_tail=model.n_edges % COMPACT_TILE,
             m_tpw=cm["tiles_per_wg"], m_past_full=model.n_edges > SORT_TILE * SORT_MAX_WG,
             first_key=int(keys[0]) if keys.size else None,
             run_at_0=keys.size > 1 and keys[0] == keys[1],
             has_top_key=keys.size > 0 and int(keys[-1]) == c.V * c.V - 1,
             n_nolink=model.counters["n_nolink"], n_indeg0=model.counters["n_indeg0"])
    for pos in (808, 2048, 4096):
        f[f"run_at_{pos}"] = bool(run_crosses(keys, pos))
    return f
