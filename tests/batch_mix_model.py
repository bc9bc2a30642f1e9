"""A numpy model of the batch mixes (include/pagerank_hip.h, pr_batch_mix_topk / pr_batch_mix_get).

blend(weights, cols): m[v] over the columns j = 0 .. width-1 in ascending order; a column whose
weight is exactly 0.0 (either sign) takes no part; the first participating column gives w_j * r_j,
every later one acc + w_j * r_j.  numpy's float64 `*` and `+` on arrays are separate IEEE operations
(no fused multiply-add), which is the definition.  A mix with no non-zero weight is +0.0 everywhere.

listing(scores, k, excluded): the IDs and scores of pr_get_topk's order -- score descending by the
order-preserving u64 image of the IEEE bits (-0.0 just below +0.0), ties by ID ascending -- over
the vertices the mix does not exclude.  numpy only; imports nothing from sparky_hip."""
import numpy as np


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def rank_keys(x):
    b = bits(x)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def blend(weights, cols):
    """weights: float64[width]; cols: the width columns, float64[V] each.  Returns float64[V]."""
    weights = np.asarray(weights, np.float64)
    assert weights.ndim == 1 and len(cols) == weights.shape[0]
    V = len(cols[0]) if len(cols) else 0
    acc = None
    with np.errstate(all="ignore"):
        for w, r in zip(weights, cols):
            if w == 0.0:
                continue
            p = np.float64(w) * np.asarray(r, np.float64)
            acc = p if acc is None else acc + p
    return np.zeros(V, np.float64) if acc is None else acc


def listing(scores, k, excluded=()):
    own = np.setdiff1d(np.arange(len(scores)), np.asarray(excluded, np.int64))
    o = own[np.lexsort((own, ~rank_keys(scores[own])))][: max(int(k), 0)]
    return o.astype(np.int32), scores[o]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
