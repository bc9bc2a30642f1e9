"""Exact, order-free expected bits for the engine's teleport dangling mode (pr_set_teleport_dangling).

exact_model.dyadic_run restated for the iteration

    q     = dc / ts
    r'[v] = t[v] + damping * (S[v] + q * t[v])

on exact_model.Graph inputs.  The family: every source has a power-of-two out-degree, damping is
2^-s, the initial ranks and the teleport terms are non-negative multiples of 2^-4, and ts -- the exact
sum of the teleport vector -- is a power of two 2^k with k >= 0.  Then dc / ts is a shift, q * t[v] is
the product of two integers on a grid, all addends are non-negative, and as long as every total stays
below 2^53 on its grid every sum is exact in any order: one correct bit pattern per iteration, whatever
the layout, the partition or the order of the dangling and L1 partials.  The model carries integers,
checks that bound itself and stops where it ends (`exact_iters`); it raises ValueError for an input
outside the family.  numpy and Python integers only.

float_run is the same iteration in float64 with one ufunc call per operation, for the CPU test that
holds the integer recurrence to it.
"""
import numpy as np

import exact_model as em
from exact_model import DyadicRun, GRID_BITS, MANT, _bits, _int_sum, _on_grid, _pow2_shift


def seed_vector(g, hub, weights=(4.0, 2.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 0.0625)):
    """(ids, values, dense vector): len(weights) seeds, zero elsewhere.  The seeds are the hub, the first
    sink, the first source without in-links, and the lowest other IDs; the weights are given in that
    order (so the hub's term is the largest and a lost q * t shows on its row)."""
    sink = np.nonzero(g.sink)[0]
    lonely = np.nonzero(~g.has_in & ~g.sink)[0]
    if sink.size == 0 or lonely.size == 0:
        raise ValueError("the input needs a sink and a source without in-links")
    ids = [int(hub), int(sink[0]), int(lonely[0])]
    v = 0
    while len(ids) < len(weights):
        if v not in ids:
            ids.append(v)
        v += 1
    ids = np.array(ids, np.int32)
    values = np.array(weights, np.float64)
    t = np.zeros(g.V)
    t[ids] = values
    return ids, values, t


def dangling_run(g, iters, teleport, damping=0.5, init=None):
    """The teleport dangling mode on Graph `g` with the V teleport terms `teleport`.  Returns
    exact_model.DyadicRun: ranks[k], dc[k], l1[k] of iteration k + 1 for as many iterations (<= iters)
    as every quantity is certified exact, exact_iters, grid_bits, width_bits."""
    V = g.V
    d = g.out_deg
    if g.nolink.any() or (d[~g.sink] & (d[~g.sink] - 1)).any():
        raise ValueError("every source's out-degree must be a power of two")
    lgd = np.zeros(V, np.int64)
    lgd[~g.sink] = np.round(np.log2(d[~g.sink])).astype(np.int64)
    lgd_max = int(lgd.max()) if V else 0
    s_damp = _pow2_shift(damping, "damping")
    t_int = _on_grid(teleport, "teleport terms")
    if t_int.shape != (V,):
        raise ValueError("teleport: V values")
    ts_int = _int_sum(t_int)  # on grid GRID_BITS
    if ts_int <= 0 or ts_int & (ts_int - 1) or ts_int < (1 << GRID_BITS):
        raise ValueError("ts must be a power of two 2^k with k >= 0")
    lgts = ts_int.bit_length() - 1 - GRID_BITS
    r_int = _on_grid(np.ones(V) if init is None else init, "initial ranks")
    if r_int.shape != (V,):
        raise ValueError("init: V values")
    F = GRID_BITS
    while F > 0 and not (r_int & 1).any():
        r_int >>= 1
        F -= 1
    t_bits = GRID_BITS
    while t_bits > 0 and not (t_int & 1).any():
        t_int >>= 1
        t_bits -= 1
    t_max = int(t_int.max())

    ranks, dcs, l1s, grid, width = [], [], [], [], []
    l1_ok = True
    n_l1 = 0
    for _ in range(iters):
        G = F + lgd_max  # contributions: r / d
        c_int = r_int << (lgd_max - lgd)
        c_int[g.sink] = 0
        c_max = int(c_int.max()) if V else 0
        if _bits(c_max) > MANT:
            break
        s_hi = g.row_sums(c_int >> em._HALF)  # in two halves, so that no int64 sum can wrap
        if _bits(int(s_hi.max())) + em._HALF > 62:
            break
        S = (s_hi << em._HALF) + g.row_sums(c_int & ((1 << em._HALF) - 1))
        S[~g.has_in] = r_int[~g.has_in] << lgd_max  # the old rank as the sum
        dc_int = _int_sum(r_int[g.sink])  # on grid F; q = dc / ts is the same integer on grid F + lgts
        if _bits(dc_int) > MANT or _bits(dc_int) + _bits(t_max) > 62:
            break
        Q = F + lgts + t_bits  # q * t: the product of two integers
        qt_int = t_int * np.int64(dc_int)
        G2 = max(G, Q)
        x_int_hi = max(_bits(int(S.max())) + (G2 - G), _bits(int(qt_int.max())) + (G2 - Q))
        if x_int_hi > 61:
            break
        x_int = (S << (G2 - G)) + (qt_int << (G2 - Q))  # S + q * t
        Fn = max(G2 + s_damp, t_bits)  # damping * x is the same integer on grid G2 + s
        if _bits(int(x_int.max())) + (Fn - G2 - s_damp) > 62 or _bits(t_max) + Fn - t_bits > 62:
            break
        rn_int = (t_int << (Fn - t_bits)) + (x_int << (Fn - G2 - s_damp))
        w = max(_bits(c_max), _bits(int(S.max())), _bits(dc_int), _bits(int(qt_int.max())), _bits(int(x_int.max())),
                _bits(int(rn_int.max())))
        if w > MANT:
            break
        l1_int = _int_sum(np.abs(rn_int - (r_int << (Fn - F))))
        l1_ok = l1_ok and _bits(l1_int) <= MANT
        n_l1 += l1_ok
        ranks.append(np.ldexp(rn_int.astype(np.float64), -Fn))
        dcs.append(float(np.ldexp(float(dc_int), -F)))
        l1s.append(float(np.ldexp(float(l1_int), -Fn)) if l1_ok else float("nan"))
        grid.append(Fn)
        width.append(w)
        r_int, F = rn_int, Fn
    n = len(ranks)
    return DyadicRun(ranks, np.array(dcs), np.array(l1s), {"ranks": n, "dc": n, "l1": n_l1}, grid, width)


def float_run(g, iters, teleport, damping, ts, init=None, dangling="local"):
    """The mode's specification in float64, every operation a ufunc call of its own and numpy's
    sequential sums; `ts` as the caller formed it.  Returns (ranks[k], dc[k], l1[k])."""
    V = g.V
    r = np.ones(V) if init is None else np.array(init, np.float64)
    t = np.asarray(teleport, np.float64)
    d = np.where(g.out_deg > 0, g.out_deg, 1).astype(np.float64)
    ranks, dcs, l1s = [], [], []
    for _ in range(iters):
        c = np.divide(r, d)
        c[g.out_deg == 0] = 0.0
        S = g.row_sums(c)
        S[~g.has_in] = r[~g.has_in]
        dc = float(np.add.reduce(r[g.sink])) if dangling == "local" else 0.0
        q = np.divide(np.float64(dc), np.float64(ts))
        x = np.add(S, np.multiply(q, t))
        rn = np.add(t, np.multiply(np.float64(damping), x))
        ranks.append(rn)
        dcs.append(dc)
        l1s.append(float(np.add.reduce(np.abs(np.subtract(rn, r)))))
        r = rn
    return ranks, np.array(dcs), np.array(l1s)
