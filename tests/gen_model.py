"""A plain model of the synthetic-graph generators and of first-appearance interning
(csrc/pr_gen.hip: k_gen_rmat, k_gen_er, k_gen_chunglu, pr_intern_device).  numpy and Python integers
only; it imports nothing from sparky_hip and loads no shared library.  tests/test_gen_model_cpu.py
checks the model against the definition below without a GPU, tests/test_gpu_generators.py holds the
kernels to the model, bit for bit.

The definition ("Generators"), all arithmetic modulo 2^64 unless said otherwise:

  splitmix64(x)      x += 0x9E3779B97F4A7C15; x = (x ^ x>>30) * 0xBF58476D1CE4E5B9;
                     x = (x ^ x>>27) * 0x94D049BB133111EB; return x ^ x>>31
  edge_hash(s, i, k) splitmix64(s * 0xD1B54A32D192ED03 ^ splitmix64(i * 0x9E3779B97F4A7C15 + k))
                     -- a function of (seed, edge index, draw index) alone: edge i does not depend
                     on the number of edges asked for
  scramble(v)        with mask = 2^scale - 1, m1 = splitmix64(s+11)|1, m2 = splitmix64(s+13)|1,
                     a1 = splitmix64(s+17), a2 = splitmix64(s+19):
                     x = (v*m1 + a1) & mask; x ^= x >> (scale+1)/2; x = (x*m2 + a2) & mask;
                     x ^= x >> (scale+2)/3;  x = (x*m1) & mask       (integer divisions)
                     -- odd multiplies, adds and xorshifts are each invertible modulo 2^scale

  R-MAT   bit level l of edge i takes the 32-bit draw u = half (l & 1) of edge_hash(seed, i, l >> 1),
          low half first.  With thr(p) = min(trunc(p * 2^32), 0xFFFFFFFF) and ta = thr(a),
          tab = thr(a + b), tabc = thr((a + b) + c):
              u <  ta          quadrant a  (src bit 0, dst bit 0)
              ta  <= u < tab   quadrant b  (0, 1)
              tab <= u < tabc  quadrant c  (1, 0)
              u >= tabc        quadrant d  (1, 1)
          (the Graph500 convention); level l sets bit l; both labels then go through scramble().
  ER      src = low half of edge_hash(seed, i, 0) & mask, dst = high half & mask.
  Chung-Lu  n_src = trunc(src_frac * n_labels).  A law (gamma, v0, n) has a = 1 - 1/(gamma - 1),
          lo = v0^a, span = (n + v0)^a - lo.  A draw h gives u = (h >> 11) * 2^-53,
          x = (lo + u*span)^(1/a) - v0 (the inverse transform of the density ~ (r + v0)^(a-1) on
          [0, n)), rank = clamp(trunc(x), 0, n - 1).  Edge i: source rank from edge_hash(seed, i, 0)
          under (gamma_out, v0_out, n_src), target rank from edge_hash(seed, i, 1) under
          (gamma_in, v0_in, n_labels).  Record E + j (j < n_nolink) has source rank n_src + j and
          target -1.  label = (rank * mul + add) mod n_labels with
          mul = (splitmix64(seed+23) mod n_labels) | 1, then += 2 until gcd(mul, n_labels) == 1,
          add = splitmix64(seed+29) mod n_labels.
  Interning  occurrence positions are 2i for src[i] and 2i+1 for dst[i]; dst == -1 is no
          occurrence.  Labels are numbered 0, 1, ... by the position of their first occurrence.

The Chung-Lu ambiguity band
---------------------------
power_rank is the only floating-point step.  lo, span and 1/a are computed on the host by both
sides (C pow, one division) and are taken as equal.  The model computes y = lo + u*span with two
roundings and x = pow(y, 1/a) - v0 with the C library's pow (math.pow, element by element, so that
the result does not depend on which vector pow numpy was built with).  The device uses the device
library's pow and may contract y to an FMA (csrc/Makefile builds with -ffp-contract=off today, which
makes y equal on both sides; the band does not rely on it).  For a > 0 (gamma > 2: every case the
GPU tests run) lo, span and u*span are positive and u*span <= y, so, in units of ulp = 2^-52
relative:

  y        model 0.5 (product) + 0.5 (sum), device 0.5 (fma): they differ by <= 1.5 ulp of y,
           which pow amplifies by |1/a|                                        1.5 |1/a|
  pow      device: the double-precision bound of the HIP device library.  No document under the
           ROCm installation states it, so 2 ulp is ASSUMED here               2
           model: the C library's documented 1 ulp                              1
  x        the subtraction rounds once on each side, <= 0.5 ulp of x <= x + v0  1

all relative to t = x + v0.  A safety factor of 16 on top (the band only has to be far below the
spacing of the draws, ~2^-53 * span/(a y) * t relative, not tight):

  BAND(1/a) = 16 * (1.5 |1/a| + 4) * 2^-52

and a draw is ambiguous when |x - round(x)| <= BAND * (x + v0) with round(x) >= 1: there a faithful
device may truncate to the other side of the integer, so its rank may be the model's +-1.  (Around
0 both sides of the boundary truncate to rank 0.)  Everywhere else the device's rank must equal
the model's.
"""
import math

import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SEED_MUL = 0xD1B54A32D192ED03

# The Chung-Lu cases tests/test_gpu_generators.py runs, and tests/test_gen_model_cpu.py caps the ambiguous
# draws of: (name, n_labels, E, gamma_out, v0_out, gamma_in, v0_in, src_frac, seed).  The small case is
# test_gpu_parity.py's test_chunglu_generator_small; its composite twin takes a seed whose first multiplier
# candidate is not coprime to 30030.  The two prefixes restate sparky_hip.CHUNGLU_PRESETS (this module must
# not import the package; the GPU file takes its parameters from the package and checks that they agree).
PREFIX = 1 << 20
CHUNGLU_CASES = [
    ("small_prime", 30011, 400_000, 2.2, 20.0, 2.1, 10.0, 0.85, 5),
    ("small_composite", 30030, 400_000, 2.2, 20.0, 2.1, 10.0, 0.85, 7),
    ("lj_prefix", 4_847_571, PREFIX, 2.3, 84.0, 2.3, 84.0, 1.0, 4),
    ("twitter_prefix", 41_652_230, PREFIX, 2.2, 100.0, 2.1, 50.0, 0.85, 5),
]

POW_ULP_DEVICE = 2.0  # assumed: not documented under the ROCm installation
POW_ULP_HOST = 1.0
SAFETY = 16.0


def _u64(x):
    return U64(int(x) & MASK64)


def splitmix64(x):
    """x: uint64 array (or anything np.asarray turns into one); returns uint64 array."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U64) + U64(GOLDEN)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def splitmix64_int(x: int) -> int:
    """The same function on one Python integer."""
    x = (x + GOLDEN) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def edge_hash(seed: int, i, k: int):
    with np.errstate(over="ignore"):
        inner = splitmix64(np.asarray(i, dtype=U64) * U64(GOLDEN) + _u64(k))
        return splitmix64(_u64(seed * SEED_MUL) ^ inner)


def scramble(v, scale: int, seed: int):
    mask = U64((1 << scale) - 1)
    m1, m2 = _u64(splitmix64_int((seed + 11) & MASK64) | 1), _u64(splitmix64_int((seed + 13) & MASK64) | 1)
    a1, a2 = _u64(splitmix64_int((seed + 17) & MASK64)), _u64(splitmix64_int((seed + 19) & MASK64))
    with np.errstate(over="ignore"):
        x = np.asarray(v, dtype=U64)
        x = (x * m1 + a1) & mask
        x = x ^ (x >> U64((scale + 1) // 2))
        x = (x * m2 + a2) & mask
        x = x ^ (x >> U64((scale + 2) // 3))
        return (x * m1) & mask


def thr(p: float) -> int:
    x = p * 4294967296.0
    return 0xFFFFFFFF if x >= 4294967295.0 else int(x)


def _labels_i32(x):
    return np.asarray(x, dtype=U64).astype(np.uint32).view(np.int32)


def rmat(scale: int, E: int, a: float, b: float, c: float, seed: int, *, scrambled: bool = True, start: int = 0):
    """Edges start .. start+E-1 as (src, dst) int32 arrays; scrambled=False: the raw bit patterns."""
    if not 1 <= scale <= 31:
        raise ValueError("scale must be in [1, 31]")
    if not (a >= 0 and b >= 0 and c >= 0 and a + b + c <= 1.0):
        raise ValueError("bad R-MAT probabilities")
    ta, tab, tabc = U64(thr(a)), U64(thr(a + b)), U64(thr(a + b + c))
    i = np.arange(start, start + E, dtype=U64)
    s = np.zeros(E, U64)
    d = np.zeros(E, U64)
    for l in range(scale):
        if l % 2 == 0:
            h = edge_hash(seed, i, l >> 1)
        u = (h >> U64(32)) if l % 2 else (h & U64(0xFFFFFFFF))
        sb = u >= tab
        db = ((u >= ta) & (u < tab)) | (u >= tabc)
        s |= sb.astype(U64) << U64(l)
        d |= db.astype(U64) << U64(l)
    if scrambled:
        s, d = scramble(s, scale, seed), scramble(d, scale, seed)
    return _labels_i32(s), _labels_i32(d)


def er(scale: int, E: int, seed: int):
    if not 1 <= scale <= 31:
        raise ValueError("scale must be in [1, 31]")
    mask = U64((1 << scale) - 1)
    h = edge_hash(seed, np.arange(E, dtype=U64), 0)
    return _labels_i32(h & mask), _labels_i32((h >> U64(32)) & mask)


class PowerLaw:
    def __init__(self, gamma: float, v0: float, n: int):
        self.a = 1.0 - 1.0 / (gamma - 1.0)
        self.one_over_a = 1.0 / self.a
        self.v0 = v0
        self.lo = math.pow(v0, self.a)
        self.span = math.pow(float(n) + v0, self.a) - self.lo
        self.n = n

    def cdf(self, t):
        """P(x <= t) of the continuous draw, t in [0, n]; P(rank <= r) = cdf(r + 1) for r < n - 1."""
        return (np.power(np.asarray(t, np.float64) + self.v0, self.a) - self.lo) / self.span


_pow = np.frompyfunc(math.pow, 2, 1)


def power_rank(pl: PowerLaw, h):
    """(rank int64, x float64) of the draws h (uint64)."""
    u = (h >> U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    y = u * pl.span
    y = pl.lo + y
    x = _pow(y, pl.one_over_a).astype(np.float64) - pl.v0
    r = np.trunc(x).astype(np.int64)
    return np.clip(r, 0, pl.n - 1), x


def label_map(n_labels: int, seed: int):
    mul = (splitmix64_int((seed + 23) & MASK64) % n_labels) | 1
    add = splitmix64_int((seed + 29) & MASK64) % n_labels
    while math.gcd(mul, n_labels) != 1:
        mul += 2
    return mul, add


def apply_label_map(rank, mul: int, add: int, n_labels: int):
    """(rank * mul + add) mod n_labels as int32; the product stays far below 2^64."""
    assert (n_labels - 1) * mul + add < 1 << 64
    return ((np.asarray(rank).astype(U64) * U64(mul) + U64(add)) % U64(n_labels)).astype(np.int32)


class ChungLu:
    """src, dst: int32 labels of the E + n_nolink records.  rs, rd: int64 ranks (rd == -1 on the
    link-less records).  xs, xd: the real draws before truncation, for the E edges.  mul, add,
    n_src, n_labels, out, inn (the two PowerLaws)."""


def chunglu(n_labels: int, E: int, gamma_out: float, v0_out: float, gamma_in: float, v0_in: float,
            src_frac: float, n_nolink: int, seed: int) -> ChungLu:
    if n_labels < 1:
        raise ValueError("n_labels must be >= 1")
    if not (gamma_out > 1.0 and gamma_in > 1.0 and gamma_out != 2.0 and gamma_in != 2.0):
        raise ValueError("power-law exponents must be > 1 and != 2")
    if not (v0_out > 0.0 and v0_in > 0.0):
        raise ValueError("v0 must be > 0")
    n_src = int(src_frac * float(n_labels))
    if n_src < 1 or n_nolink < 0 or n_src + n_nolink > n_labels:
        raise ValueError("src_frac * n_labels + n_nolink must fit in [1, n_labels]")
    g = ChungLu()
    g.n_labels, g.n_src = n_labels, n_src
    g.out, g.inn = PowerLaw(gamma_out, v0_out, n_src), PowerLaw(gamma_in, v0_in, n_labels)
    g.mul, g.add = label_map(n_labels, seed)
    i = np.arange(E, dtype=U64)
    rs, g.xs = power_rank(g.out, edge_hash(seed, i, 0))
    rd, g.xd = power_rank(g.inn, edge_hash(seed, i, 1))
    g.rs = np.concatenate([rs, n_src + np.arange(n_nolink, dtype=np.int64)])
    g.rd = np.concatenate([rd, np.full(n_nolink, -1, np.int64)])
    g.src = apply_label_map(g.rs, g.mul, g.add, n_labels)
    g.dst = np.where(g.rd < 0, np.int32(-1), apply_label_map(np.maximum(g.rd, 0), g.mul, g.add, n_labels))
    return g


def band(one_over_a: float) -> float:
    """The relative half-width derived in the module docstring (a > 0 only)."""
    if not one_over_a > 0:
        raise ValueError("the band is derived for a > 0 (gamma > 2) only")
    return SAFETY * (1.5 * abs(one_over_a) + POW_ULP_DEVICE + POW_ULP_HOST + 1.0) * 2.0 ** -52


def ambiguous(x, v0: float, one_over_a: float):
    """Mask of the draws whose truncation a faithful device may round to the other side."""
    x = np.asarray(x, np.float64)
    k = np.rint(x)
    return (np.abs(x - k) <= band(one_over_a) * (x + v0)) & (k >= 1)


def first_appearance(src, dst):
    """(V, src', dst'): labels renumbered by first occurrence, positions 2i (src) and 2i+1 (dst);
    dst == -1 is no occurrence and stays -1."""
    src, dst = np.asarray(src), np.asarray(dst)
    occ = np.stack([src, dst], 1).ravel()
    pos = np.flatnonzero(occ >= 0)
    labels, first = np.unique(occ[pos], return_index=True)
    order = np.argsort(pos[first], kind="stable")
    newid = np.full(int(labels.max()) + 1 if labels.size else 1, -1, np.int64)
    newid[labels[order]] = np.arange(labels.size)
    s2 = newid[src] if src.size else np.zeros(0, np.int64)
    d2 = np.where(dst >= 0, newid[np.maximum(dst, 0)], -1) if dst.size else np.zeros(0, np.int64)
    return int(labels.size), s2.astype(np.int32), d2.astype(np.int32)
