"""The batch's teleport dangling mode (pr_batch_set_dangling, csrc/pr_batch_dangling.h) on top of the
order-exact model of tests/batch_order_model.py.  Pure numpy.

In teleport mode column j's iteration is

    q      = dc / ts                          one rounded divide
    r'[v]  = t[v] + damping * (S[v] + q * t[v])

with S the row sums of batch_order_model.BatchModel (the mode does not touch them), ts the sum of the
column's teleport vector as the device reports it, and every operation a separate element-wise
float64 numpy operation: numpy rounds each one and never contracts two of them.

Fallback: a column whose ts is exactly 0 (no vector, a padding column, a vector that sums to 0) or
not finite takes BatchModel.step, the uniform dc / N, bit for bit.
"""
import numpy as np

import batch_order_model as bom


def uses_teleport(ts):
    """csrc/pr_batch_dangling.h batch_dangling_uses_teleport: ts finite and != 0."""
    ts = float(ts)
    return bool(np.isfinite(ts)) and ts != 0.0


class DanglingModel(bom.BatchModel):
    """BatchModel plus step_teleport(): one column's iteration in PR_BATCH_DANGLING_TELEPORT."""

    def step_teleport(self, r, t, dc, ts, damping=0.85):
        """The new ranks of one column: r previous ranks, t teleport terms, dc the dangling sum used,
        ts the device's sum of t (0.0 for a column without a vector)."""
        if not uses_teleport(ts):
            return self.step(r, t, dc, damping)
        t = np.asarray(t, np.float64)
        S = self.row_sums(np.asarray(r, np.float64))
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.float64(dc) / np.float64(ts)
            term = q * t
            inner = S + term
            scaled = np.float64(damping) * inner
            return t + scaled
