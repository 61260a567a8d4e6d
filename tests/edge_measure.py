"""The collect / print / assert pattern of the kernel-edge suites (test_gpu_forward_edges.py, test_gpu_reverse_edges.py,
test_gpu_glow_edges.py, test_gpu_flow_edges.py).  A helper module, not a test."""
import numpy as np

from conftest import assert_close


class Measure:
    """collects |diff| / bound over the cases of one test; report() prints the largest ratio, then asserts every case (ratio <= 1)"""

    def __init__(self, kernel, suite="forward-edges"):
        self.kernel, self.suite, self.rows = kernel, suite, []

    def add(self, case, got, ref, bound):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (self.kernel, case, got.shape, ref.shape)
        bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
        diff = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(diff == 0.0, 0.0, diff / bound)          # a zero bound admits a zero difference only; NaN stays NaN
        self.rows.append((case, ratio))

    def report(self):
        worst = [(float("inf") if np.isnan(r).any() else float(r.max()) if r.size else 0.0, case) for case, r in self.rows]
        top = max(worst, key=lambda w: w[0])
        print("%s: %s: max(|diff| / bound) = %.3f over %d cases (at %s)" % (self.suite, self.kernel, top[0], len(worst), top[1]))
        for case, ratio in self.rows:
            assert_close(ratio, np.zeros_like(ratio), 0.0, atol=1.0, what="%s %s: |diff| / bound" % (self.kernel, case))
