"""The rule of the field-statistics launch (include/gfv.h gfv_field_stats_update) restated in numpy.

Written from the header's paragraph, not from the kernel: tests/test_fieldstats_gpu.py compares the kernel with it launch by launch,
bit for bit.  float64 operations in the order written (difference, sum, product, sum - each one rounding), np.fmin / np.fmax for
the extremes.  Nothing here touches a GPU.
"""
import numpy as np

from window_ref import COUNTER, ENABLED, LAST, N, RECORD, START, STOP, STRIDE, commit, take  # noqa: F401  (the window: once)

SUMS, AUX = 7, 9

f32, f64 = np.float32, np.float64


class FieldStatsRef:
    """The record and the state a sequence of launches works on, and `launch()`: one launch applied to them."""

    def __init__(self, n_rows, start=1, stride=1, stop=-1, enabled=1):
        self.n_rows = int(n_rows)
        self.rec = np.zeros(RECORD, dtype=np.int32)
        self.rec[[START, STRIDE, STOP, ENABLED]] = (start, stride, stop, enabled)
        self.rec[LAST] = -1
        self.sums = np.zeros((SUMS, self.n_rows), dtype=f64)
        self.aux = np.zeros((AUX, self.n_rows), dtype=f32)

    def reset(self):
        self.rec[LAST], self.rec[N] = -1, 0

    def launch(self, field, clock):
        """field [n_rows, >= 3] float32 (columns 0:3 are used), clock: the value of the clock word.  -> whether it sampled."""
        c = int(clock)
        taken = take(self.rec, c)
        if taken:
            x = np.asarray(field, dtype=f32)[:, 0:3].T                      # [3, n_rows]
            assert x.shape == (3, self.n_rows)
            if self.rec[N] == 0:
                self.aux[0:3], self.aux[3:6], self.aux[6:9] = x, x, x
                self.sums[:] = 0.0
            else:
                with np.errstate(all="ignore"):
                    d = x.astype(f64) - self.aux[0:3].astype(f64)
                    self.sums[0:3] = self.sums[0:3] + d
                    self.sums[3:6] = self.sums[3:6] + d * d
                    self.sums[6] = self.sums[6] + d[0] * d[1]
                    self.aux[3:6] = np.fmin(self.aux[3:6], x)
                    self.aux[6:9] = np.fmax(self.aux[6:9], x)
        commit(self.rec, c, taken)
        return taken

    def moments(self):
        """mean [n,3], var [n,3] (population), cov_uv [n] in float64 by the formulas of the header; min, max [n,3] float32."""
        n = int(self.rec[N])
        assert n > 0
        m1 = self.sums[0:3] / n
        return {"n": n, "mean": (self.aux[0:3].astype(f64) + m1).T, "var": (self.sums[3:6] / n - m1 * m1).T,
                "cov_uv": self.sums[6] / n - m1[0] * m1[1], "min": self.aux[3:6].T.copy(), "max": self.aux[6:9].T.copy()}


def over(fields, clocks, n_rows, **window):
    """The reference after one launch per (field, clock) pair."""
    ref = FieldStatsRef(n_rows, **window)
    for f, c in zip(fields, clocks):
        ref.launch(f, c)
    return ref


def two_pass(samples):
    """float64 two-pass statistics of samples [n, rows, 3] (fp32 data): mean, population variance, cov(u, v)."""
    x = np.asarray(samples, dtype=f64)
    mean = x.mean(axis=0)
    dev = x - mean
    return {"mean": mean, "var": (dev * dev).mean(axis=0), "cov_uv": (dev[:, :, 0] * dev[:, :, 1]).mean(axis=0)}


REL = 1e-12


def check_against_two_pass(got, x, s2n, what):
    """got: mean, var, cov_uv, min, max of the samples x [n, rows, 3]; s2n = max(S2 / n) of the statistic's own sums (about K).
    The bounds (derived in tests/test_fieldstats_cpu.py): |mean - ref| <= 1e-12 max|x|; |var - ref|, |cov - ref| <= 1e-12 max(S2 / n)."""
    ref = two_pass(x)
    e_mean = float(np.abs(np.asarray(got["mean"], dtype=f64) - ref["mean"]).max())
    e_var = float(np.abs(np.asarray(got["var"], dtype=f64) - ref["var"]).max())
    e_cov = float(np.abs(np.asarray(got["cov_uv"], dtype=f64) - ref["cov_uv"]).max())
    b_mean, b_var = REL * float(np.abs(x).max()), REL * s2n
    print(f"{what}: mean err {e_mean:.2e} (bound {b_mean:.2e}), var err {e_var:.2e}, cov err {e_cov:.2e} (bound {b_var:.2e})")
    assert e_mean <= b_mean and e_var <= b_var and e_cov <= b_var, (what, e_mean, e_var, e_cov)
    assert (np.asarray(got["min"]) == x.min(axis=0)).all() and (np.asarray(got["max"]) == x.max(axis=0)).all()
