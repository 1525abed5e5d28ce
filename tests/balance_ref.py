"""The loss-balancing rule of include/gfv.h (gfv_loss_balance) restated in plain Python: float64 arithmetic, one IEEE operation per
Python operation, in the order the header writes them.  What the GPU tests compare csrc/balance.hip with and what the CPU tests
check the rule's properties on.  Only math.exp may differ from the device's exp in its last bits."""
import math
import struct

INVERSE, PROGRESS = 1, 2
LANES = 64


def f32(x):
    """float32(x) as a Python float (round to nearest even; beyond the fp32 range: inf, like a C cast)."""
    try:
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def statistic(losses):
    """s[3] of `losses` (rows of four numbers, taken as fp32 values): the header's fixed order - 64 strided partial sums, added
    from the left, folded by halves."""
    B = len(losses)
    out = []
    for k in range(3):
        p = [0.0] * LANES
        for b in range(B):
            r = [f32(v) for v in losses[b]]
            t = (r[0], r[1] + r[2], r[3])[k]
            p[b % LANES] = p[b % LANES] + t
        h = LANES // 2
        while h >= 1:
            for j in range(h):
                p[j] = p[j] + p[j + h]
            h //= 2
        out.append(p[0] / float(B))
    return out


class Balance:
    """The record of one balancer and `observe`, the launch.  Attribute names are the header's."""

    def __init__(self, kind, w0, g=(1.0, 1.0, 1.0), decay=0.9, warmup=10, every=1, floor=1e-30, alpha=0.9, tau=1.0):
        self.kind, self.decay, self.warmup, self.every, self.floor = kind, float(decay), int(warmup), int(every), float(floor)
        self.alpha, self.tau = float(alpha), float(tau)
        self.g, self.w0 = [float(v) for v in g], [float(v) for v in w0]
        self.n = self.n_applied = self.n_updates = self.n_skipped = 0
        self.power = 1.0
        self.m, self.s, self.s_ref = [0.0] * 3, [0.0] * 3, [0.0] * 3
        self.lam, self.w = [1.0] * 3, list(self.w0)
        self.mh = [0.0] * 3            # (not a word of the record: the bias-corrected average of the last observation)

    def observe(self, losses, hold=None, hyper=None):
        """One launch.  hold: None (no hold word) or the word's value.  hyper: a list of 8 numbers; words 5 .. 7 are written on a
        publish.  -> True on a publish."""
        s = statistic(losses)
        if any(math.isnan(v) or math.isinf(v) or v < 0.0 for v in s):
            self.n_skipped += 1
            return False
        self.n += 1
        self.power = self.power * self.decay
        for k in range(3):
            self.m[k] = self.decay * self.m[k] + (1.0 - self.decay) * s[k]
            self.mh[k] = self.m[k] / (1.0 - self.power)
        self.s = s
        if self.n == 1:
            self.s_ref = list(self.mh)
        applied = hold is None or hold != 0
        if applied:
            self.n_applied += 1
        every = max(self.every, 1)
        if not (applied and self.n > self.warmup and self.n_applied % every == 0):
            return False
        mh, w0 = self.mh, self.w0
        if self.kind == PROGRESS:
            z = [(mh[k] / max(self.s_ref[k], self.floor)) / self.tau for k in range(3)]
            zm = max(max(z[0], z[1]), z[2])
            e = [math.exp(z[k] - zm) for k in range(3)]
            E = (e[0] + e[1]) + e[2]
            for k in range(3):
                self.lam[k] = self.alpha * self.lam[k] + (1.0 - self.alpha) * (3.0 * (e[k] / E))
                self.w[k] = w0[k] * self.lam[k]
            self.s_ref = list(mh)
        else:
            self.R0 = (w0[0] * mh[0] + w0[1] * mh[1]) + w0[2] * mh[2]
            G = (self.g[0] + self.g[1]) + self.g[2]
            for k in range(3):
                self.w[k] = ((self.g[k] / G) * self.R0) / max(mh[k], self.floor)
        self.n_updates += 1
        if hyper is not None:
            for k in range(3):
                hyper[5 + k] = f32(self.w[k])
        return True

    def words(self):
        return dict(n=self.n, n_applied=self.n_applied, n_updates=self.n_updates, n_skipped=self.n_skipped)

    def doubles(self):
        return dict(power=[self.power], m=list(self.m), s=list(self.s), s_ref=list(self.s_ref), lam=list(self.lam), w=list(self.w))
