"""The adaptive time step (gfv/timescheme.py `StepControl`) restated in numpy for the tests: the Courant rate of a
field, the controller, the step ratio, the variable-step BDF2 baseline and step, and the time.

Everything takes a `dtype`: float64 (the default) is the statement the kernels are compared against within a tolerance; float32
evaluates the same expressions with one rounding per operation in the order written here - the order include/gfv.h writes down -
and is what a host applies where a test asks for a host-driven loop that a device-decided one must equal bit for bit.  The time is
a float64 sum in either.

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import numpy as np

f64 = np.float64
BDF1, BDF2 = 1, 2


def cell_rates(x, uvp_dim, crow, knode, kS, area, cbatch, dtype=f64):
    """Per cell j of graph b = cbatch[j], over its incidences k: u_j = the mean of x[knode[k], 0:2] / uvp_dim[b, 0:2];
    rate_j = sum_k |u_j . kS[k]| / (2 area[j]).  Sums ascending in k from 0.  -> [C]"""
    x, dim = np.asarray(x).astype(dtype), np.asarray(uvp_dim).astype(dtype).reshape(-1, 3)
    kS, area = np.asarray(kS).astype(dtype).reshape(-1, 2), np.asarray(area).astype(dtype).reshape(-1)
    crow, knode, cbatch = np.asarray(crow, np.int64), np.asarray(knode, np.int64), np.asarray(cbatch, np.int64)
    n = crow[1:] - crow[:-1]
    C = n.shape[0]
    du, dv = dim[cbatch, 0], dim[cbatch, 1]
    sx, sy = np.zeros(C, dtype), np.zeros(C, dtype)
    for q in range(int(n.max())):
        m = q < n
        node = knode[crow[:-1][m] + q]
        sx[m] = sx[m] + x[node, 0] / du[m]
        sy[m] = sy[m] + x[node, 1] / dv[m]
    cnt = np.maximum(n, 1).astype(dtype)
    mx, my = sx / cnt, sy / cnt
    acc = np.zeros(C, dtype)
    for q in range(int(n.max())):
        m = q < n
        k = crow[:-1][m] + q
        acc[m] = acc[m] + np.abs(mx[m] * kS[k, 0] + my[m] * kS[k, 1])
    rate = acc / (dtype(2.0) * area)
    return np.where((n > 0) & (rate > 0), rate, dtype(0.0)).astype(dtype)


def graph_rates(rates, cbatch, B):
    """rate[b] = the maximum over the cells of graph b.  -> ([B] maxima, [B] runners-up: the largest value below, 0 if none)"""
    cbatch = np.asarray(cbatch, np.int64)
    top, second = np.zeros(B, rates.dtype), np.zeros(B, rates.dtype)
    for b in range(B):
        r = np.sort(rates[cbatch == b])
        top[b] = r[-1]
        second[b] = r[-2] if r.shape[0] > 1 else 0.0
    return top, second


def controller(rate, dt_last, dt_plan, ctl, dtype=f64):
    """ctl: anything with courant, grow, shrink, min_factor, max_factor.  -> (Co, dt_next, omega), each [B]"""
    t = lambda v: np.asarray(v).astype(dtype)
    rate, dt_last, dt_plan = t(rate), t(dt_last), t(dt_plan)
    courant, grow, shrink = dtype(ctl.courant), dtype(ctl.grow), dtype(ctl.shrink)
    co = (rate * dt_last).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where(co > 0, courant / np.where(co > 0, co, dtype(1.0)), grow).astype(dtype)
    fac = np.minimum(np.maximum(fac, shrink), grow)
    dt_next = (dt_last * fac).astype(dtype)
    dt_next = np.minimum(np.maximum(dt_next, dtype(ctl.min_factor) * dt_plan), dtype(ctl.max_factor) * dt_plan).astype(dtype)
    omega = (dt_next / dt_last).astype(dtype)
    return co, dt_next, omega


def bdf2_divisors(omega, dtype=f64):
    """(q, h): ustar = u_n + (u_n - u_{n-1}) / q and dt_eff = dt_next / h - the weights omega^2 / (1 + 2 omega) and
    (1 + omega) / (1 + 2 omega) as divisions by their reciprocals q = (1 + 2 omega) / omega^2, h = (1 + 2 omega) / (1 + omega): at
    omega = 1 they are exactly 3 and 1.5, today's (u_n - u_{n-1}) / 3 and dt / 1.5."""
    w = np.asarray(omega).astype(dtype)
    one, two = dtype(1.0), dtype(2.0)
    num = one + two * w
    return (num / (w * w)).astype(dtype), (num / (one + w)).astype(dtype)


class StepRule:
    """The pair of launches in numpy: `launch(x_backup, clock)` with the host's side (`reset`, `install_previous`) in front."""

    def __init__(self, plan, ctl, scheme=BDF2, dtype=f64):
        """plan: a dict of numpy arrays batch, uvp_dim, dt, crow, knode, kS, area, cbatch."""
        self.p, self.ctl, self.scheme, self.dtype = plan, ctl, scheme, dtype
        self.batch = np.asarray(plan["batch"], np.int64)
        self.dt_plan = np.asarray(plan["dt"]).astype(dtype).reshape(-1)
        self.dim = np.asarray(plan["uvp_dim"]).astype(dtype).reshape(-1, 3)
        N, self.B = self.batch.shape[0], self.dt_plan.shape[0]
        self.ring = np.zeros((2, N, 2), dtype)
        self.dts = np.zeros((2, self.B), dtype)
        self.times = np.zeros((2, self.B), f64)
        self.base = self.tbase = 0
        self.dt0, self.time0 = self.dt_plan.copy(), np.zeros(self.B, f64)
        self.history = {}

    def _start(self, clock, dt_last, time):
        self.tbase = clock
        self.dt0 = self.dt_plan.copy() if dt_last is None else np.asarray(dt_last).astype(self.dtype)
        self.time0 = np.zeros(self.B, f64) if time is None else np.asarray(time, f64).copy()
        self.history = {}

    def reset(self, clock, dt_last=None, time=None):
        self._start(clock, dt_last, time)
        self.base = clock

    def install_previous(self, previous, clock, dt_last=None, time=None):
        self._start(clock, dt_last, time)
        self.ring[(clock & 1) ^ 1] = np.asarray(previous).astype(self.dtype)[:, 0:2]
        self.base = clock - 1

    def launch(self, x_backup, clock):
        """-> a dict of everything the pair writes for this clock (and `active`, `rates` [C], `dt_last`)."""
        d, p, c = self.dtype, self.p, int(clock)
        x = np.asarray(x_backup).astype(d)
        rates = cell_rates(x, p["uvp_dim"], p["crow"], p["knode"], p["kS"], p["area"], p["cbatch"], d)
        rate, _ = graph_rates(rates, p["cbatch"], self.B)
        first = c <= self.tbase
        dt_last = self.dt0.copy() if first else self.dts[c & 1].copy()
        co, dt_next, omega = controller(rate, dt_last, self.dt_plan, self.ctl, d)
        active = self.scheme == BDF2 and c > self.base
        cur = x[:, 0:2]
        dimn = self.dim[self.batch][:, 0:2]
        if active:
            q, h = bdf2_divisors(omega, d)
            prev = self.ring[(c & 1) ^ 1]
            ustar = ((cur + (cur - prev) / q[self.batch][:, None]) / dimn).astype(d)
            dt_eff = (dt_next / h).astype(d)
        else:
            ustar, dt_eff = (cur / dimn).astype(d), dt_next.copy()
        time = self.time0.copy() if first else self.times[(c & 1) ^ 1] + dt_last.astype(f64)
        self.ring[c & 1] = cur
        self.dts[(c + 1) & 1] = dt_next
        self.times[c & 1] = time
        self.history[c] = {"clock": c, "dt": dt_next.copy(), "courant": co.copy(), "time": time.copy()}
        return {"active": bool(active), "rates": rates, "rate": rate, "dt_last": dt_last, "courant": co, "dt": dt_next,
                "omega": omega, "ustar": ustar, "dt_eff": dt_eff, "time": time}


def plan_arrays(plan):
    """The arrays `StepRule` reads, from a gfv plan (device tensors) as numpy."""
    return {k: getattr(plan, k).detach().cpu().numpy() for k in ("batch", "uvp_dim", "dt", "crow", "knode", "kS", "area", "cbatch")}
