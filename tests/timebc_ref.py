"""Unsteady boundary data in plain numpy float64 (gfv/timebc.py, csrc/timebc.hip; include/gfv.h gfv_time_bc_update): the four
waveforms, one launch (mask, products, history row) and the clock rule, each operation one IEEE double operation in the order the
header writes it - so everything but `sin` is reproducible to the bit."""
import numpy as np

f32, f64 = np.float32, np.float64
NODE_TYPES = {"inflow": 1, "wall": 3, "in_wall": 5}
TWO_PI = f64(6.283185307179586)
assert TWO_PI == f64(2.0) * f64(np.pi)


def const(value):
    return ("const", f64(value))


def ramp(g0, g1, t0, t1, shape="linear"):
    return ("ramp", f64(g0), f64(g1), f64(t0), f64(t1), shape)


def sine(mean, amp, freq, phase=0.0, start=0.0):
    return ("sine", f64(mean), f64(amp), f64(freq), f64(phase), f64(start))


def table(times, values, periodic=False):
    return ("table", np.asarray(times, dtype=f64), np.asarray(values, dtype=f64), bool(periodic))


def wave(w, t):
    """g(t) of one waveform at one float64 time."""
    t = f64(t)
    kind = w[0]
    if kind == "const":
        return w[1]
    if kind == "ramp":
        _, g0, g1, t0, t1, shape = w
        s = (t - t0) / (t1 - t0)
        s = min(max(s, f64(0.0)), f64(1.0))
        if shape == "smooth":
            s2 = s * s
            s = s2 * (f64(3.0) - f64(2.0) * s)
        return g0 + (g1 - g0) * s
    if kind == "sine":
        _, mean, amp, freq, phase, start = w
        tau = max(t - start, f64(0.0))
        arg = (TWO_PI * freq) * tau + phase
        return mean + amp * np.sin(arg)
    if kind == "table":
        _, T, V, periodic = w
        n = len(T)
        if periodic and n >= 2:
            span = T[-1] - T[0]
            m = np.fmod(t - T[0], span)
            if m < 0:
                m = m + span
            t = T[0] + m
        if t <= T[0]:
            return V[0]
        if t >= T[-1]:
            return V[-1]
        k = int(np.searchsorted(T, t, side="right")) - 1          # T[k] <= t < T[k + 1]
        f = (t - T[k]) / (T[k + 1] - T[k])
        return V[k] + (V[k + 1] - V[k]) * f
    raise ValueError(kind)


def sine_argument(w, t):
    """The argument of `sin` for a sine waveform (what the accuracy of the device's `sin` is measured at)."""
    _, mean, amp, freq, phase, start = w
    return (TWO_PI * freq) * max(f64(t) - start, f64(0.0)) + phase


def type_mask(nodes):
    return sum(1 << NODE_TYPES[n] for n in nodes)


def launch(clock, dt, batch, node_type, y0, theta0, velocity, source, nodes, y, theta5=None, col8=None, hist=None):
    """One launch for field `clock` (the owner's counter + 1 + the offset), in place on y [N, 2] f32, theta5 [B] f32, col8 [N] f32
    and hist [K, B, 3] f64.  velocity / source: one waveform per graph, or None (the channel is off: nothing of it is written)."""
    B = len(dt)
    c = f64(int(clock))
    t = np.array([c * f64(dt[b]) for b in range(B)], dtype=f64)
    gv = np.array([wave(velocity[b], t[b]) if velocity is not None else 1.0 for b in range(B)], dtype=f64)
    gs = np.array([wave(source[b], t[b]) if source is not None else 1.0 for b in range(B)], dtype=f64)
    if velocity is not None:
        m = ((type_mask(nodes) >> np.clip(node_type, 0, 31)) & 1).astype(bool) & (node_type >= 0) & (node_type < 32)
        y[m] = (gv[batch[m]][:, None] * y0[m].astype(f64)).astype(f32)
    if source is not None:
        v = (gs * theta0.astype(f64)).astype(f32)
        if theta5 is not None:
            theta5[:] = v
        if col8 is not None:
            col8[:] = v[batch]
    if hist is not None and 1 <= clock <= hist.shape[0]:
        hist[clock - 1, :, 0], hist[clock - 1, :, 1], hist[clock - 1, :, 2] = t, gv, gs
    return t, gv, gs


def rows(clocks, dt, velocity, source):
    """The history rows (t, g_v, g_s) [k, B] for a list of clocks."""
    B = len(dt)
    t = np.array([[f64(int(c)) * f64(dt[b]) for b in range(B)] for c in clocks], dtype=f64)
    gv = np.array([[wave(velocity[b], t[k, b]) if velocity is not None else 1.0 for b in range(B)] for k in range(len(clocks))], dtype=f64)
    gs = np.array([[wave(source[b], t[k, b]) if source is not None else 1.0 for b in range(B)] for k in range(len(clocks))], dtype=f64)
    return t.reshape(len(clocks), B), gv.reshape(len(clocks), B), gs.reshape(len(clocks), B)


def next_clock(counter, offset=0):
    """The clock rule: the launch behind the advance that moved the owner's counter to `counter` writes the data of field
    counter + 1 (+ the offset of a resumed run); attach() and reset() find counter = 0 and write field 1."""
    return int(counter) + 1 + int(offset)


def from_object(w):
    """A gfv.timebc waveform object -> this module's tuple."""
    name = type(w).__name__
    if name == "Const":
        return const(w.value)
    if name == "Ramp":
        return ramp(w.g0, w.g1, w.t0, w.t1, w.shape)
    if name == "Sine":
        return sine(w.mean, w.amp, w.freq, w.phase, w.start)
    if name == "Table":
        return table(w.times, w.values, w.periodic)
    raise ValueError(name)
