"""The flow integrals (include/gfv.h gfv_flow_integrals; gfv/integrals.py) restated in float64 numpy.

Written from the header's paragraph, not from the kernel or from gfv/integrals.py: the boundary kind of every incidence by brute
force, the cell chunks, the per-cell closed-polygon sums and the twelve columns per graph (sums by math.fsum, maxima by max), and
the launch with its record and ring.  The fp32 step the header names (the division by uvp_dim) is fp32 here too; everything else
is float64 - so what separates the kernel from this file is the kernel's own double rounding, which the tests bound.  Nothing here
touches a GPU.
"""
import math

import numpy as np

import probes_ref as P
from window_ref import COUNTER, ENABLED, LAST, N, RECORD, START, STOP, STRIDE, commit, take  # noqa: F401  (the window: once)

SUMS, MAXS, CHUNK = 10, 2, 64
COLS = SUMS + MAXS
INFLOW, OUTFLOW = 1, 2
U = 2.0 ** -53
U32 = 2.0 ** -24

f32, f64 = np.float32, np.float64


def mesh_arrays(graphs, plan):
    """probes_ref's arrays (the incidence rows, vertices, areas, graph ranges, face ends, face types) and the boundary kinds."""
    m = P.mesh_arrays(graphs, plan)
    m["btype"] = btype(m["kface"], m["face_type"])
    return m


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def btype(kface, face_type):
    """Per incidence: 0 where its face has two incidences; where it has exactly one, 1 (INFLOW), 2 (OUTFLOW) or 3 (anything else).
    By brute force: one count per face."""
    kface = np.asarray(kface, dtype=np.int64)
    out = np.zeros(len(kface), dtype=np.int32)
    for k, f in enumerate(kface):
        if int((kface == f).sum()) == 1:
            t = int(face_type[f])
            out[k] = 1 if t == INFLOW else 2 if t == OUTFLOW else 3
    return out


def chunks(gcell_ptr):
    """-> (cchunk_beg, cchunk_end, gcchunk_ptr): at most CHUNK consecutive cells, never across a graph."""
    beg, end, ptr = [], [], [0]
    for b in range(len(gcell_ptr) - 1):
        c = int(gcell_ptr[b])
        while c < int(gcell_ptr[b + 1]):
            beg.append(c)
            c = min(c + CHUNK, int(gcell_ptr[b + 1]))
            end.append(c)
        ptr.append(len(beg))
    return np.array(beg, dtype=np.int32), np.array(end, dtype=np.int32), np.array(ptr, dtype=np.int32)


# ---- the per-cell terms ------------------------------------------------------------------------------------------------------------
def node_values(m, field):
    """phi [N, 3]: field[:, c] / uvp_dim[batch, c], ONE fp32 division."""
    x = np.asarray(field, dtype=f32)[:, 0:3]
    return (x / np.asarray(m["uvp_dim"], dtype=f32).reshape(-1, 3)[m["batch"]]).astype(f32)


def _cells(m, phi, sign, dtype):
    """The twelve per-cell terms [C, 12] and (Gamma / a, D / a) [C, 2] of node values `phi`, every operation in `dtype`; sign +1.0
    with absolute operands gives the magnitudes."""
    crow = np.asarray(m["crow"], dtype=np.int64)
    n = np.diff(crow)
    assert (n >= 1).all()
    first = crow[:-1]
    kface = np.asarray(m["kface"], dtype=np.int64)
    s, r, v = np.asarray(m["es"])[kface], np.asarray(m["er"])[kface], np.asarray(m["knode"], dtype=np.int64)
    S = np.asarray(m["kS"]).astype(dtype)
    phi = np.asarray(phi).astype(dtype)
    half = dtype(0.5)
    uf, vf = half * (phi[s, 0] + phi[r, 0]), half * (phi[s, 1] + phi[r, 1])
    d = uf * S[:, 0] + vf * S[:, 1]
    g = vf * S[:, 0] + dtype(sign) * (uf * S[:, 1])
    seg = lambda x: np.add.reduceat(x, first).astype(dtype)
    D, G = seg(d), seg(g)
    nn = n.astype(dtype)
    ubar, vbar, pbar = seg(phi[v, 0]) / nn, seg(phi[v, 1]) / nn, seg(phi[v, 2]) / nn
    a = np.asarray(m["area"]).astype(dtype)
    bt = np.asarray(m["btype"])
    zero = dtype(0.0)
    out = np.zeros((len(n), COLS), dtype=dtype)
    out[:, 0] = a
    out[:, 1] = (half * (ubar * ubar + vbar * vbar)) * a
    out[:, 2] = (half * (G * G)) / a
    out[:, 3] = (D * D) / a
    out[:, 4] = D
    out[:, 5] = G
    out[:, 6] = pbar * a
    for j in (1, 2, 3):
        out[:, 6 + j] = seg(np.where(bt == j, d, zero))
    out[:, 10] = np.abs(D) / a
    out[:, 11] = np.abs(G) / a
    return out, np.stack((G / a, D / a), 1)


def cell_terms(m, phi, dtype=f64):
    """-> (terms [C, 12], magnitudes [C, 12], cell_out [C, 2]): the per-cell terms of the header, the same expressions with every
    product and addend replaced by its absolute value, and (Gamma_C / a, D_C / a)."""
    t, out = _cells(m, phi, -1.0, dtype)
    mag, _ = _cells(dict(m, kS=np.abs(np.asarray(m["kS"])), area=np.abs(np.asarray(m["area"]))), np.abs(np.asarray(phi)), 1.0, f64)
    return t, mag, out


def graph_rows(m, phi, dtype=f64):
    """-> (rows [B, 12], magnitudes [B, 12], cell_out [C, 2]): per graph the sums of columns 0 .. 9 (float64: math.fsum, correctly
    rounded; float32: accumulated in fp32) and the maxima of columns 10, 11 from +0.0; of the magnitudes the sums and the LARGEST."""
    t, mag, out = cell_terms(m, phi, dtype)
    B = len(m["gcell_ptr"]) - 1
    rows, amag = np.zeros((B, COLS), dtype=f64), np.zeros((B, COLS), dtype=f64)
    for b in range(B):
        c0, c1 = int(m["gcell_ptr"][b]), int(m["gcell_ptr"][b + 1])
        for q in range(SUMS):
            rows[b, q] = math.fsum(t[c0:c1, q]) if dtype is f64 else float(t[c0:c1, q].sum(dtype=f32))
            amag[b, q] = math.fsum(mag[c0:c1, q])
        for q in range(SUMS, COLS):
            rows[b, q] = float(np.fmax.reduce(t[c0:c1, q], initial=0.0)) if c1 > c0 else 0.0
            amag[b, q] = float(mag[c0:c1, q].max()) if c1 > c0 else 0.0
    return rows, amag, out.astype(f64)


def k_max(m):
    return int(np.diff(np.asarray(m["crow"])).max())


def bound(m, mag):
    """How far a device row [B, 12] may lie from graph_rows(): a term costs at most (2 k_max + 8) roundings (a k-term sum of
    three-operation addends, squared, scaled), the sum over a graph's Nc_b cells in any order at most Nc_b + 16, so
    (Nc_b + 2 k_max + 24) 2^-53 sum_C mag_C for the ten sums, and (2 k_max + 8) 2^-53 of the largest magnitude for the two maxima."""
    cells = np.diff(np.asarray(m["gcell_ptr"])).astype(f64)[:, None]
    k = float(k_max(m))
    out = (cells + 2.0 * k + 24.0) * U * np.asarray(mag, dtype=f64)
    out[:, SUMS:] = (2.0 * k + 8.0) * U * np.asarray(mag, dtype=f64)[:, SUMS:]
    return out


def cell_bound(m, mag):
    """The bound of one cell's (Gamma / a, D / a) [C, 2]: (2 k_max + 8) 2^-53 of that cell's magnitude."""
    return (2.0 * k_max(m) + 8.0) * U * np.asarray(mag, dtype=f64)[:, [11, 10]]


# ---- the record and the ring ---------------------------------------------------------------------------------------------------------
class FlowRef:
    """The record, the ring and the cell fields a sequence of launches works on, and `launch()`: one launch applied to them."""

    def __init__(self, m, keep, start=1, stride=1, stop=-1, enabled=1):
        self.m, self.keep = m, int(keep)
        self.B, self.C = len(m["gcell_ptr"]) - 1, len(m["crow"]) - 1
        self.rec = np.zeros(RECORD, dtype=np.int32)
        self.rec[[START, STRIDE, STOP, ENABLED]] = (start, stride, stop, enabled)
        self.rec[LAST] = -1
        self.hist = np.zeros((self.keep, self.B, COLS), dtype=f64)
        self.hist_clock = np.zeros(self.keep, dtype=np.int32)
        self.mag = np.zeros((self.keep, self.B, COLS), dtype=f64)
        self.cell_out = np.zeros((self.C, 2), dtype=f64)
        self.cell_mag = np.zeros((self.C, COLS), dtype=f64)

    def reset(self):
        self.rec[LAST], self.rec[N] = -1, 0

    def launch(self, field, clock):
        c = int(clock)
        taken = take(self.rec, c)
        if taken:
            row = int(self.rec[N]) % self.keep
            phi = node_values(self.m, field)
            self.hist[row], self.mag[row], self.cell_out = graph_rows(self.m, phi)
            self.cell_mag = cell_terms(self.m, phi)[1]
            self.hist_clock[row] = c
        commit(self.rec, c, taken)
        return taken

    def rows(self):
        """The last min(n, keep) rows in clock order: (clock [k], hist [k, B, 12], magnitudes [k, B, 12])."""
        n = int(self.rec[N])
        k = min(n, self.keep)
        order = [(n - k + q) % self.keep for q in range(k)]
        return self.hist_clock[order].copy(), self.hist[order].copy(), self.mag[order].copy()
