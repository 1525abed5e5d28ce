"""Probes (include/gfv.h gfv_probe_sample; gfv/probes.py) restated in float64 numpy.

Written from the header's paragraph, not from the kernel or from gfv/probes.py: the location by brute force over the cells of a
graph, the value and the gradient at a point through the vertices' WLSQ gradients (`wallforce_ref.gradients`: np.linalg.solve with
the right-hand side, no weights), and the launch itself on given weight tables (math.fsum of the products) with the record and
the ring.  The fp32 step the header names (the division by uvp_dim) is fp32 here too; everything else is float64.  Nothing here
touches a GPU.
"""
import math

import numpy as np

import wallforce_ref as W
from window_ref import COUNTER, ENABLED, LAST, N, RECORD, START, STOP, STRIDE, commit, take  # noqa: F401  (the window: once)

SUMS = 9
U = 2.0 ** -53
U32 = 2.0 ** -24

f32, f64 = np.float32, np.float64
_np = W._np


# ---- the mesh as arrays ------------------------------------------------------------------------------------------------------------
def mesh_arrays(graphs, plan):
    """wallforce_ref's arrays and what the location reads: the cells' incidence rows, their vertices, areas and graph ranges."""
    m = W.mesh_arrays(graphs, plan)
    m.update({"C": int(plan.C), "crow": _np(plan.crow).astype(np.int64), "knode": _np(plan.knode).astype(np.int64),
              "gcell_ptr": _np(plan.gcell_ptr).astype(np.int64), "area": _np(plan.area).astype(f32)})
    return m


# ---- location, by brute force ------------------------------------------------------------------------------------------------------
def cell_distance(m, C, x):
    """d(C) of the header: the largest of ((x - fpos[kface[k]]) . kS[k]) / |kS[k]| over the cell's incidences, in double."""
    k0, k1 = m["crow"][C], m["crow"][C + 1]
    S = m["kS"][k0:k1].astype(f64)
    fc = m["fpos"][m["kface"][k0:k1]].astype(f64)
    d = ((x[0] - fc[:, 0]) * S[:, 0] + (x[1] - fc[:, 1]) * S[:, 1]) / np.sqrt(S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1])
    return float(d.max())


def distances(m, x, b):
    """d of every cell of graph b -> (first cell of the graph, d [cells of b])."""
    c0, c1 = int(m["gcell_ptr"][b]), int(m["gcell_ptr"][b + 1])
    k0, k1 = int(m["crow"][c0]), int(m["crow"][c1])
    S = m["kS"][k0:k1].astype(f64)
    fc = m["fpos"][m["kface"][k0:k1]].astype(f64)
    dk = ((x[0] - fc[:, 0]) * S[:, 0] + (x[1] - fc[:, 1]) * S[:, 1]) / np.sqrt(S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1])
    return c0, np.maximum.reduceat(dk, m["crow"][c0:c1] - k0)                  # (every cell has an incidence: no empty segment)


def locate(m, x, b):
    """-> (cell, outside, how many cells of the graph have d <= 0): the cell of least d, the lowest index among equals."""
    c0, d = distances(m, np.asarray(x, dtype=f64), b)
    best = 0
    for j in range(1, len(d)):
        if d[j] < d[best]:
            best = j
    cell = c0 + best
    return cell, float(d[best]) / math.sqrt(float(m["area"][cell])), int((d <= 0).sum())


def vertices(m, cell):
    return m["knode"][m["crow"][cell]:m["crow"][cell + 1]]


# ---- the value and the gradient at a point -----------------------------------------------------------------------------------------
def value_gradient(m, cell, x, field):
    """-> (value [3], gradient [3, 2]) of the header's two formulas: the mean over the cell's k vertices of phi_c(v) + g_v[c] . (x -
    pos[v]) and of g_v[c], g_v by np.linalg.solve on the row-normalised system."""
    V = vertices(m, cell)
    assert len(set(V.tolist())) == len(V)
    phi = W.node_values(m, field).astype(f64)
    g = W.gradients(m, V, field)                                               # [k, 3, 2]
    off = np.asarray(x, dtype=f64) - m["pos"][V].astype(f64)                   # [k, 2]
    val = phi[V] + (g * off[:, None, :]).sum(2)                                # [k, 3]
    return val.mean(0), g.mean(0)


def grad_bound(m, nodes, field):
    """Per (node, channel): 64 * kappa * 2^-53 * || sum_s |B_s| |dphi_s| / rn ||_2, kappa the largest cond_2(A / rn) of `nodes` - how
    far two backward-stable double solutions of one vertex system may lie apart (the form and the derivation of
    tests/test_wallforce_gpu.py `_grad_bound`: a transposed solve against the stencil's rows is as stable as a solve with the
    right-hand side).  -> [len(nodes), 3]"""
    q, cond = W.gradient_bounds(m, nodes, field)
    return 64.0 * float(cond.max()) * U * q


def combined_bound(m, cell, x, field, nnz, mag):
    """Per entry q = 3 c + j [9]: how far `weights @ phi` (or the device's row) may lie from value_gradient(): the bound of the
    gradients times (1 + |x - pos[v]|_1), averaged over the vertices, plus the sum bound (nnz + 16) 2^-53 sum |w| |phi| (`mag` [9]:
    a sum of nnz products each rounded once, in any order, and the merge of the weights, each rounded a few times)."""
    V = vertices(m, cell)
    gb = grad_bound(m, V, field)                                               # [k, 3]
    off = np.abs(np.asarray(x, dtype=f64) - m["pos"][V].astype(f64)).sum(1)    # [k]
    per = (gb * (1.0 + off)[:, None]).mean(0)                                  # [3]
    return np.repeat(per, 3) + (nnz + 16.0) * U * np.asarray(mag, dtype=f64)


# ---- the launch on given tables ----------------------------------------------------------------------------------------------------
def dot_rows(pw_ptr, pw_node, pw_w, phi, dtype=f64):
    """-> (rows [P, 9], magnitudes [P, 9]): per probe and q = 3 c + j the sum over its entries of pw_w[e, j] * phi[pw_node[e], c]
    (math.fsum: correctly rounded) and of the products' absolute values.  dtype float32: the variant that multiplies and
    accumulates in fp32, entry after entry."""
    P = len(pw_ptr) - 1
    rows, mag = np.zeros((P, SUMS), dtype=f64), np.zeros((P, SUMS), dtype=f64)
    for p in range(P):
        e0, e1 = int(pw_ptr[p]), int(pw_ptr[p + 1])
        w = np.asarray(pw_w[e0:e1], dtype=f64)                                 # [n, 3]
        v = np.asarray(phi, dtype=f64)[np.asarray(pw_node[e0:e1], dtype=np.int64)]     # [n, 3]
        for c in range(3):
            for j in range(3):
                prod = w[:, j] * v[:, c]
                if dtype is f64:
                    rows[p, 3 * c + j] = math.fsum(prod)
                else:
                    acc = f32(0.0)
                    for a, b in zip(w[:, j].astype(f32), v[:, c].astype(f32)):
                        acc = f32(acc + f32(a * b))
                    rows[p, 3 * c + j] = float(acc)
                mag[p, 3 * c + j] = math.fsum(np.abs(prod))
    return rows, mag


class ProbesRef:
    """The record and the ring a sequence of launches works on, and `launch()`: one launch applied to them."""

    def __init__(self, pw_ptr, pw_node, pw_w, uvp_dim, batch, keep, start=1, stride=1, stop=-1, enabled=1):
        self.ptr, self.node, self.w = np.asarray(pw_ptr), np.asarray(pw_node), np.asarray(pw_w, dtype=f64)
        self.dim, self.batch = np.asarray(uvp_dim, dtype=f32).reshape(-1, 3), np.asarray(batch, dtype=np.int64)
        self.P, self.keep = len(self.ptr) - 1, int(keep)
        self.rec = np.zeros(RECORD, dtype=np.int32)
        self.rec[[START, STRIDE, STOP, ENABLED]] = (start, stride, stop, enabled)
        self.rec[LAST] = -1
        self.hist = np.zeros((self.keep, self.P, SUMS), dtype=f64)
        self.hist_clock = np.zeros(self.keep, dtype=np.int32)
        self.mag = np.zeros((self.keep, self.P, SUMS), dtype=f64)

    def reset(self):
        self.rec[LAST], self.rec[N] = -1, 0

    def phi(self, field):
        return (np.asarray(field, dtype=f32)[:, 0:3] / self.dim[self.batch]).astype(f32)       # ONE fp32 division

    def launch(self, field, clock):
        c = int(clock)
        taken = take(self.rec, c)
        if taken:
            row = int(self.rec[N]) % self.keep
            self.hist[row], self.mag[row] = dot_rows(self.ptr, self.node, self.w, self.phi(field))
            self.hist_clock[row] = c
        commit(self.rec, c, taken)
        return taken

    def rows(self):
        """The last min(n, keep) rows in clock order: (clock [k], hist [k, P, 9], magnitudes [k, P, 9])."""
        n = int(self.rec[N])
        k = min(n, self.keep)
        order = [(n - k + q) % self.keep for q in range(k)]
        return self.hist_clock[order].copy(), self.hist[order].copy(), self.mag[order].copy()
