"""The wall-force launches (include/gfv.h gfv_wall_force_grad, gfv_wall_force_sum; gfv/wallforce.py) restated in float64 numpy.

Written from the header's paragraph, not from the kernels: the selection of the faces, the launch tables, the body nodes' WLSQ
gradients (np.linalg.solve on the row-normalised system), the six sums per graph, and the record with its ring.  The fp32 steps
the header names (the division by uvp_dim, the face-to-node offsets) are fp32 here too; everything else is float64, summed by
math.fsum - so what separates a kernel from this file is the kernel's own double rounding, which the tests bound.  Nothing here
touches a GPU.
"""
import math

import numpy as np

from window_ref import COUNTER, ENABLED, LAST, N, RECORD, START, STOP, STRIDE, commit, take  # noqa: F401  (the window: once)

SUMS, CHUNK = 6, 64
WALL_BOUNDARY = 3

f32, f64 = np.float32, np.float64


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


# ---- the mesh as arrays ------------------------------------------------------------------------------------------------------------
def mesh_arrays(graphs, plan):
    """What the restatement reads, as numpy arrays: from the five graph objects (selection) and the plan (stencil, incidences)."""
    gn, ge, gi = graphs[0], graphs[2], graphs[4]
    return {
        "B": int(gi.theta_PDE.shape[0]), "N": int(plan.N), "E": int(plan.E), "M": int(plan.M),
        "face_type": _np(ge.face_type).reshape(-1).astype(np.int64), "cells_face": _np(ge.face).reshape(-1).astype(np.int64),
        "face_pos": _np(ge.pos).astype(f64), "edge_index": _np(gn.edge_index).astype(np.int64),
        "batch": _np(gn.batch).reshape(-1).astype(np.int64),
        "es": _np(plan.es).astype(np.int64), "er": _np(plan.er).astype(np.int64), "pos": _np(plan.pos).astype(f32),
        "fpos": _np(plan.fpos).astype(f32), "kface": _np(plan.kface).astype(np.int64), "kS": _np(plan.kS).astype(f32),
        "x_rowptr": _np(plan.x_rowptr).astype(np.int64), "x_out": _np(plan.x_out).astype(np.int64), "x_B": _np(plan.x_B).astype(f32),
        "An": _np(plan.An).astype(f32).reshape(int(plan.N), int(plan.M), int(plan.M)), "rn": _np(plan.rn).astype(f32),
        "theta": _np(plan.theta).astype(f32), "uvp_dim": _np(plan.uvp_dim).astype(f32).reshape(-1, 3),
    }


# ---- which faces --------------------------------------------------------------------------------------------------------------------
def incidences(m):
    return np.bincount(m["cells_face"], minlength=m["E"])


def select_faces(m, faces=None, box=None):
    """Ascending face indices: wall type, exactly one incidence, named by `faces` (bool mask or indices) if given, centre inside
    `box` (one (xmin, xmax, ymin, ymax) or a list of B) if given."""
    ok = (m["face_type"] == WALL_BOUNDARY) & (incidences(m) == 1)
    sel = ok.copy()
    if faces is not None:
        faces = np.asarray(faces)
        named = faces.astype(bool) if faces.dtype == bool else np.isin(np.arange(m["E"]), faces)
        if (named & ~ok).any():
            raise ValueError("a named face does not qualify")
        sel &= named
    if box is not None:
        boxes = np.asarray(box, dtype=f64)
        boxes = np.broadcast_to(boxes, (m["B"], 4)) if boxes.ndim == 1 else boxes
        bx = boxes[m["batch"][m["edge_index"][0]]]
        p = m["face_pos"]
        sel &= (p[:, 0] >= bx[:, 0]) & (p[:, 0] <= bx[:, 1]) & (p[:, 1] >= bx[:, 2]) & (p[:, 1] <= bx[:, 3])
    out = np.nonzero(sel)[0]
    if out.size == 0:
        raise ValueError("no face")
    return out


def build_tables(m, selected):
    """bnode [Nb], wface [Nf, 4] = (f, k, ja, jb), wchunk_beg / wchunk_end, gwchunk_ptr [B + 1], faces per graph [B]."""
    sel = np.asarray(selected, dtype=np.int64)
    k = np.array([np.nonzero(m["kface"] == f)[0] for f in sel])          # (exactly one incidence each: a [Nf, 1] array)
    assert k.shape == (sel.size, 1)
    s, r = m["es"][sel], m["er"][sel]
    bnode = np.unique(np.concatenate((s, r)))
    pos_of = {int(v): j for j, v in enumerate(bnode)}
    wface = np.stack((sel, k[:, 0], [pos_of[int(v)] for v in s], [pos_of[int(v)] for v in r]), 1).astype(np.int32)
    fb = m["batch"][s]
    assert (np.diff(fb) >= 0).all()
    counts = np.bincount(fb, minlength=m["B"])
    beg, end, ptr, row = [], [], [0], 0
    for b in range(m["B"]):
        for st in range(row, row + counts[b], CHUNK):
            beg.append(st)
            end.append(min(st + CHUNK, row + counts[b]))
        row += counts[b]
        ptr.append(len(beg))
    return {"bnode": bnode.astype(np.int32), "wface": wface, "wchunk_beg": np.array(beg, dtype=np.int32),
            "wchunk_end": np.array(end, dtype=np.int32), "gwchunk_ptr": np.array(ptr, dtype=np.int32), "faces": counts}


# ---- stage 1: the body nodes' gradients ------------------------------------------------------------------------------------------
def node_values(m, field):
    """phi [N, 3]: field[:, c] / uvp_dim[batch, c], ONE fp32 division."""
    x = np.asarray(field, dtype=f32)[:, 0:3]
    return (x / m["uvp_dim"][m["batch"]]).astype(f32)


def gradients(m, bnode, field, solve_dtype=f64):
    """gb [Nb, 3, 2] float64: the first two entries of the solution of (A / rn) g = (sum_s B_s (phi_out - phi_i)) / rn.  solve_dtype
    float32: the variant whose elimination runs in fp32 (the right-hand side and the matrix are formed in double, then rounded)."""
    phi = node_values(m, field).astype(f64)
    gb = np.zeros((len(bnode), 3, 2), dtype=f64)
    for j, i in enumerate(np.asarray(bnode, dtype=np.int64)):
        s0, s1 = m["x_rowptr"][i], m["x_rowptr"][i + 1]
        Bs = m["x_B"][s0:s1].astype(f64)                                  # [S, M]
        d = phi[m["x_out"][s0:s1]] - phi[i]                               # [S, 3]
        rn = m["rn"][i].astype(f64)
        rhs = (Bs.T @ d) / rn[:, None]                                    # [M, 3]
        A = m["An"][i].astype(f64) / rn[:, None]
        sol = np.linalg.solve(A.astype(solve_dtype), rhs.astype(solve_dtype)).astype(f64)
        gb[j] = sol[0:2].T
    return gb


def gradient_bounds(m, bnode, field):
    """Per (body node, channel): || sum_s |B_s| |phi_out - phi_i| / rn ||_2, and per body node cond_2(A / rn), in float64."""
    phi = node_values(m, field).astype(f64)
    q = np.zeros((len(bnode), 3), dtype=f64)
    cond = np.zeros(len(bnode), dtype=f64)
    for j, i in enumerate(np.asarray(bnode, dtype=np.int64)):
        s0, s1 = m["x_rowptr"][i], m["x_rowptr"][i + 1]
        rn = m["rn"][i].astype(f64)
        a = (np.abs(m["x_B"][s0:s1].astype(f64)).T @ np.abs(phi[m["x_out"][s0:s1]] - phi[i])) / rn[:, None]      # [M, 3]
        q[j] = np.linalg.norm(a, axis=0)
        cond[j] = np.linalg.cond(m["An"][i].astype(f64) / rn[:, None])
    return q, cond


# ---- stage 2: the six sums per graph ------------------------------------------------------------------------------------------------
def _terms(ps, pr, rs, rr, gs, gr, S, th3, th4, arm, sign):
    pf = 0.5 * ((ps + (rs * gs[:, 2]).sum(1)) + (pr + (rr * gr[:, 2]).sum(1)))
    Fp = (th3 * pf)[:, None] * S
    G = 0.5 * (gs[:, 0:2] + gr[:, 0:2])                                   # [Nf, c, a]
    Fv = sign * th4[:, None] * (G * S[:, None, :]).sum(2)
    Mp = arm[:, 0] * Fp[:, 1] + sign * arm[:, 1] * Fp[:, 0]
    Mv = arm[:, 0] * Fv[:, 1] + sign * arm[:, 1] * Fv[:, 0]
    return np.concatenate((Fp, Fv, Mp[:, None], Mv[:, None]), 1)


def _face_data(m, wface, origin, field):
    phi = node_values(m, field)
    w = np.asarray(wface, dtype=np.int64)
    f, k, ja, jb = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
    s, r = m["es"][f], m["er"][f]
    b = m["batch"][s]
    rs = (m["fpos"][f] - m["pos"][s]).astype(f32).astype(f64)            # (fp32 differences)
    rr = (m["fpos"][f] - m["pos"][r]).astype(f32).astype(f64)
    S = m["kS"][k].astype(f64)
    th3, th4 = m["theta"][b, 3].astype(f64), m["theta"][b, 4].astype(f64)
    ps, pr = phi[s, 2].astype(f64), phi[r, 2].astype(f64)
    arm = m["fpos"][f].astype(f64) - np.broadcast_to(np.asarray(origin, dtype=f32), (m["B"], 2)).astype(f64)[b]
    return (ps, pr, rs, rr, S, th3, th4, arm), ja, jb, b


def face_terms(m, wface, origin, field, gb):
    """The six terms per selected face [Nf, 6] = (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) in float64, their magnitudes [Nf, 6] - the same
    expressions with every operand replaced by its absolute value (what a rounding of an intermediate is relative to) - and the
    graph of every face."""
    (ps, pr, rs, rr, S, th3, th4, arm), ja, jb, b = _face_data(m, wface, origin, field)
    gs, gr = np.asarray(gb, dtype=f64)[ja], np.asarray(gb, dtype=f64)[jb]  # [Nf, 3, 2]
    t = _terms(ps, pr, rs, rr, gs, gr, S, th3, th4, arm, -1.0)
    mag = _terms(*(np.abs(v) for v in (ps, pr, rs, rr, gs, gr, S, th3, th4, arm)), 1.0)
    return t, mag, b


def gradient_sensitivity(m, wface, origin, field, dgb):
    """How far the six sums of every graph [B, 6] can move when every gradient entry gb[j, c, a] moves by at most dgb[j, c, a]: the
    magnitudes of the terms with the node values left out and the gradients replaced by their uncertainties, summed."""
    (ps, pr, rs, rr, S, th3, th4, arm), ja, jb, b = _face_data(m, wface, origin, field)
    d = np.abs(np.asarray(dgb, dtype=f64))
    mag = _terms(0.0 * ps, 0.0 * pr, np.abs(rs), np.abs(rr), d[ja], d[jb], np.abs(S), np.abs(th3), np.abs(th4), np.abs(arm), 1.0)
    return np.stack([mag[b == g].sum(0) for g in range(m["B"])])


def graph_sums(m, wface, origin, field, gb):
    """-> (sums [B, 6], magnitudes [B, 6]): per graph the correctly rounded sums (math.fsum) of the terms and of their magnitudes."""
    t, mag, b = face_terms(m, wface, origin, field, gb)
    out, amag = np.zeros((m["B"], SUMS), dtype=f64), np.zeros((m["B"], SUMS), dtype=f64)
    for g in range(m["B"]):
        rows = b == g
        for q in range(SUMS):
            out[g, q], amag[g, q] = math.fsum(t[rows, q]), math.fsum(mag[rows, q])
    return out, amag


# ---- the record and the ring --------------------------------------------------------------------------------------------------------
class WallForcesRef:
    """The record and the ring a sequence of launch pairs works on, and `launch()`: one pair applied to them."""

    def __init__(self, m, tables, origin, keep, start=1, stride=1, stop=-1, enabled=1):
        self.m, self.t, self.keep = m, tables, int(keep)
        self.origin = np.broadcast_to(np.asarray(origin, dtype=f32), (m["B"], 2))
        self.rec = np.zeros(RECORD, dtype=np.int32)
        self.rec[[START, STRIDE, STOP, ENABLED]] = (start, stride, stop, enabled)
        self.rec[LAST] = -1
        self.hist = np.zeros((self.keep, m["B"], SUMS), dtype=f64)
        self.hist_clock = np.zeros(self.keep, dtype=np.int32)
        self.mag = np.zeros((self.keep, m["B"], SUMS), dtype=f64)         # (the magnitudes of a row's sums: for the tests' bound)

    def reset(self):
        self.rec[LAST], self.rec[N] = -1, 0

    def launch(self, field, clock, gb=None):
        """field [N, >= 3] float32; clock: the value of the clock word; gb: the gradients the second stage reads (None: the first
        stage's own).  -> whether the pair sampled."""
        c = int(clock)
        taken = take(self.rec, c)
        if taken:
            if gb is None:
                gb = gradients(self.m, self.t["bnode"], field)
            row = int(self.rec[N]) % self.keep
            self.hist[row], self.mag[row] = graph_sums(self.m, self.t["wface"], self.origin, field, gb)
            self.hist_clock[row] = c
        commit(self.rec, c, taken)
        return taken

    def rows(self):
        """The last min(n, keep) rows in clock order: (clock [k], hist [k, B, 6], magnitudes [k, B, 6])."""
        n = int(self.rec[N])
        k = min(n, self.keep)
        order = [(n - k + q) % self.keep for q in range(k)]
        return self.hist_clock[order].copy(), self.hist[order].copy(), self.mag[order].copy()


# ---- the body's polygon (for the known answers) ---------------------------------------------------------------------------------
def shoelace_area(m, selected):
    """The area of the closed polygon the selected faces of ONE graph form (their end nodes chained), by the shoelace formula."""
    sel = np.asarray(selected, dtype=np.int64)
    nxt = {}
    for a, b in zip(m["es"][sel], m["er"][sel]):
        nxt.setdefault(int(a), []).append(int(b))
        nxt.setdefault(int(b), []).append(int(a))
    assert all(len(v) == 2 for v in nxt.values()), "the faces do not form closed loops"
    start = int(m["es"][sel[0]])
    loop, prev, cur = [start], None, start
    while True:
        a, b = nxt[cur]
        step = a if a != prev else b
        if step == start:
            break
        loop.append(step)
        prev, cur = cur, step
    assert len(loop) == len(nxt), "more than one loop"
    p = m["pos"][loop].astype(f64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))
