"""Probes: the signal of a run at fixed points and along lines, interpolated on the device.

What every user of an unsteady run asks for - the velocity behind the cylinder for the shedding frequency, the pressure at the
stagnation point, the vorticity in the wake, the u(y) centreline of the lid-driven cavity - without a `.cpu()` of the field per
step and without a point-in-cell search of the user's own.  `Probes` is ONE small launch behind the launch that advances the field
(`gfv_probe_sample`; csrc/probes.hip, include/gfv.h), following the owner's clock - `Rollout`'s step counter, `MarchStep`'s level
count - as `FieldStats` and `WallForces` do (gfv/follow.py), sampling the fields of the same window rule (gfv/window.py):

    pr = Probes(points, graph=None, start=1, stride=1, stop=None, keep=4096, tolerance=1e-6)
    pts = line((0.3, 0.2), (1.0, 0.2), 32)          # [32, 2] float64, end points included: a wake rake, the cavity centreline
    r = Rollout(model, graphs, max_steps=2000, probes=pr)
    r.run(steps=2000)
    h = pr.read()       # n, clock [k], value [k,P,3], gradient [k,P,3,2], points [P,2], graph [P], cell [P], outside [P], uvp_dim [P,3]
    w, d = vorticity(h), divergence(h)              # [k, P], on the host: v_x - u_y, u_x + v_y
    ms = MarchStep(model, graphs, ..., probes=Probes(pts))       # one sample per completed level
    s = sample(graphs, field, pts)                  # one field, no owner: value [P,3], gradient [P,3,2], cell [P], outside [P]

What a probe is.  A point `x` and the graph it lies in (`graph`: an int for all points or one per point; None only for a batch of
one graph - the graphs of a batch may overlap in space).  Values are dimensionless, the units of `WallForces`: node values divided
by `uvp_dim` (one fp32 division); `h["uvp_dim"]` holds the factors of every probe's graph.

Location, once, when the owner attaches the object.  For every cell C of the graph, d(C) = the largest signed distance of x to
the lines of the cell's faces (outward positive, from the stored face centres and outward face vectors); the probe's cell is the
cell of least d, the lowest index among equals.  CELLS ARE TAKEN AS CONVEX: d <= 0 exactly inside a convex cell, and a non-convex
cell may claim a point of its neighbour.  `outside` = d / sqrt(cell area) says how far, as a fraction of the cell's size, the point
lies outside the mesh; above `tolerance` the point is refused (inside a body, beyond the boundary), below it the probe is accepted,
unmoved.

Interpolation.  The scheme's own second-order reconstruction - node value plus WLSQ gradient times offset, as the face kernel
forms a face value from its two ends - averaged over the k vertices of the cell with equal weights:

    value_c(x) = (1/k) sum_v ( phi_c(v) + g_v[c] . (x - pos[v]) )        gradient_c(x) = (1/k) sum_v g_v[c]

Both are fixed linear functionals of the node values, so all the linear algebra - the transposed WLSQ systems of the vertices, the
merge of their stencils - is done once at attach time, in float64 (`build_tables`, plain torch, needs no GPU, the same bits run
after run), and a step pays one launch: a sparse dot product of a few dozen entries per probe, in double, in a fixed order.  The
rule in full: include/gfv.h.

The ring holds the last `keep` samples; the time of a sample is joined through its clock (`Rollout`: clock * dt; a `MarchStep` with a
`StepControl`: `step_history()`).  A row of the ring is bitwise what `sample()` returns for that step's field.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the record, the weight tables, the ring and its clocks.  One owner per object.  Not part of any `state_dict()`.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import lib as L
from .fieldstats import check_field
from .follow import Follower
from .wallforce import TERMS, check_keep, split_history
from .window import N_SAMPLES, UNCHANGED, Window

LOCATE_ELEMENTS = 2 ** 24      # no intermediate of the location is larger


# ---- checks that need no GPU -----------------------------------------------------------------------------------------------------
def check_points(points):
    """-> [P, 2] float64 CPU tensor, P >= 1, every number finite."""
    try:
        if isinstance(points, torch.Tensor):
            p = points.detach().to(device="cpu", dtype=torch.float64)
        else:                                                  # (Python floats are doubles: they must not pass through fp32)
            p = torch.from_numpy(np.array(points, dtype=np.float64))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"points must be [P, 2] finite numbers, got {points!r}") from None
    if p.dim() != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError(f"points must be [P, 2] with P >= 1, got shape {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError("points must be finite numbers")
    return p.contiguous().clone()


def check_graph(graph, P, B=None):
    """None, an int or P ints -> None or a list of P ints; with B: checked against 0 .. B - 1, None allowed only for B == 1 (then
    a list of zeros)."""
    is_int = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if graph is None:
        if B is not None and B != 1:
            raise ValueError(f"graph=None needs a batch of one graph; this batch has {B} (graphs of a batch may overlap in space: "
                             "say which graph every point lies in)")
        return None if B is None else [0] * P
    if is_int(graph):
        out = [int(graph)] * P
    else:
        if isinstance(graph, torch.Tensor):
            if graph.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
                raise ValueError(f"graph must be an int or {P} ints, got dtype {graph.dtype}")
            graph = graph.reshape(-1).tolist()
        try:
            out = list(graph)
        except TypeError:
            raise ValueError(f"graph must be None, an int or {P} ints, got {graph!r}") from None
        if not all(is_int(v) for v in out):
            raise ValueError(f"graph must be None, an int or {P} ints, got {graph!r}")
        if len(out) != P:
            raise ValueError(f"graph: one int per point: {len(out)} for {P} points")
        out = [int(v) for v in out]
    if min(out) < 0 or (B is not None and max(out) >= B):
        raise ValueError(f"graph: an index outside 0 .. {'B - 1' if B is None else B - 1}")
    return out


def check_tolerance(tolerance):
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real) or not 0 <= tolerance < float("inf"):
        raise ValueError(f"tolerance must be a finite number >= 0 (a fraction of the cell's size), got {tolerance!r}")
    return float(tolerance)


def check_graphs(graphs):
    """Batches of a DevicePool are refused (the pool swaps the meshes behind a plan; a location fixed at attach time would not
    follow it).  Needs no GPU."""
    if getattr(graphs[0], "_gfv_pool_plan", None) is not None:
        raise ValueError("Probes: graphs of a DevicePool are not supported (the pool owns the meshes of a batch; Sweep and "
                         "PoolTrainStep are out of scope)")


def line(p0, p1, n):
    """n points from p0 to p1, evenly spaced, both end points included and exact -> [n, 2] float64."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 2:
        raise ValueError(f"line: n must be an integer >= 2 (both end points are included), got {n!r}")
    ends = check_points([p0, p1])
    t = (torch.arange(n, dtype=torch.float64) / float(n - 1)).reshape(-1, 1)
    out = ends[0] + t * (ends[1] - ends[0])
    out[0], out[-1] = ends[0], ends[1]
    return out


# ---- location: plain torch, on the host, in float64 -----------------------------------------------------------------------------
def locate(plan, points, graph=None, tolerance=1e-6):
    """The cell of every point -> (cell [P] int64, outside [P] float64, graph [P] int64), CPU tensors.  Cells are taken as convex.
    ValueError names the first point whose `outside` exceeds `tolerance`."""
    pts = check_points(points)
    P, B = int(pts.shape[0]), int(plan.B)
    gr = torch.tensor(check_graph(graph, P, B), dtype=torch.int64)
    tolerance = check_tolerance(tolerance)
    crow = plan.crow.cpu().to(torch.int64)
    gptr = plan.gcell_ptr.cpu().to(torch.int64)
    kface = plan.kface.cpu().to(torch.int64)
    kS = plan.kS.cpu().to(torch.float64)
    fc = plan.fpos.cpu().to(torch.float64)[kface]                                  # [Sg, 2]: the face centre of an incidence
    area = plan.area.cpu().to(torch.float64)
    slen = torch.sqrt(kS[:, 0] * kS[:, 0] + kS[:, 1] * kS[:, 1])
    kcell = torch.repeat_interleave(torch.arange(crow.numel() - 1, dtype=torch.int64), crow[1:] - crow[:-1])
    cell = torch.zeros(P, dtype=torch.int64)
    dmin = torch.zeros(P, dtype=torch.float64)
    for b in range(B):
        mine = torch.nonzero(gr == b).reshape(-1)
        if mine.numel() == 0:
            continue
        c0, c1 = int(gptr[b]), int(gptr[b + 1])
        k0, k1 = int(crow[c0]), int(crow[c1])
        if c1 <= c0 or k1 <= k0:
            raise ValueError(f"Probes: graph {b} has no cell")
        nk, nc = k1 - k0, c1 - c0
        col = (kcell[k0:k1] - c0).reshape(1, nk)
        ids = torch.arange(nc, dtype=torch.int64).reshape(1, nc)
        rows = max(1, LOCATE_ELEMENTS // nk)
        for r0 in range(0, int(mine.numel()), rows):
            sel = mine[r0:r0 + rows]
            x = pts[sel]                                                           # [R, 2]
            dk = ((x[:, 0:1] - fc[k0:k1, 0]) * kS[k0:k1, 0] + (x[:, 1:2] - fc[k0:k1, 1]) * kS[k0:k1, 1]) / slen[k0:k1]
            d = torch.full((int(sel.numel()), nc), -math.inf, dtype=torch.float64)
            d = d.scatter_reduce(1, col.expand(int(sel.numel()), nk), dk, "amax")  # (a maximum: no order to depend on)
            least = d.min(1).values
            first = torch.where(d == least.reshape(-1, 1), ids, nc).min(1).values  # ties: the lowest index
            cell[sel], dmin[sel] = first + c0, least
    outside = dmin / torch.sqrt(area[cell])
    bad = torch.nonzero(~(outside <= tolerance)).reshape(-1)                       # (a NaN is refused too)
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"Probes: {int(bad.numel())} of {P} points lie outside the mesh; point {i} ({float(pts[i, 0])!r}, "
                         f"{float(pts[i, 1])!r}) of graph {int(gr[i])} has outside = {float(outside[i]):.6g} of its nearest cell's "
                         f"size (cell {int(cell[i])}), tolerance {tolerance:g}")
    return cell, outside, gr


# ---- the weights: plain torch, on the host, in float64 ----------------------------------------------------------------------------
class ProbeTables:
    """What build_tables makes: pw_ptr [P + 1] int32, pw_node [nnz] int32, pw_w [nnz, 3] float64 (CPU tensors until placed), P,
    nnz."""

    def to(self, dev):
        self.pw_ptr, self.pw_node, self.pw_w = (t.to(dev).contiguous() for t in (self.pw_ptr, self.pw_node, self.pw_w))
        return self


def build_tables(plan, points, cell):
    """The CSR weight table of include/gfv.h for probes at `points` [P, 2] located in `cell` [P].  The rows the few vertices need
    are gathered to the host; duplicates are merged by sort-and-segment, each segment summed by math.fsum (correctly rounded: no
    order to depend on) - the same inputs give the same bytes."""
    pts = check_points(points)
    cell = torch.as_tensor(cell).reshape(-1).to(device="cpu", dtype=torch.int64)
    P, M = int(pts.shape[0]), int(plan.M)
    if int(cell.numel()) != P:
        raise ValueError(f"build_tables: {int(cell.numel())} cells for {P} points")
    if M not in TERMS:
        raise ValueError(f"Probes: the plan's reconstruction has {M} terms; 2, 5, 9 and 14 are supported")
    if int(cell.min()) < 0 or int(cell.max()) >= int(plan.C):
        raise ValueError(f"build_tables: a cell index outside 0 .. {int(plan.C) - 1}")
    dev = plan.crow.device
    cd = cell.to(dev)
    crow = plan.crow.to(torch.int64)
    cb, ce = crow[cd].cpu(), crow[cd + 1].cpu()
    kcount = ce - cb                                                               # k: the vertices of a probe's cell
    kidx = torch.cat([torch.arange(int(a), int(e), dtype=torch.int64) for a, e in zip(cb, ce)])
    vert = plan.knode.to(torch.int64)[kidx.to(dev)].cpu()                          # the vertices, probe after probe
    vprobe = torch.repeat_interleave(torch.arange(P, dtype=torch.int64), kcount)
    uv, vpos = torch.unique(vert, return_inverse=True)                             # (sorted)
    uvd = uv.to(dev)
    U = int(uv.numel())
    # ---- per unique vertex: z_a of (A / rn)^T z_a = e_a, a = 0, 1 ---------------------------------------------------------------
    rn = plan.rn.reshape(-1, M)[uvd].cpu().to(torch.float64)                       # [U, M]
    A = plan.An.reshape(-1, M, M)[uvd].cpu().to(torch.float64) / rn.reshape(U, M, 1)
    rhs = torch.zeros((U, M, 2), dtype=torch.float64)
    rhs[:, 0, 0] = rhs[:, 1, 1] = 1.0
    Z = torch.linalg.solve(A.transpose(1, 2), rhs)                                 # [U, M, 2]
    rp = plan.x_rowptr.to(torch.int64)
    s0, s1 = rp[uvd].cpu(), rp[uvd + 1].cpu()
    sidx = torch.cat([torch.arange(int(a), int(e), dtype=torch.int64) for a, e in zip(s0, s1)] + [torch.zeros(0, dtype=torch.int64)])
    sown = torch.repeat_interleave(torch.arange(U, dtype=torch.int64), s1 - s0)
    Bn = plan.x_B.reshape(-1, M)[sidx.to(dev)].cpu().to(torch.float64) / rn[sown]  # [S', M]
    sout = plan.x_out.to(torch.int64)[sidx.to(dev)].cpu()
    t = torch.einsum("sm,sma->sa", Bn, Z[sown])                                    # [S', 2]: dg_a / dphi(x_out[s]) at the vertex
    pos = plan.pos[uvd].cpu().to(torch.float64)                                    # [U, 2]
    sfirst = torch.zeros(U + 1, dtype=torch.int64)
    sfirst[1:] = torch.cumsum(s1 - s0, 0)
    # ---- per probe: the entries of its vertices, merged ------------------------------------------------------------------------
    ptr, nodes, weights = [0], [], []
    vfirst = torch.zeros(P + 1, dtype=torch.int64)
    vfirst[1:] = torch.cumsum(kcount, 0)
    for p in range(P):
        k = int(kcount[p])
        ent_node, ent_w = [], []
        x = pts[p]
        for q in range(int(vfirst[p]), int(vfirst[p + 1])):
            u = int(vpos[q])
            a, e = int(sfirst[u]), int(sfirst[u + 1])
            ta = t[a:e] / float(k)                                                 # [S, 2]
            off = x - pos[u]
            n_out = sout[a:e]
            n_own = torch.full((e - a,), int(uv[u]), dtype=torch.int64)
            for nn, sign in ((n_out, 1.0), (n_own, -1.0)):
                g = sign * ta
                ent_node.append(nn)
                ent_w.append(torch.stack((off[0] * g[:, 0] + off[1] * g[:, 1], g[:, 0], g[:, 1]), 1))
            ent_node.append(torch.tensor([int(uv[u])], dtype=torch.int64))
            ent_w.append(torch.tensor([[1.0 / float(k), 0.0, 0.0]], dtype=torch.float64))
        en, ew = torch.cat(ent_node), torch.cat(ent_w)
        order = torch.sort(en, stable=True).indices
        en, ew = en[order].tolist(), ew[order].tolist()
        i = 0
        while i < len(en):
            j = i
            while j < len(en) and en[j] == en[i]:
                j += 1
            nodes.append(en[i])
            weights.append([math.fsum(r[c] for r in ew[i:j]) for c in range(3)])
            i = j
        ptr.append(len(nodes))
    tb = ProbeTables()
    tb.pw_ptr = torch.tensor(ptr, dtype=torch.int32)
    tb.pw_node = torch.tensor(nodes, dtype=torch.int32)
    tb.pw_w = torch.tensor(weights, dtype=torch.float64).reshape(-1, 3)
    tb.P, tb.nnz = P, len(nodes)
    return tb


def split_rows(rows):
    """Ring rows [k, P, 9] float64 -> (value [k, P, 3], gradient [k, P, 3, 2])."""
    r = rows.reshape(rows.shape[0], rows.shape[1], 3, 3)
    return r[:, :, :, 0].contiguous(), r[:, :, :, 1:3].contiguous()


class Probes(Follower):
    KEYWORD = "probes"
    NO_ANDERSON = "the ring would record the signal of fields that are not steps; call gfv.probes.sample() on the converged field"

    def __init__(self, points, graph=None, start=1, stride=1, stop=None, keep=4096, tolerance=1e-6):
        self.points = check_points(points)
        self._graph = check_graph(graph, int(self.points.shape[0]))                # (checked against B when the owner is known)
        self._window = Window(start, stride, stop)
        self.keep = check_keep(keep)
        self.tolerance = check_tolerance(tolerance)
        # device state: allocated by attach(), never reallocated
        self.rec = self.tables = self.hist = self.hist_clock = None
        self.graph = self.cell = self.outside = None
        self._plan = None
        self.P = int(self.points.shape[0])

    start = property(lambda self: self._window.start)
    stride = property(lambda self: self._window.stride)
    stop = property(lambda self: self._window.stop)
    enabled = property(lambda self: self._window.enabled)

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    def _check_graphs(self, graphs):
        check_graphs(graphs)
        check_graph(self._graph, self.P, int(graphs[4].theta_PDE.shape[0]))

    def attach(self, owner, graphs, plan, x_backup, clock, clock_word=0):
        """Called by the owner's constructor with the tensor it advances, its int32 record `clock` and the word of it that counts
        the fields written: locates the points, builds the weight tables and allocates the record and the ring (once).  -> self"""
        self.check_free()
        self._check_graphs(graphs)
        n = check_field(x_backup)
        if n != plan.N:
            raise ValueError(f"Probes: the node state has {n} rows, the plan {plan.N}")
        if int(plan.M) not in TERMS:
            raise ValueError(f"Probes: the plan's reconstruction has {plan.M} terms; 2, 5, 9 and 14 are supported")
        dev = x_backup.device
        cell, outside, gr = locate(plan, self.points, self._graph, self.tolerance)
        t = build_tables(plan, self.points, cell).to(dev)
        self.hist = torch.zeros((self.keep, self.P, L.PROBE_SUMS), dtype=torch.float64, device=dev)
        self.hist_clock = torch.zeros(self.keep, dtype=torch.int32, device=dev)
        self._xb, self._clock, self._clock_ptr = x_backup, clock, clock.data_ptr() + 4 * int(clock_word)
        self.graph, self.cell, self.outside = gr, cell, outside
        self.tables, self._plan, self.rec = t, plan, self._window.attach(dev)
        self._claim(owner)
        return self

    def launch(self):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        pl, t = self._plan, self.tables
        L.check(L.load().gfv_probe_sample(self._xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.batch.data_ptr(), t.pw_ptr.data_ptr(),
                                          t.pw_node.data_ptr(), t.pw_w.data_ptr(), self.P, self._clock_ptr, self.rec.data_ptr(),
                                          self.hist.data_ptr(), self.hist_clock.data_ptr(), self.keep, L.stream_ptr()),
                "gfv_probe_sample")

    def set_window(self, start=None, stride=None, stop=UNCHANGED, enabled=None):
        """`Window.set`: a new window under recorded lists.  The history so far stays: reset() starts over."""
        self._window.set(start, stride, stop, enabled)

    def reset(self):
        """`Window.reset`, in stream order; the owner's reset() calls it.  The ring needs no clearing (rows are read up to n)."""
        self._need()
        self._window.reset()

    # ---- reading (each of these is one synchronisation) ----------------------------------------------------------------------
    def count(self):
        """Samples taken so far."""
        self._need()
        return self._window.count()

    def raw(self):
        """(record [8] int32, hist [keep, P, 9] float64, hist_clock [keep] int32) as CPU copies (one synchronisation)."""
        self._need()
        nb_rec, nb_hist = 4 * L.PROBE_RECORD, 8 * self.hist.numel()
        packed = torch.cat([self.rec.view(torch.uint8), self.hist.view(torch.uint8).reshape(-1),
                            self.hist_clock.view(torch.uint8)]).cpu()
        return (packed[:nb_rec].view(torch.int32).clone(),
                packed[nb_rec:nb_rec + nb_hist].view(torch.float64).reshape(tuple(self.hist.shape)).clone(),
                packed[nb_rec + nb_hist:].view(torch.int32).clone())

    def read(self):
        """{"n", "clock" [k], "value" [k,P,3], "gradient" [k,P,3,2], "points" [P,2], "graph" [P], "cell" [P], "outside" [P],
        "uvp_dim" [P,3]} as CPU tensors, k = min(n, keep) rows in clock order (k may be 0).  value[.., c] and gradient[.., c, :] =
        (d/dx, d/dy) of channel c = u, v, p; float64, dimensionless (times uvp_dim: dimensional)."""
        rec, hist, hclock = self.raw()
        n = int(rec[N_SAMPLES])
        clock, rows = split_history(n, self.keep, hist, hclock)
        value, gradient = split_rows(rows)
        dim = self._plan.uvp_dim.reshape(-1, 3).cpu().to(torch.float32)[self.graph]
        return {"n": n, "clock": clock, "value": value, "gradient": gradient, "points": self.points.clone(),
                "graph": self.graph.clone(), "cell": self.cell.clone(), "outside": self.outside.clone(), "uvp_dim": dim}


def vorticity(h):
    """v_x - u_y of every row and probe of a read() -> [k, P] (on the host)."""
    g = h["gradient"]
    return g[..., 1, 0] - g[..., 0, 1]


def divergence(h):
    """u_x + v_y of every row and probe of a read() -> [k, P] (on the host)."""
    g = h["gradient"]
    return g[..., 0, 0] + g[..., 1, 1]


def sample(graphs, field, points, graph=None, tolerance=1e-6):
    """The probes of one field, no owner: the same launch on a clock word of its own.  field: [N, 3] (u, v, p) or [N, 12] (a node
    state), dimensional, on the GPU.  -> {"value" [P,3], "gradient" [P,3,2], "cell" [P], "outside" [P]} CPU tensors (one
    synchronisation)."""
    from .functions import require_gpu
    from .plan import get_plan
    if not isinstance(field, torch.Tensor) or field.dim() != 2 or field.shape[1] not in (3, 12):
        raise ValueError("sample: field must be a [N, 3] or [N, 12] tensor")
    pr = Probes(points, graph=graph, start=1, keep=1, tolerance=tolerance)
    require_gpu(field)
    require_gpu(graphs[0].x)
    plan = get_plan(graphs)
    if int(field.shape[0]) != plan.N:
        raise ValueError(f"sample: field has {int(field.shape[0])} rows, the graphs {plan.N} nodes")
    xb = torch.zeros((plan.N, 12), dtype=torch.float32, device=field.device)
    xb[:, 0:3] = field[:, 0:3].to(torch.float32)
    clock = torch.ones(1, dtype=torch.int32, device=field.device)
    pr.attach("sample", graphs, plan, xb, clock)
    pr.launch()
    rec, hist, _ = pr.raw()
    assert int(rec[N_SAMPLES]) == 1
    value, gradient = split_rows(hist)
    return {"value": value[0], "gradient": gradient[0], "cell": pr.cell.clone(), "outside": pr.outside.clone()}
