"""Flow integrals: the energy, enstrophy and mass balance of a run, per graph, summed on the device.

The scalars an unsteady run is judged by - has the transient died out (kinetic energy), is the wake shedding and resolved
(enstrophy, peak vorticity), how far is the field from divergence-free (the L2 and the max norm of the discrete divergence), does
what enters leave (the flux through the inflow and the outflow faces) - without a `.cpu()` of the field per step and without a
Green-Gauss loop of the user's own over the plan's incidence tables.  `FlowIntegrals` is ONE small launch behind the launch that
advances the field (`gfv_flow_integrals`; csrc/integrals.hip, include/gfv.h), following the owner's clock - `Rollout`'s step counter,
`MarchStep`'s level count - as `FieldStats`, `WallForces` and `Probes` do (gfv/follow.py), sampling the fields of the same window rule
(gfv/window.py):

    fi = FlowIntegrals(start=1, stride=1, stop=None, keep=4096, fields=False)
    r = Rollout(model, graphs, max_steps=2000, integrals=fi)
    r.run(steps=2000)
    h = fi.read()       # n, clock [k]; per sample and graph [k, B]: area, kinetic_energy, enstrophy, div_l2, div_max, vort_max,
                        # net_outflow, circulation, mean_pressure, inflow, outflow, other_flux; columns [k, B, 12]
    ms = MarchStep(model, graphs, ..., integrals=FlowIntegrals())        # one row per completed level
    clock, w, d = FlowIntegrals(fields=True) ... .cell_fields()          # the latest sample's cell vorticity and divergence [C]
    e = evaluate(graphs, field, fields=True)                             # one field, no owner: the same keys, [B]; vorticity, divergence [C]

What is summed.  Values are dimensionless, the units of `WallForces`: node values divided by `uvp_dim` (one fp32 division).  Per
cell, over its (cell, face) incidences with the cell's outward face vectors S and the trapezoid face value u_f = the mean of the
face's two end nodes (exact for a linear field; NOT the residual's reconstructed face value: no gradient, no LU):

    D = sum_k u_f . S          (the integral of div u over the cell)
    Gamma = sum_k (v_f S.x - u_f S.y)      (its circulation: the integral of the vorticity dv/dx - du/dy)

and the mean (ubar, vbar, pbar) over the cell's vertices.  Twelve columns per graph (include/gfv.h): the area, the kinetic energy
sum 1/2 |ubar|^2 a, the enstrophy sum 1/2 Gamma^2 / a, sum D^2 / a, the net outflow sum D, the circulation sum Gamma, sum pbar a, the
flux through the one-incidence faces typed INFLOW, OUTFLOW and anything else, and the maxima of |D| / a and |Gamma| / a.  Which
incidence is a boundary face of which kind (`btype`) is fixed when the owner attaches the object, as the wall forces' selection is: a
later edit of `face_type` does not move it.  The tables are plain torch ops that need no GPU: `build_btype`, `build_chunks`.

The ring holds the last `keep` samples; the time of a sample is joined through its clock (`Rollout`: clock * dt; a `MarchStep` with a
`StepControl`: `step_history()`).  No floating-point atomics, no sum across graphs, a fixed summation order: the same run gives the
same bits, and a row of the ring is bitwise what `evaluate()` returns for that step's field.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the record, the tables, the partial sums, the ring and its clocks, the cell fields.  One owner per object.  Not
part of any `state_dict()`.  Out of scope: `Sweep`, `PoolTrainStep`, `TrainStep`, data-parallel runs.
"""
from __future__ import annotations

import torch

from . import lib as L
from .fieldstats import check_field
from .follow import Follower
from .wallforce import check_keep, split_history
from .window import N_SAMPLES, UNCHANGED, Window

INFLOW, OUTFLOW = 1, 2                 # NodeType: the face types the balance tells apart
BT_INTERIOR, BT_INFLOW, BT_OUTFLOW, BT_OTHER = 0, 1, 2, 3
COLUMNS = L.FLOW_SUMS + L.FLOW_MAXS
# the columns of a row (include/gfv.h)
AREA, KINETIC, ENSTROPHY, DIV2, NET_OUTFLOW, CIRCULATION, PRESSURE_AREA, FLUX_IN, FLUX_OUT, FLUX_OTHER, DIV_MAX, VORT_MAX = range(12)


# ---- checks that need no GPU -----------------------------------------------------------------------------------------------------
def check_fields(fields):
    if not isinstance(fields, bool):
        raise ValueError(f"fields must be a bool (keep the cell vorticity and divergence of the latest sample), got {fields!r}")
    return fields


def check_graphs(graphs):
    """Batches of a DevicePool are refused (the pool rewrites their face types and swaps the meshes behind a plan; tables fixed
    at attach time would not follow it).  Needs no GPU."""
    if getattr(graphs[0], "_gfv_pool_plan", None) is not None:
        raise ValueError("FlowIntegrals: graphs of a DevicePool are not supported (the pool owns the meshes and face types of a "
                         "batch; Sweep and PoolTrainStep are out of scope)")


# ---- the tables: plain torch ops on whatever device the plan lives on ----------------------------------------------------------------
def build_btype(plan, face_type):
    """int32 [Sg]: per (cell, face) incidence 0 where its face has two incidences; where it has exactly one: 1 for an INFLOW face,
    2 for an OUTFLOW face, 3 for any other (include/gfv.h)."""
    ftype = torch.as_tensor(face_type).reshape(-1).to(device=plan.kface.device, dtype=torch.int64)
    if int(ftype.numel()) != int(plan.E):
        raise ValueError(f"FlowIntegrals: face_type has {int(ftype.numel())} entries, the plan {int(plan.E)} faces")
    frow = plan.frow.to(torch.int64)
    one = (frow[1:] - frow[:-1]) == 1
    kind = torch.where(ftype == INFLOW, BT_INFLOW, torch.where(ftype == OUTFLOW, BT_OUTFLOW, BT_OTHER))
    per_face = torch.where(one, kind, BT_INTERIOR)
    return per_face[plan.kface.to(torch.int64)].to(torch.int32).contiguous()


class FlowTables:
    """What build_tables makes: btype [Sg], cchunk_beg / cchunk_end [n_cchunks], gcchunk_ptr [B + 1] (int32, on the plan's device),
    cells [B] (int64, CPU: cells per graph), n_cchunks, C, B."""


def build_chunks(gcell_ptr, chunk=L.FLOW_CHUNK):
    """The cell chunks of a batch from its graphs' cell ranges [B + 1]: at most `chunk` consecutive cells, never across a graph ->
    (cchunk_beg, cchunk_end, gcchunk_ptr) as lists."""
    ptr = [int(v) for v in torch.as_tensor(gcell_ptr).reshape(-1).tolist()]
    beg, end, gcp = [], [], [0]
    for b in range(len(ptr) - 1):
        for st in range(ptr[b], ptr[b + 1], chunk):
            beg.append(st)
            end.append(min(st + chunk, ptr[b + 1]))
        gcp.append(len(beg))
    return beg, end, gcp


def build_tables(plan, face_type):
    dev = plan.kface.device
    t = FlowTables()
    t.btype = build_btype(plan, face_type)
    beg, end, gcp = build_chunks(plan.gcell_ptr)
    if not beg:
        raise ValueError("FlowIntegrals: the batch holds no cell")
    t.cchunk_beg = torch.tensor(beg, dtype=torch.int32, device=dev)
    t.cchunk_end = torch.tensor(end, dtype=torch.int32, device=dev)
    t.gcchunk_ptr = torch.tensor(gcp, dtype=torch.int32, device=dev)
    ptr = plan.gcell_ptr.cpu().to(torch.int64)
    t.cells = (ptr[1:] - ptr[:-1]).clone()
    t.n_cchunks, t.C, t.B = len(beg), int(plan.C), int(plan.B)
    return t


def split_columns(rows):
    """Rows [..., B, 12] float64 -> the named quantities of read(), each [..., B].  A graph without cells has a row of zeros: its
    div_l2 and mean_pressure (0 / 0) are given as 0."""
    a = rows[..., AREA]
    per_area = lambda v: torch.where(a > 0, v / a, torch.zeros_like(v))
    return {"area": a.clone(), "kinetic_energy": rows[..., KINETIC].clone(), "enstrophy": rows[..., ENSTROPHY].clone(),
            "div_l2": torch.sqrt(per_area(rows[..., DIV2])), "div_max": rows[..., DIV_MAX].clone(), "vort_max": rows[..., VORT_MAX].clone(),
            "net_outflow": rows[..., NET_OUTFLOW].clone(), "circulation": rows[..., CIRCULATION].clone(),
            "mean_pressure": per_area(rows[..., PRESSURE_AREA]), "inflow": rows[..., FLUX_IN].clone(),
            "outflow": rows[..., FLUX_OUT].clone(), "other_flux": rows[..., FLUX_OTHER].clone(), "columns": rows.clone()}


class FlowIntegrals(Follower):
    KEYWORD = "integrals"
    NO_ANDERSON = ("the ring would record integrals of fields that are not steps; call gfv.integrals.evaluate() on the converged "
                   "field")

    def __init__(self, start=1, stride=1, stop=None, keep=4096, fields=False):
        self._window = Window(start, stride, stop)
        self.keep = check_keep(keep)
        self.fields = check_fields(fields)
        # device state: allocated by attach(), never reallocated
        self.rec = self.tables = self.partial = self.hist = self.hist_clock = self.cell_out = None
        self._plan = None

    start = property(lambda self: self._window.start)
    stride = property(lambda self: self._window.stride)
    stop = property(lambda self: self._window.stop)
    enabled = property(lambda self: self._window.enabled)

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    _check_graphs = staticmethod(check_graphs)

    def attach(self, owner, graphs, plan, x_backup, clock, clock_word=0):
        """Called by the owner's constructor with the tensor it advances, its int32 record `clock` and the word of it that counts
        the fields written: fixes the boundary kinds, builds the tables and allocates the record and the state (once).  -> self"""
        self.check_free()
        check_graphs(graphs)
        n = check_field(x_backup)
        if n != plan.N:
            raise ValueError(f"FlowIntegrals: the node state has {n} rows, the plan {plan.N}")
        dev = x_backup.device
        t = build_tables(plan, graphs[2].face_type)
        self.partial = torch.zeros((t.n_cchunks, COLUMNS), dtype=torch.float64, device=dev)
        self.hist = torch.zeros((self.keep, t.B, COLUMNS), dtype=torch.float64, device=dev)
        self.hist_clock = torch.zeros(self.keep, dtype=torch.int32, device=dev)
        self.cell_out = torch.zeros((t.C, 2), dtype=torch.float64, device=dev) if self.fields else None
        self._xb, self._clock, self._clock_ptr = x_backup, clock, clock.data_ptr() + 4 * int(clock_word)
        self.tables, self._plan, self.rec = t, plan, self._window.attach(dev)
        self._claim(owner)
        return self

    def launch(self):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        pl, t = self._plan, self.tables
        L.check(L.load().gfv_flow_integrals(
            self._xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.crow.data_ptr(), pl.kface.data_ptr(), pl.knode.data_ptr(),
            pl.kS.data_ptr(), t.btype.data_ptr(), pl.es.data_ptr(), pl.er.data_ptr(), pl.area.data_ptr(), t.cchunk_beg.data_ptr(),
            t.cchunk_end.data_ptr(), t.gcchunk_ptr.data_ptr(), t.n_cchunks, t.C, t.B, self._clock_ptr, self.rec.data_ptr(),
            self.partial.data_ptr(), self.hist.data_ptr(), self.hist_clock.data_ptr(), self.keep,
            self.cell_out.data_ptr() if self.cell_out is not None else None, L.stream_ptr()), "gfv_flow_integrals")

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

    def _packed(self, *more):
        nb_rec, nb_hist, nb_clock = 4 * L.FLOW_RECORD, 8 * self.hist.numel(), 4 * self.keep
        packed = torch.cat([self.rec.view(torch.uint8), self.hist.view(torch.uint8).reshape(-1), self.hist_clock.view(torch.uint8)]
                           + [m.view(torch.uint8).reshape(-1) for m in more]).cpu()
        a, b = nb_rec + nb_hist, nb_rec + nb_hist + nb_clock
        return (packed[:nb_rec].view(torch.int32).clone(),
                packed[nb_rec:a].view(torch.float64).reshape(tuple(self.hist.shape)).clone(),
                packed[a:b].view(torch.int32).clone(), packed[b:].clone())      # (a copy: a view at an odd word cannot be doubles)

    def raw(self):
        """(record [8] int32, hist [keep, B, 12] float64, hist_clock [keep] int32) as CPU copies (one synchronisation)."""
        self._need()
        return self._packed()[0:3]

    def read(self):
        """{"n", "clock" [k], and per sample and graph [k, B]: "area", "kinetic_energy", "enstrophy", "div_l2" (= sqrt(div^2 / area)),
        "div_max", "vort_max", "net_outflow", "circulation", "mean_pressure" (= pressure . area / area), "inflow", "outflow",
        "other_flux"; "columns" [k, B, 12]: the rows as the device holds them; "cells" [B]} as CPU tensors, k = min(n, keep) rows in
        clock order (k may be 0).  float64; dimensionless.  Fluxes are outward: an inflow is negative.  A graph without cells has
        zeros throughout."""
        rec, hist, hclock = self.raw()
        n = int(rec[N_SAMPLES])
        clock, rows = split_history(n, self.keep, hist, hclock)
        return dict(split_columns(rows), n=n, clock=clock, cells=self.tables.cells.clone())

    def cell_fields(self):
        """(clock, vorticity [C], divergence [C]) of the latest sample as CPU float64 tensors (one synchronisation): Gamma_C / a and
        D_C / a of every cell.  Needs `fields=True` and a sample."""
        self._need()
        if self.cell_out is None:
            raise RuntimeError("this FlowIntegrals keeps no cell fields: build it with fields=True")
        rec, _, hclock, rest = self._packed(self.cell_out)
        n = int(rec[N_SAMPLES])
        if n < 1:
            raise RuntimeError("FlowIntegrals.cell_fields: no sample has been taken yet")
        out = rest.view(torch.float64).reshape(-1, 2)
        return int(hclock[(n - 1) % self.keep]), out[:, 0].clone(), out[:, 1].clone()


def evaluate(graphs, field, fields=False):
    """The integrals of one field, no owner: the same launch on a clock word of its own.  field: [N, 3] (u, v, p) or [N, 12] (a
    node state), dimensional, on the GPU.  -> the named quantities of read(), each [B], "columns" [B, 12] and, with `fields`,
    "vorticity" [C] and "divergence" [C], as float64 CPU tensors (one synchronisation)."""
    from .functions import require_gpu
    from .plan import get_plan
    if not isinstance(field, torch.Tensor) or field.dim() != 2 or field.shape[1] not in (3, 12):
        raise ValueError("evaluate: field must be a [N, 3] or [N, 12] tensor")
    fi = FlowIntegrals(start=1, keep=1, fields=fields)
    require_gpu(field)
    require_gpu(graphs[0].x)
    check_graphs(graphs)
    plan = get_plan(graphs)
    if int(field.shape[0]) != plan.N:
        raise ValueError(f"evaluate: field has {int(field.shape[0])} rows, the graphs {plan.N} nodes")
    xb = torch.zeros((plan.N, 12), dtype=torch.float32, device=field.device)
    xb[:, 0:3] = field[:, 0:3].to(torch.float32)
    clock = torch.ones(1, dtype=torch.int32, device=field.device)
    fi.attach("evaluate", graphs, plan, xb, clock)
    fi.launch()
    rec, hist, _, rest = fi._packed(*([fi.cell_out] if fields else []))
    assert int(rec[N_SAMPLES]) == 1
    out = split_columns(hist[0])
    if fields:
        cells = rest.view(torch.float64).reshape(-1, 2)
        out["vorticity"], out["divergence"] = cells[:, 0].clone(), cells[:, 1].clone()
    return out
