"""Second-order time differencing on the device (gfv/timescheme.py, csrc/timescheme.hip; include/gfv.h gfv_time_scheme_update,
gfv_phi_fwd_ts).

1. the kernel alone against the numpy rule of tests/timescheme_ref.py, launch by launch, bit for bit;
2. the finite-volume section with a separate baseline and step against float64, stage by stage and one loss of one graph at a
   time; the tolerances are tests/fvm_float64.py's (4 x the float32 oracle's own error on the same inputs, floor 2^-22);
3. nothing changes until history exists: "bdf1" is a march without a scheme, "bdf2" is one through the end of level 0;
4. the device-decided march equals the host-driven loop, bit for bit, in eager, list and hipGraph mode;
5. run-ahead, held steps, reset and resume;   6. together with time_bc and field_stats, in either order of the launches;
7. the refusals that need the device.

Measured on the MI355X (2: largest column of each family over the 18 cases, per-graph max-normalised; yardstick = the float32
oracle on the same inputs, of which the tolerance is 4 x per column):

    family                       yardstick, poly / cyl_cavity_b2              kernels
    phi                          5.5e-08 ... 6.5e-08                          5.1e-08 ... 8.3e-08   (floor 2^-22)
    grad, Ff, phic, gradc        4.5e-05 ... 1.0e-04 / 6.5e-07 ... 2.2e-06    6.3e-08 ... 1.5e-07
    cres                         3.0e-05 ... 1.5e-04 / 1.7e-06                9.2e-08 ... 4.4e-07
    sums, losses                 1.5e-05 ... 5.4e-05 / 4.9e-07 ... 9.2e-07    3.1e-08 ... 2.8e-07
    uvp_node, uvp_cell           4.1e-05 ... 4.4e-05 / 6.3e-07 ... 6.8e-07    9.7e-08 ... 1.6e-07
    one-hot gdec                 8.3e-05 ... 2.9e-04 / 1.7e-06 ... 4.4e-06    4.9e-06 ... 1.1e-05 / 3.8e-07 ... 4.6e-07
    a reference without the baseline / without the step, cres momentum columns: at least 332 x / 329 x the tolerance (poly,
    conserved, implicit), up to 4.1e5 x"""
import functools

import numpy as np
import pytest
import torch

import fvm_float64 as F
import timescheme_ref as R
from test_march_gpu import LR, TOL, _assert_same, _graphs, _cpu_graphs, _model, _same_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
MAX_INNER = 5
CLOCKS = (0, 0, 1, 1, 1, 2, 3)
SEED_COEF, SEED_DEC, SEED_STAR = 7, 11, 13


def _same(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
class _Kernel:
    """The launch at the C ABI on buffers of its own, with one guard row / element behind ustar and dt_eff."""

    def __init__(self, sizes, scheme, seed):
        g = np.random.default_rng(seed)
        self.B, self.N = len(sizes), int(sum(sizes))
        self.batch = np.repeat(np.arange(self.B), sizes).astype(np.int32)
        self.dim = (0.5 + g.random((self.B, 3))).astype(f32)            # distinct per graph and per column
        self.dt = (0.01 * (1.0 + np.arange(self.B)) * (1.0 + g.random(self.B))).astype(f32)
        # four fields whose rows carry distinct values in every column: a launch reading another column computes something else
        self.fields = [(g.standard_normal((self.N, 12)) + np.arange(12)[None, :]).astype(f32) for _ in range(4)]
        self.previous = g.standard_normal((self.N, 3)).astype(f32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d_batch, self.d_dim, self.d_dt = d(self.batch), d(self.dim), d(self.dt)
        self.d_fields = [d(f) for f in self.fields]
        self.xb = torch.zeros((self.N, 12), dtype=torch.float32, device="cuda")
        self.clock = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.rec = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.ring = torch.zeros((2, self.N, 2), dtype=torch.float32, device="cuda")
        self.ustar = torch.full((self.N + 1, 2), 7.0, device="cuda")
        self.dt_eff = torch.full((self.B + 1,), 7.0, device="cuda")
        self.ref = R.LaunchRule(self.batch, self.dim, self.dt, scheme)

    def write_rec(self):
        self.rec.copy_(torch.from_numpy(self.ref.rec.copy()))

    def launch(self, clock):
        from gfv import lib as L
        self.xb.copy_(self.d_fields[clock])
        self.clock.fill_(clock)
        self.write_rec()
        L.check(L.load().gfv_time_scheme_update(
            self.xb.data_ptr(), self.d_batch.data_ptr(), self.d_dim.data_ptr(), self.d_dt.data_ptr(), self.N, self.B,
            self.clock.data_ptr(), self.rec.data_ptr(), self.ring.data_ptr(), self.ustar.data_ptr(), self.dt_eff.data_ptr(),
            L.stream_ptr()), "gfv_time_scheme_update")
        torch.cuda.synchronize()
        active = self.ref.launch(self.fields[clock], clock)
        what = (self.N, clock, active)
        assert _same(self.ring, self.ref.ring), what
        assert _same(self.ustar[:self.N], self.ref.ustar), what
        assert _same(self.dt_eff[:self.B], self.ref.dt_eff), what
        assert bool((self.ustar[self.N] == 7.0).all()) and float(self.dt_eff[self.B]) == 7.0, what
        assert _same(self.xb, self.fields[clock]) and self.rec.cpu().tolist() == self.ref.rec.tolist(), what     # read-only
        return active


@pytest.mark.parametrize("sizes", [(190, 29), (200, 57)], ids=["N219", "N257"])
def test_the_kernel_alone_against_the_numpy_rule_bit_for_bit(sizes):
    """N = 219 (no multiple of 64 or 256; the row counts of tests/test_march_gpu.py's stand-alone case) and N = 257 (one full
    workgroup and one row), B = 2: ring, ustar and dt_eff after every launch of the clock sequence 0, 0, 1, 1, 1, 2, 3 from a
    start without history, a reset in the middle of a run, the start with `previous=`, and "bdf1"."""
    k = _Kernel(sizes, R.BDF2, seed=3)
    k.ref.reset(0)
    assert [k.launch(c) for c in CLOCKS] == [False, False, True, True, True, True, True]
    assert not _same(k.dt_eff[:k.B], k.dt)
    k.ref.reset(3)                                       # history forgotten at clock 3: first order again, then second
    assert not k.launch(3) and _same(k.dt_eff[:k.B], k.dt)
    k = _Kernel(sizes, R.BDF2, seed=4)
    k.ref.install_previous(k.previous, 0)
    k.ring.copy_(torch.from_numpy(k.ref.ring))
    assert [k.launch(c) for c in CLOCKS] == [True] * len(CLOCKS)
    k = _Kernel(sizes, R.BDF1, seed=5)
    k.ref.reset(0)
    assert [k.launch(c) for c in CLOCKS] == [False] * len(CLOCKS)


# ---- 2. the section with a scheme against float64 --------------------------------------------------------------------------------
MESHES = ("poly", "cyl_cavity_b2")
VARIANTS = ("conserved-fused", "conserved-unfused", "non-conserved")


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(mesh):
    from gfv import plan
    c = _Case()
    c.graphs = F.distinct_coefficients(_cpu_graphs(mesh), SEED_COEF)
    c.dev_graphs = tuple(g.clone().to("cuda") for g in c.graphs)
    c.plan = plan.build_plan(*c.dev_graphs)
    c.N = c.graphs[0].x.shape[0]
    c.dec, c.uv_old = F.draw_dec(c.N, SEED_DEC), F.uv_old_of(c.graphs)
    c.dt = c.graphs[4].dt_graph.reshape(-1).to(torch.float32)
    c.uv_star, c.dt_eff = R.draw_baseline(c.uv_old, c.dt, SEED_STAR)
    c.dec_d, c.uv_old_d, c.uv_star_d, c.dt_eff_d = c.dec.cuda(), c.uv_old.cuda(), c.uv_star.cuda(), c.dt_eff.cuda()
    c.G64, c.G32 = F.graph_tensors(c.graphs), F.graph_tensors(c.graphs, torch.float32)
    return c


@functools.lru_cache(maxsize=None)
def _reference(mesh, conserved, integrator):
    """float64 stages with the baseline and the step, and the float32 oracle's own column errors against them."""
    c = _case(mesh)
    ref = F.detached(R.stages_ts(c.dec.double(), c.uv_old.double(), c.uv_star.double(), c.dt_eff.double(), c.G64, conserved,
                                 integrator))
    o32 = F.detached(R.stages_ts(c.dec, c.uv_old, c.uv_star, c.dt_eff, c.G32, conserved, integrator))
    return ref, F.column_errors(o32, ref, c.G64)


@functools.lru_cache(maxsize=None)
def _reference_gradients(mesh, conserved, integrator):
    c = _case(mesh)
    ref = R.one_hot_gradients_ts(c.dec.double(), c.uv_old.double(), c.uv_star.double(), c.dt_eff.double(), c.G64, conserved,
                                 integrator)
    o32 = R.one_hot_gradients_ts(c.dec, c.uv_old, c.uv_star, c.dt_eff, c.G32, conserved, integrator)
    return ref, F.gradient_errors(o32, ref, c.G64)


def _engine(variant, integrator):
    from gfv.engine import Engine
    e = Engine(integrator=integrator, ncn_smooth=True, conserved_form=variant != "non-conserved", order="2nd")
    e._fvm_fuse = variant != "conserved-unfused"
    return e


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in d.items() if v is not None}


@pytest.mark.parametrize("integrator", F.MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_the_section_with_a_scheme_against_float64(mesh, variant, integrator):
    """Engine.fvm_fwd(..., time_state=(uv_star, dt_eff)) and fvm_bwd on meshes with distinct coefficients, a baseline that is not
    uv_old and a step that is not dt: every stage the call returns, column by column, and every one-hot gradient."""
    conserved = variant != "non-conserved"
    c = _case(mesh)
    ref, yard = _reference(mesh, conserved, integrator)
    eng = _engine(variant, integrator)
    losses, uvp_node, uvp_cell, sv = eng.fvm_fwd(c.dec_d, c.uv_old_d, c.plan, time_state=(c.uv_star_d, c.dt_eff_d))
    got = {k: sv[k] for k in ("phi", "grad", "Ff", "phic", "cres", "sums", "gradc")}
    got.update(losses=losses, uvp_node=uvp_node, uvp_cell=uvp_cell)
    got = _cpu(got)
    assert ("gradc" in got) == (not conserved)
    assert _same(got["phi"][:, 5:7], c.uv_star) and bool((got["phi"][:, 7] == 0).all())
    names = set(got)
    err = F.column_errors(got, ref, c.G64)
    assert set(err) == names, names ^ set(err)
    tol = F.tolerance(yard)
    fe, fy = F.family_max(err), F.family_max(yard)
    print(f"stages {mesh} {variant} {integrator}: " + ", ".join(f"{k} {fe[k]:.1e} (oracle32 {fy[k]:.1e})" for k in fe))
    bad = F.failures(err, {k: tol[k] for k in err})
    assert not bad, bad
    # the adjoint, one loss of one graph at a time
    gref, gyard = _reference_gradients(mesh, conserved, integrator)
    B = c.plan.B
    grads = {}
    for b in range(B):
        for l in range(4):
            gloss = torch.zeros(B, 4, device="cuda")
            gloss[b, l] = 1.0
            grads[(b, l)] = eng.fvm_bwd(sv, gloss, c.plan)
    grads = _cpu(grads)
    for key in set(grads) - set(gref):
        assert key[1] == 3 and bool((grads[key] == 0).all()), key
    assert len(gref) >= 4 * B - B
    gerr = F.gradient_errors({k: grads[k] for k in gref}, gref, c.G64)
    print(f"adjoint {mesh} {variant} {integrator}: {max(float(e.max()) for e in gerr.values()):.1e} "
          f"(oracle32 {max(float(e.max()) for e in gyard.values()):.1e})")
    bad = F.failures(gerr, F.tolerance(gyard))
    assert not bad, bad


@pytest.mark.parametrize("integrator", F.MODES)
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
@pytest.mark.parametrize("mesh", MESHES)
def test_the_inputs_can_tell_the_scheme_from_its_absence(mesh, conserved, integrator):
    """A reference evaluated with uv_star := uv_old, and one with dt_eff := dt, each move the momentum columns of cres by more
    than 100 x the tolerance, for every graph: a section that ignored the baseline or the step would fail the test above."""
    c = _case(mesh)
    ref, yard = _reference(mesh, conserved, integrator)
    tol = F.tolerance(yard)["cres"][:, 1:3]
    d = lambda t: t.double()
    for what, star, step in (("uv_star := uv_old", c.uv_old, c.dt_eff), ("dt_eff := dt", c.uv_star, c.dt)):
        wrong = F.detached(R.stages_ts(d(c.dec), d(c.uv_old), d(star), d(step), c.G64, conserved, integrator))
        e = F.column_errors(wrong, ref, c.G64, names=("cres",))["cres"][:, 1:3]
        print(f"{mesh} {conserved} {integrator} {what}: {float((e / tol).min()):.0f} x the tolerance at the least")
        assert bool((e > 100.0 * tol).all()), (what, (e / tol).tolist())


def test_without_time_state_and_with_a_plain_one_the_section_keeps_its_bits():
    """time_state = (uv_old, dt) gives the bits of the call without the keyword - forward and adjoint, fused and not - and the two
    share a plan without handing each other's gfv_fvm_mesh_t: the cache is keyed by the step's address."""
    c = _case("cyl_cavity_b2")
    gloss = (0.5 + torch.rand(c.plan.B, 4, generator=torch.Generator().manual_seed(41))).cuda()
    dt_copy = c.plan.dt.clone()
    for variant in VARIANTS:
        eng = _engine(variant, "imex")
        outs = []
        for ts in (None, (c.uv_old_d, dt_copy), None, (c.uv_star_d, c.dt_eff_d)):
            losses, node, cell, sv = eng.fvm_fwd(c.dec_d, c.uv_old_d, c.plan, time_state=ts)
            outs.append(_cpu(dict(losses=losses, node=node, cell=cell, cres=sv["cres"], gdec=eng.fvm_bwd(sv, gloss, c.plan))))
        for k in outs[0]:
            assert _same(outs[0][k], outs[1][k]) and _same(outs[0][k], outs[2][k]), (variant, k)
        assert not _same(outs[0]["cres"], outs[3]["cres"]) and not _same(outs[0]["gdec"], outs[3]["gdec"])
    assert _same(c.plan.dt, dt_copy)                                  # plan.dt is never written
    keys = list(c.plan.__dict__["_fvm_mesh_cache"])
    assert len({k[-1] for k in keys}) >= 3                            # the plan's dt, its copy, dt_eff: a struct each


# ---- the state two marches are compared by --------------------------------------------------------------------------------------
def _named(ms, buf):
    """A flat buffer by parameter.  The alignment padding between tensors is not state (TrainStep.named_state;
    tests/test_march_gpu.py `_full_state`): its gradient slots take what a shared workspace held, and an object with a scheme
    allocates differently from one without - the one padding element behind the decoder's three biases then moves differently."""
    return torch.cat([ms.G.view_of(buf, n).reshape(-1) for n in ms.G.off]).cpu()


def _named_state(ms):
    torch.cuda.synchronize()
    return {"p": _named(ms, ms.flat_p), "m": _named(ms, ms.flat_m), "v": _named(ms, ms.flat_v),
            "adam_t": ms.adam_state[0:1].cpu().clone(), "x_backup": ms.x_backup.cpu().clone()}


# ---- 3. nothing changes until history exists ---------------------------------------------------------------------------------------
def _march(mode, scheme, tol=TOL, **kw):
    from gfv.march import MarchStep
    from gfv.timescheme import TimeScheme
    kw.setdefault("model", None)
    model = kw.pop("model") or _model()
    graphs = kw.pop("graphs", None) or _graphs()
    sch = TimeScheme(scheme) if isinstance(scheme, str) else scheme
    return MarchStep(model, graphs, lr=LR, use_graph=mode, tol=tol, max_inner=MAX_INNER, max_levels=8, time_scheme=sch, **kw)


@functools.lru_cache(maxsize=None)
def _plain_march(mode):
    """A march without a scheme: the state after each of three levels, and the rows."""
    ms = _march(mode, None)
    states, rows = [], []
    for _ in range(3):
        rows += ms.run(levels=1, max_ahead=8)
        states.append(_named_state(ms))
    return states, rows


@pytest.mark.parametrize("mode", [False, "list"], ids=["eager", "list"])
def test_nothing_changes_until_history_exists(mode):
    states, rows = _plain_march(mode)
    one = _march(mode, "bdf1")
    got = one.run(levels=3, max_ahead=8)
    _assert_same(_named_state(one), states[2], f"bdf1 {mode}")
    _same_rows(got, rows)
    assert one.time_scheme.read()["order"] == 1
    two = _march(mode, "bdf2")
    assert two.time_scheme.read()["order"] == 1
    got = two.run(levels=1, max_ahead=8)
    _assert_same(_named_state(two), states[0], f"bdf2 level 0 {mode}")
    _same_rows(got, rows[:1])
    read = two.time_scheme.read()
    assert (read["clock"], read["order"]) == (1, 2)
    two.run(levels=1, max_ahead=8)
    assert not _same(_named_state(two)["x_backup"], states[1]["x_backup"])


# ---- 4. device-decided equals host-driven ------------------------------------------------------------------------------------------
def _scheme_state(sch):
    torch.cuda.synchronize()
    return {"ring": sch.ring.cpu().clone(), "ustar": sch.ustar.cpu().clone(), "dt_eff": sch.dt_eff.cpu().clone()}


@functools.lru_cache(maxsize=None)
def _fixed_march():
    ms = _march("list", "bdf2", tol=None, keep=3)
    rows = ms.run(levels=3)
    assert [(r["inner"], r["capped"]) for r in rows] == [(MAX_INNER, True)] * 3
    return ms, _named_state(ms), _scheme_state(ms.time_scheme)


@pytest.mark.parametrize("mode", [False, "list", True], ids=["eager", "list", "hipgraph"])
def test_the_device_decided_march_equals_the_host_driven_loop(mode):
    from gfv.timescheme import TimeScheme
    from gfv.trainer import TrainStep
    ms, want, want_sch = _fixed_march()
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=mode, time_scheme=TimeScheme("bdf2"))
    for _ in range(3):
        for _ in range(MAX_INNER):
            ts.step()
        ts.advance_time()
    _assert_same(_named_state(ts), want, f"host-driven {mode}")
    _assert_same(_scheme_state(ts.time_scheme), want_sch, f"host-driven {mode} scheme")
    pl = ms.plan
    batch, dim, dt = pl.batch.cpu().numpy(), pl.uvp_dim.cpu().numpy(), pl.dt.cpu().numpy().astype(f32)
    ustar = R.ustar_of(ms.snapshot(2).cpu().numpy(), ms.snapshot(1).cpu().numpy(), batch, dim)
    for sch in (ms.time_scheme, ts.time_scheme):
        read = sch.read()
        assert (read["clock"], read["order"]) == (3, 2)
        assert _same(read["ustar"], ustar)
        assert _same(read["dt_eff"], dt / f32(1.5)) and not _same(read["dt_eff"], dt)
        assert _same(read["previous"], ms.snapshot(1)[:, 0:2])
    assert _same(pl.dt, dt)


# ---- 5. run-ahead, held steps, reset, resume ---------------------------------------------------------------------------------------
def test_run_ahead_and_held_steps_leave_the_same_bits():
    outs = []
    for ahead in (0, 32):
        ms = _march("list", "bdf2")
        ms.run(levels=3, max_ahead=ahead)
        outs.append((_named_state(ms), _scheme_state(ms.time_scheme), ms.stats()))
    assert outs[0][2]["held"] == 0
    _assert_same(outs[0][0], outs[1][0], "run-ahead")
    _assert_same(outs[0][1], outs[1][1], "run-ahead scheme")
    print("held with max_ahead=32:", outs[1][2]["held"])
    # steps issued past the target change neither ring nor ustar (ms: the max_ahead=32 object, at its target)
    before, sch_before, held = _named_state(ms), _scheme_state(ms.time_scheme), ms.stats()["held"]
    for _ in range(3):
        ms.step()
    assert ms.stats()["held"] == held + 3
    _assert_same(_named_state(ms), before, "held")
    _assert_same(_scheme_state(ms.time_scheme), sch_before, "held scheme")


def _carry_over(first, scheme):
    """A new object on the field, the model and the optimiser state of `first` (the field is the caller's to carry over)."""
    torch.cuda.synchronize()
    model = _model()
    model.load_state_dict(first.model.state_dict())
    graphs = _graphs()
    graphs[0].x.copy_(first.x_backup)
    return _march("list", scheme, model=model, graphs=graphs)


def test_reset_makes_the_next_level_first_order_again():
    ms = _march("list", "bdf2")
    ms.run(levels=2, max_ahead=8)
    assert ms.time_scheme.read()["order"] == 2
    ms.reset()
    read = ms.time_scheme.read()
    assert (read["clock"], read["order"], read["previous"]) == (0, 1, None)
    uv_old = (ms.x_backup[:, 0:2] / ms.plan.uvp_dim[ms.plan.batch.long()][:, 0:2]).cpu()
    assert _same(read["ustar"], uv_old) and _same(read["dt_eff"], ms.plan.dt)
    sd = ms.state_dict()
    assert sd["gfv_time_scheme"] == {"scheme": "bdf2", "has_previous": False, "previous": None}
    # a fresh object without a scheme on the same field, model and optimiser state: its level 0 is backward Euler
    fresh = _carry_over(ms, None)
    fresh.load_state_dict(sd)
    assert fresh.time_scheme is None and "gfv_time_scheme" not in fresh.state_dict()
    rows, want = ms.run(levels=1, max_ahead=8), fresh.run(levels=1, max_ahead=8)
    _same_rows(rows, want)
    _assert_same(_named_state(ms), _named_state(fresh), "level 0 after reset()")


def test_a_resumed_march_continues_at_second_order():
    whole = _march("list", "bdf2")
    whole.run(levels=4, max_ahead=8)
    first = _march("list", "bdf2")
    first.run(levels=2, max_ahead=8)
    sd = first.state_dict()
    saved = sd["gfv_time_scheme"]
    assert saved["scheme"] == "bdf2" and saved["has_previous"] and not saved["previous"].is_cuda
    assert tuple(saved["previous"].shape) == (first.plan.N, 2)
    second = _carry_over(first, "bdf2")
    assert second.time_scheme.read()["order"] == 1
    second.load_state_dict(sd)
    read = second.time_scheme.read()
    assert (read["clock"], read["order"]) == (0, 2) and _same(read["previous"], saved["previous"])
    _assert_same({k: v for k, v in _scheme_state(second.time_scheme).items() if k != "ring"},
                 {k: v for k, v in _scheme_state(first.time_scheme).items() if k != "ring"}, "installed")
    installed = _scheme_state(second.time_scheme)
    # ... which `previous=` at construction does too, and a dict of another scheme is refused
    from gfv.timescheme import TimeScheme
    third = _carry_over(first, TimeScheme("bdf2", previous=saved["previous"].cuda()))
    assert third.time_scheme.read()["order"] == 2
    _assert_same(_scheme_state(third.time_scheme), installed, "previous=")
    with pytest.raises(ValueError, match="does not load into"):
        _carry_over(first, "bdf1").load_state_dict(sd)
    second.run(levels=2, max_ahead=8)
    _assert_same(_named_state(second), _named_state(whole), "resumed")


# ---- 6. together with time_bc and field_stats -----------------------------------------------------------------------------------------
def test_with_time_bc_and_field_stats_the_order_of_the_launches_does_not_matter():
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.march import MarchStep
    from gfv.timescheme import TimeScheme

    class Reversed(MarchStep):
        def _follow_level(self):
            self.time_scheme.launch()
            self.time_bc.launch()
            self.field_stats.launch()

    outs = []
    for cls in (MarchStep, Reversed):
        tbc, fs, sch = T.TimeBC(velocity=T.Ramp(0.5, 1.25, 0.0, 2.0, "smooth")), FieldStats(start=1), TimeScheme("bdf2")
        ms = cls(_model(), _graphs(), lr=LR, use_graph="list", tol=TOL, max_inner=MAX_INNER, max_levels=8, time_bc=tbc,
                 field_stats=fs, time_scheme=sch)
        ms.run(levels=2, max_ahead=8)
        state = _named_state(ms)
        state.update(_scheme_state(sch))
        rec, sums, aux = fs.raw()
        state.update(y=ms.plan.y.cpu().clone(), hist=tbc.hist.cpu().clone(), fs_rec=rec, fs_sums=sums, fs_aux=aux)
        outs.append(state)
        assert int(rec[4]) == 2 and sch.read()["order"] == 2
    _assert_same(outs[0], outs[1], "order of the followers")
    assert len({float(v) for v in tbc.read()["velocity"][:, 0]}) == 3                # (the boundary data moved with the levels)


# ---- 7. refusals that need the device ------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_device():
    from gfv import meshgen
    from gfv.pool import DevicePool
    from gfv.pool_trainer import PoolTrainStep
    from gfv.timescheme import TimeScheme
    from gfv.trainer import TrainStep
    sch = TimeScheme("bdf2")
    ts = TrainStep(_model(), _graphs(), lr=LR, time_scheme=sch)
    assert ts.time_scheme is sch and sch.read()["clock"] == 0
    with pytest.raises(ValueError, match="history belongs to the nodes of ONE batch"):
        ts.set_batch(_graphs())
    with pytest.raises(ValueError, match="already attached to a TrainStep"):
        _march(False, sch)
    with pytest.raises(ValueError, match="already attached to a TrainStep"):
        TrainStep(_model(), _graphs(), lr=LR, time_scheme=sch)
    ms = _march(False, "bdf2")
    with pytest.raises(RuntimeError, match="the device advances it"):
        ms.time_scheme.tick()
    N = ts.plan.N
    for bad in (torch.zeros(N + 1, 2, device="cuda"), torch.zeros(N - 1, 3, device="cuda")):
        with pytest.raises(ValueError, match=f"previous must be a \\[{N}, >= 2\\] tensor"):
            TrainStep(_model(), _graphs(), lr=LR, time_scheme=TimeScheme("bdf2", previous=bad))
        with pytest.raises(ValueError, match="previous must be a"):
            sch.install_previous(bad)
    m = meshgen.finish_mesh(meshgen.raw_quad_cavity(n=6, jitter=0.1, tri_fraction=0.0, seed=13), U=1.0)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=3)])
    with pytest.raises(ValueError, match="the pool owns the fields"):
        PoolTrainStep(_model(), pool, max_graphs=1, lr=LR, time_scheme=TimeScheme("bdf2"))
    # a scheme an attach refused stays free
    free = TimeScheme("bdf2", previous=torch.zeros(N + 1, 2, device="cuda"))
    with pytest.raises(ValueError):
        TrainStep(_model(), _graphs(), lr=LR, time_scheme=free)
    free.check_free()
