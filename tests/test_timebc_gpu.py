"""Unsteady boundary data on the device (gfv/timebc.py, csrc/timebc.hip; include/gfv.h gfv_time_bc_update).

1. the kernel alone against tests/timebc_ref.py: Const, Ramp (both shapes) and Table (clamped and periodic) bit for bit - y,
   theta[:, 5], feature column 8, the history row - and rows outside the mask and channels that are off untouched (sentinels);
   Sine within the measured distance of the device's `sin` from numpy's;
2. the `Rollout` hook-up is a host that copies `evaluate(clock)` in before every step, bit for bit, in both launch modes;
3. `set()` under a recorded list, and `reset()`;      4. `MarchStep` with levels the host can count;
5. `MarchStep` with levels only the device can count;   6. the `state_dict` round trip;
7. `time_bc=None` is the step it was;                  8. refusals that need the device.

The Sine bound.  SINE_MEASURED is max |g_dev - g_ref| / |amp| over this file's arguments (four clocks, three dt, six waveforms:
arguments of sin between 0 and 5.2e3, |mean| at most 4 |amp| - the sum mean + amp sin rounds to a spacing of g, so the
figure relative to |amp| grows with |mean| / |amp|), measured on the MI355X against numpy: test 1 prints it.  The test asserts 4 x that value (the
margin covers other arguments in the same range) and that the bound stays below 2^-40, which guarantees that y differs from
float32(reference) by at most one float32 spacing of (|mean| + |amp|) |y0| - asserted as well."""
import functools

import numpy as np
import pytest
import torch

import cases
import timebc_ref as R
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
SINE_MEASURED = 2.0 ** -53          # measured on the MI355X; the test prints the value it finds
SINE_BOUND = 4.0 * SINE_MEASURED
SENTINEL = 12345.678


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
DT = np.array([0.1, 0.25, 0.013], dtype=f32)
CLOCKS = (1, 2, 7, 1000)


def _exact_waves():
    from gfv import timebc as T
    return [T.Const(0.75), T.Ramp(0.0, 1.5, 0.05, 150.0), T.Ramp(2.0, -1.0, 0.2, 1.7, "smooth"),
            T.Table([0.05, 0.2, 0.3, 1.75, 20.0, 300.0], [1.0, -0.5, 0.25, 3.0, 1.0 / 3.0, 2.0]),
            T.Table([0.0, 0.1, 0.7, 1.3], [0.1, 1.1, -0.7, 0.3], periodic=True)]


def _sine_waves():
    from gfv import timebc as T
    return [T.Sine(1.0, 0.3, 0.2), T.Sine(0.0, 1.0, 3.3, phase=0.4), T.Sine(-2.0, 0.5, 0.05, start=0.15),
            T.Sine(0.5, 2.0, 1.0, phase=-1.0), T.Sine(1.0, 0.5, 0.0, phase=2.0), T.Sine(0.0, 1e3, 1.7, start=0.3)]


class _Alone:
    """Made-up buffers of N rows and B graphs, and one launch of the kernel on them."""

    def __init__(self, N, B, seed):
        from gfv import lib as L
        rng = np.random.default_rng(seed)
        self.N, self.B, self.K = N, B, 1001
        self.batch = np.sort(rng.integers(0, B, N)).astype(np.int32)
        self.batch[0] = 0
        self.nt = rng.integers(0, 6, N).astype(np.int32)
        self.nt[0] = 1                                                  # row 0 is an inflow row whatever the draw
        self.y0 = (rng.standard_normal((N, 2)) * 10.0 ** rng.uniform(-2, 2, (N, 2))).astype(f32)
        self.theta0 = rng.uniform(0.5, 2.0, B).astype(f32) * np.where(np.arange(B) % 2 == 0, 1, -1).astype(f32)
        self.dt = DT[:B].copy()
        self.d = dict(batch=_dev(self.batch), nt=_dev(self.nt), y0=_dev(self.y0), theta0=_dev(self.theta0), dt=_dev(self.dt),
                      rec=torch.zeros((B, 2, L.TIME_BC_RECORD), dtype=torch.float64, device="cuda"),
                      tab=torch.zeros((B, 2, 2, L.TIME_BC_TABLE_MAX), dtype=torch.float64, device="cuda"),
                      ctl=torch.zeros(L.TIME_BC_CTL, dtype=torch.int32, device="cuda"),
                      clock=torch.zeros(1, dtype=torch.int32, device="cuda"))

    def set_waves(self, vel, src):
        self.vel, self.src = vel, src
        for b in range(self.B):
            for ch, ws in enumerate((vel, src)):
                if ws is None:
                    continue
                rec, times, values = ws[b].pack()
                self.d["rec"][b, ch].copy_(torch.tensor(rec, dtype=torch.float64))
                if times is not None:
                    self.d["tab"][b, ch, 0, :len(times)].copy_(torch.tensor(times, dtype=torch.float64))
                    self.d["tab"][b, ch, 1, :len(times)].copy_(torch.tensor(values, dtype=torch.float64))

    def launch(self, clock, nodes, offset=0):
        """-> (device results, reference results) of one launch on sentinel-filled outputs."""
        from gfv import lib as L
        d, N, B = self.d, self.N, self.B
        y = torch.full((N, 2), SENTINEL, dtype=torch.float32, device="cuda")
        theta = torch.full((B, 9), SENTINEL, dtype=torch.float32, device="cuda")
        xb = torch.full((N, 12), SENTINEL, dtype=torch.float32, device="cuda")
        x = torch.full((N, 12), SENTINEL, dtype=torch.float32, device="cuda")
        hist = torch.full((self.K, B, 3), SENTINEL, dtype=torch.float64, device="cuda")
        d["clock"].copy_(torch.tensor([clock - 1 - offset], dtype=torch.int32))
        d["ctl"][0:1].copy_(torch.tensor([offset], dtype=torch.int32))
        channels = (1 if self.vel is not None else 0) | (2 if self.src is not None else 0)
        L.check(L.load().gfv_time_bc_update(
            d["clock"].data_ptr(), d["ctl"].data_ptr(), d["rec"].data_ptr(), d["tab"].data_ptr(), d["dt"].data_ptr(),
            d["batch"].data_ptr(), d["nt"].data_ptr(), N, B, d["y0"].data_ptr(), y.data_ptr(), d["theta0"].data_ptr(),
            theta.data_ptr() + 4 * 5, 9, xb.data_ptr(), x.data_ptr(), hist.data_ptr(), self.K, R.type_mask(nodes), channels,
            L.stream_ptr()), "gfv_time_bc_update")
        torch.cuda.synchronize()
        got = dict(y=y.cpu().numpy(), theta=theta.cpu().numpy(), xb=xb.cpu().numpy(), x=x.cpu().numpy(), hist=hist.cpu().numpy())
        want = dict(y=np.full((N, 2), SENTINEL, f32), theta=np.full((B, 9), SENTINEL, f32), xb=np.full((N, 12), SENTINEL, f32),
                    hist=np.full((self.K, B, 3), SENTINEL, f64))
        th5, c8 = want["theta"][:, 5].copy(), want["xb"][:, 8].copy()
        R.launch(clock, self.dt, self.batch, self.nt, self.y0, self.theta0,
                 None if self.vel is None else [R.from_object(w) for w in self.vel],
                 None if self.src is None else [R.from_object(w) for w in self.src], nodes, want["y"], th5, c8, want["hist"])
        want["theta"][:, 5], want["xb"][:, 8] = th5, c8
        want["x"] = want["xb"]
        return got, want


@pytest.mark.parametrize("N", [1, 179, 257, 1000])
def test_the_kernel_alone_is_the_reference_bit_for_bit(N):
    waves = _exact_waves()
    for B in (1, 3):
        k = _Alone(N, B, seed=100 * N + B)
        masked = (k.nt == 1) | (k.nt == 5)
        assert masked.any() and np.abs(k.y0[masked]).min() > 0          # not vacuous: a driven row with a target that is not 0
        for shift in range(len(waves)):
            vel = [waves[(shift + b) % 5] for b in range(B)]
            src = [waves[(shift + b + 2) % 5] for b in range(B)]
            for nodes, v, s in ((("inflow", "in_wall"), vel, src), (("wall",), vel, None), (("inflow", "in_wall", "wall"), None, src)):
                if shift > 1 and v is not vel:
                    continue                                            # (the channel-off cases: two wave sets are enough)
                k.set_waves(v, s)
                for clock in CLOCKS:
                    got, want = k.launch(clock, nodes)
                    for key in ("y", "theta", "xb", "x", "hist"):
                        assert _same(got[key], want[key]), (N, B, shift, nodes, clock, key)
                    # what must stay: rows outside the mask, every column but 5 / 8, every history row but one, a channel that is off
                    m = ((R.type_mask(nodes) >> k.nt) & 1).astype(bool)
                    assert (got["y"][~m] == f32(SENTINEL)).all() and (np.delete(got["xb"], 8, axis=1) == f32(SENTINEL)).all()
                    assert (np.delete(got["theta"], 5, axis=1) == f32(SENTINEL)).all()
                    assert (np.delete(got["hist"], clock - 1, axis=0) == SENTINEL).all()
                    if v is None:
                        assert (got["y"] == f32(SENTINEL)).all() and (got["hist"][clock - 1, :, 1] == 1.0).all()
                    else:
                        assert (got["y"][m] != f32(SENTINEL)).all()
                    if s is None:
                        assert (got["theta"] == f32(SENTINEL)).all() and (got["xb"] == f32(SENTINEL)).all()
                        assert (got["x"] == f32(SENTINEL)).all() and (got["hist"][clock - 1, :, 2] == 1.0).all()
        # the clock offset of a resumed run: counter + 1 + offset is the field
        k.set_waves([waves[b % 5 + 1 if b % 5 < 4 else 0] for b in range(B)], None)
        got, want = k.launch(7, ("inflow",), offset=4)
        assert all(_same(got[key], want[key]) for key in ("y", "theta", "xb", "x", "hist"))


@pytest.mark.parametrize("N", [1, 179, 257, 1000])
def test_the_kernel_alone_sine_within_the_measured_bound(N):
    assert SINE_BOUND <= 2.0 ** -40
    waves = _sine_waves()
    worst, worst_arg = 0.0, 0.0
    for B in (1, 3):
        k = _Alone(N, B, seed=100 * N + B)
        for shift in range(len(waves)):
            vel = [waves[(shift + b) % 6] for b in range(B)]
            src = [waves[(shift + b + 3) % 6] for b in range(B)]
            k.set_waves(vel, src)
            for clock in CLOCKS:
                got, want = k.launch(clock, ("inflow", "in_wall"))
                row, ref = got["hist"][clock - 1], want["hist"][clock - 1]
                assert _same(row[:, 0], ref[:, 0])                                              # t: exact
                assert (np.delete(got["hist"], clock - 1, axis=0) == SENTINEL).all()
                m = (k.nt == 1) | (k.nt == 5)
                assert (got["y"][~m] == f32(SENTINEL)).all()
                for ch, ws in ((1, vel), (2, src)):
                    for b in range(B):
                        amp = abs(ws[b].amp)
                        err = abs(row[b, ch] - ref[b, ch]) / amp
                        arg = float(R.sine_argument(R.from_object(ws[b]), ref[b, 0]))
                        if err > worst:
                            worst, worst_arg = err, arg
                        assert err <= SINE_BOUND, (N, B, clock, ws[b], err)
                # y against float32(reference): at most one float32 spacing of (|mean| + |amp|) |y0|
                scale = np.array([abs(w.mean) + abs(w.amp) for w in vel])[k.batch][:, None] * np.abs(k.y0.astype(f64))
                ulp = np.spacing(scale.astype(f32)).astype(f64)
                diff = np.abs(got["y"].astype(f64) - want["y"].astype(f64))
                assert (diff[m] <= ulp[m]).all(), (N, B, clock)
                th_scale = np.array([abs(w.mean) + abs(w.amp) for w in src]) * np.abs(k.theta0.astype(f64))
                assert (np.abs(got["theta"][:, 5].astype(f64) - want["theta"][:, 5].astype(f64)) <= np.spacing(th_scale.astype(f32))).all()
                assert _same(got["xb"][:, 8], got["theta"][k.batch, 5]) and _same(got["x"], got["xb"])
    print(f"sine N={N}: max |g_dev - g_ref| / |amp| = {worst:.3e} = 2^{np.log2(worst) if worst else -np.inf:.2f} (argument {worst_arg:.4g})")


# ---- the model and the graphs ----------------------------------------------------------------------------------------------------
def _model():
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    m = NNmodel(default_params(dataset_size=1))
    sd = m.state_dict()
    for k, v in O.init_parameters(cases.WEIGHT_SEED).items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


@functools.lru_cache(maxsize=None)
def _cpu_graphs(which):
    """The suites' small inputs with a source coefficient that is not zero (theta_PDE[:, 5] and the node-feature column that holds
    it) and - cyl_cavity_b2 - the cavity's WALL rows given a target that is not zero (its lid is of type INFLOW: the "wall" mask
    would drive rows that are all zero)."""
    if which == "poly":
        from test_config5_gpu import _small_polygon_graphs
        graphs = _small_polygon_graphs()
    else:
        graphs = cases.make_graphs(which)
    gn, gi = graphs[0], graphs[4]
    B = gi.theta_PDE.shape[0]
    gi.theta_PDE[:, 5] = torch.tensor([0.3, -0.2][:B], dtype=gi.theta_PDE.dtype)
    gn.x[:, 8] = gi.theta_PDE[gn.batch, 5].to(gn.x.dtype)
    if which == "cyl_cavity_b2":
        wall1 = (gn.node_type.reshape(-1) == 3) & (gn.batch == 1)
        assert int(wall1.sum()) > 0
        gn.y[wall1, 0] = 0.125
    return graphs


def _graphs(which, rollout=True):
    hg = tuple(g.clone().to("cuda") for g in _cpu_graphs(which))
    if rollout:
        hg[0].norm_uvp, hg[0].norm_global = True, True
    return hg


def _assert_driven(plan, tbc):
    """At least one masked row per graph with a target that is not zero, and a source coefficient that is not zero."""
    nt, batch = plan.node_type.cpu().numpy(), plan.batch.cpu().numpy()
    m = ((tbc.type_mask >> nt) & 1).astype(bool)
    y0 = tbc.y0.cpu().numpy()
    for b in range(plan.B):
        assert (np.abs(y0[m & (batch == b)]).max(axis=1) > 0).any(), b
    assert (tbc.theta0.cpu().numpy() != 0).all()


def _copy_in(owner, y, th):
    """What a host must do per step without TimeBC: the targets, the coefficient, and its feature column in x_backup and x."""
    pl = owner.plan
    pl.y.copy_(y)
    pl.theta[:, 5].copy_(th)
    col = th[pl.batch.long()]
    owner.x_backup[:, 8].copy_(col)
    owner.x[:, 8].copy_(col)


# ---- 2. the Rollout hook-up ------------------------------------------------------------------------------------------------------
STEPS = 12


def _b2_waves():
    from gfv import timebc as T
    return dict(velocity=[T.Sine(1.0, 0.3, 0.2), T.Ramp(0.0, 1.0, 0.0, 0.55, "smooth")],
                source=[T.Ramp(1.0, -1.0, 0.05, 0.3), T.Table([0.0, 0.3, 0.5], [1.0, 2.0, 0.5], periodic=True)],
                nodes=("inflow", "in_wall", "wall"))


def _snap(r, outs):
    torch.cuda.synchronize()
    pl = r.plan
    return {"x_backup": r.x_backup.cpu().clone(), "x": r.x.cpu().clone(), "y": pl.y.cpu().clone(), "theta": pl.theta.cpu().clone(),
            "losses": outs[0].cpu().clone(), "uvp_node": outs[1].cpu().clone(), "uvp_cell": outs[2].cpu().clone()}


@functools.lru_cache(maxsize=None)
def _rollout_with(mode):
    from gfv.rollout import Rollout
    from gfv.timebc import TimeBC
    tbc = TimeBC(**_b2_waves())
    r = Rollout(_model(), _graphs("cyl_cavity_b2"), max_steps=STEPS, launch_mode=mode, time_bc=tbc)
    assert r.time_bc is tbc
    _assert_driven(r.plan, tbc)
    snaps = []
    for _ in range(STEPS):
        snaps.append(_snap(r, r.step()))
    if mode == "cmd_list":
        st = r._lists.stats()
        assert st["recorded"] == 1 and st["replayed"] >= 6 and st["eager"] >= 2, st
    return r, tbc, snaps, r.history.cpu().clone(), tbc.read()


@functools.lru_cache(maxsize=None)
def _rollout_by_hand():
    """An eager Rollout WITHOUT time_bc; the test copies evaluate(clock) in before each step."""
    from gfv.rollout import Rollout
    _, tbc, *_ = _rollout_with("eager")
    r = Rollout(_model(), _graphs("cyl_cavity_b2"), max_steps=STEPS, launch_mode="eager")
    assert r.time_bc is None
    snaps = []
    _copy_in(r, *tbc.evaluate(1))
    for k in range(1, STEPS + 1):
        outs = r.step()
        _copy_in(r, *tbc.evaluate(k + 1))             # (in place for the next step: where the launch behind the advance leaves it)
        snaps.append(_snap(r, outs))
    return snaps, r.history.cpu().clone()


@pytest.mark.parametrize("mode", ["cmd_list", "eager"])
def test_rollout_is_a_host_that_copies_evaluate_in_before_every_step(mode):
    _, tbc, snaps, history, read = _rollout_with(mode)
    want_snaps, want_history = _rollout_by_hand()
    assert _same(history, want_history)
    for k, (a, b) in enumerate(zip(snaps, want_snaps)):
        for key in a:
            assert _same(a[key], b[key]), (mode, k + 1, key)
    # the run moved: the driven rows and the coefficient differ between steps
    assert not _same(snaps[0]["y"], snaps[5]["y"]) and not _same(snaps[0]["theta"], snaps[5]["theta"])
    # read(): clocks 1 .. STEPS + 1 (the data of the next field are in place), against the reference
    w = _b2_waves()
    dt = tbc._plan.dt.cpu().numpy()
    t, gv, gs = R.rows(range(1, STEPS + 2), dt, [R.from_object(v) for v in w["velocity"]], [R.from_object(v) for v in w["source"]])
    assert read["clock"].tolist() == list(range(1, STEPS + 2))
    assert _same(read["t"], t) and _same(read["source"], gs) and _same(read["velocity"][:, 1], gv[:, 1])
    assert (np.abs(read["velocity"][:, 0].numpy() - gv[:, 0]) <= SINE_BOUND * 0.3).all()         # graph 0: the Sine
    assert read["t"].dtype == torch.float64 and not read["t"].is_cuda


def test_both_launch_modes_give_the_same_bits():
    a, b = _rollout_with("cmd_list"), _rollout_with("eager")
    assert _same(a[3], b[3]) and all(_same(a[4][k], b[4][k]) for k in a[4])
    assert all(_same(u[key], v[key]) for u, v in zip(a[2], b[2]) for key in u)


# ---- 3. set() under a recorded list, reset() -------------------------------------------------------------------------------------
def test_set_holds_from_the_next_step_without_a_new_recording_and_reset_starts_over():
    from gfv import timebc as T
    from gfv.rollout import Rollout
    first = T.Sine(1.0, 0.3, 0.2)
    tbc = T.TimeBC(velocity=[T.Const(1.0), first], nodes=("inflow",))
    r = Rollout(_model(), _graphs("cyl_cavity_b2"), max_steps=STEPS, time_bc=tbc)
    _assert_driven(r.plan, tbc)
    dt = r.plan.dt.cpu().numpy()
    for _ in range(5):
        r.step()
    st = r._lists.stats()
    assert st["recorded"] == 1 and st["replayed"] >= 1
    second = T.Sine(1.0, 0.3, 0.7)
    tbc.set(velocity=second, graph=1)                                    # steps 1 .. 5 ran under `first`; step 6 runs under `second`
    assert tbc.waveforms(1) == (second, None) and tbc.waveforms(0) == (T.Const(1.0), None)
    for _ in range(3):
        r.step()
    assert r._lists.stats()["recorded"] == 1 and r._lists.stats()["replayed"] == st["replayed"] + 3
    read = tbc.read()
    assert read["clock"].tolist() == list(range(1, 10))
    _, old, _ = R.rows(range(1, 6), dt, [R.const(1.0), R.from_object(first)], None)
    _, new, _ = R.rows(range(6, 10), dt, [R.const(1.0), R.from_object(second)], None)
    want = np.concatenate([old, new])
    assert _same(read["velocity"][:, 0], want[:, 0]) and (read["source"] == 1.0).all()
    assert (np.abs(read["velocity"][:, 1].numpy() - want[:, 1]) <= SINE_BOUND * 0.3).all()
    assert np.abs(new[0, 1] - R.wave(R.from_object(first), f64(6) * f64(dt[1]))) > 1e-3          # the change is one a test can see
    assert _same(r.plan.y, tbc.evaluate(9)[0])
    with pytest.raises(ValueError, match="built as None"):
        tbc.set(source=T.Const(2.0))
    with pytest.raises(ValueError, match="waveforms for a batch"):
        tbc.set(velocity=[T.Const()] * 3)
    with pytest.raises(IndexError):
        tbc.set(velocity=T.Const(), graph=2)
    # reset(): the owner's - the boundary data of step 1 again, the waveforms as they stand
    r.reset()
    read = tbc.read()
    assert read["clock"].tolist() == [1] and _same(r.plan.y, tbc.evaluate(1)[0])
    r.step()
    assert tbc.read()["clock"].tolist() == [1, 2] and _same(r.plan.y, tbc.evaluate(2)[0])
    assert r._lists.stats()["recorded"] == 1


# ---- 4. - 6. MarchStep -------------------------------------------------------------------------------------------------------------
LR, TOL, MAX_INNER, LEVELS = 5e-5, 0.96758, 5, 3      # the constants of tests/test_march_gpu.py (its docstring derives TOL)


def _poly_bc():
    from gfv import timebc as T
    return T.TimeBC(velocity=T.Ramp(0.5, 1.25, 0.0, 2.0, "smooth"), source=T.Table([0.0, 1.0, 1.5], [1.0, 0.25, 2.0]))


def _march_state(ts):
    torch.cuda.synchronize()
    return {"flat_p": ts.flat_p.cpu().clone(), "flat_m": ts.flat_m.cpu().clone(), "flat_v": ts.flat_v.cpu().clone(),
            "adam_t": ts.adam_state[0:1].cpu().clone(), "x_backup": ts.x_backup.cpu().clone(), "y": ts.plan.y.cpu().clone(),
            "theta": ts.plan.theta.cpu().clone()}


def _same_rows(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert _same(ra[k], rb[k]) if isinstance(ra[k], torch.Tensor) else ra[k] == rb[k], k


def _march(tol, time_bc, **kw):
    import test_march_gpu as TM
    from gfv.march import MarchStep
    assert (TM.LR, TM.TOL, TM.MAX_INNER, TM.LEVELS) == (LR, TOL, MAX_INNER, LEVELS)
    graphs = kw.pop("graphs", None) or _graphs("poly", rollout=False)
    model = kw.pop("model", None) or _model()
    return MarchStep(model, graphs, lr=LR, use_graph="list", tol=tol, max_inner=MAX_INNER, max_levels=8, time_bc=time_bc, **kw)


@functools.lru_cache(maxsize=None)
def _whole_march():
    """Three levels of MAX_INNER iterations each (tol=None: the host knows where the levels end), uninterrupted."""
    tbc = _poly_bc()
    ms = _march(None, tbc)
    assert ms.plan.N == 179
    _assert_driven(ms.plan, tbc)
    rows = ms.run(levels=LEVELS, max_ahead=0)
    return ms, tbc, rows, _march_state(ms)


def test_march_with_levels_the_host_can_count_is_a_host_that_copies_evaluate_in():
    _, tbc, rows, state = _whole_march()
    assert [r["inner"] for r in rows] == [MAX_INNER] * LEVELS and all(r["capped"] for r in rows)
    plain = _march(None, None)
    assert plain.time_bc is None
    plain_rows = []
    for level in range(LEVELS):
        _copy_in(plain, *tbc.evaluate(level + 1))
        plain_rows += plain.run(levels=1, max_ahead=0)
    _copy_in(plain, *tbc.evaluate(LEVELS + 1))            # (where the launch behind the last advance leaves the data)
    want = _march_state(plain)
    for k in state:
        assert _same(state[k], want[k]), k
    _same_rows(rows, plain_rows)
    read = tbc.read()
    dt = plain.plan.dt.cpu().numpy()
    w = _poly_bc()
    t, gv, gs = R.rows(range(1, LEVELS + 2), dt, [R.from_object(w._velocity)], [R.from_object(w._source)])
    assert _same(read["t"], t) and _same(read["velocity"], gv) and _same(read["source"], gs)
    assert len({float(v) for v in gv[:, 0]}) == LEVELS + 1 and len({float(v) for v in gs[:, 0]}) == LEVELS + 1


def test_march_with_levels_only_the_device_can_count():
    tbc = _poly_bc()
    ms = _march(TOL, tbc)
    rows = ms.run(levels=LEVELS, max_ahead=8)
    inner = [r["inner"] for r in rows]
    print("inner iterations per level:", inner, "held:", ms.stats()["held"])
    assert len(set(inner)) > 1                                           # the host could not have known where the levels end
    read = tbc.read()
    dt = ms.plan.dt.cpu().numpy()
    assert read["clock"].tolist() == [1, 2, 3, 4]
    t, gv, gs = R.rows(range(1, LEVELS + 2), dt, [R.from_object(tbc._velocity)], [R.from_object(tbc._source)])
    assert _same(read["t"], t) and _same(read["velocity"], gv) and _same(read["source"], gs)
    assert _same(read["t"][:, 0], np.array([f64(c) * f64(dt[0]) for c in (1, 2, 3, 4)]))
    y, th = tbc.evaluate(ms.level + 1)
    assert ms.level == LEVELS and _same(ms.plan.y, y) and _same(ms.plan.theta[:, 5], th)
    assert _same(ms.x_backup[:, 8], th[ms.plan.batch.long()]) and _same(ms.x[:, 8], ms.x_backup[:, 8])
    # held steps change nothing
    before, hist, held = _march_state(ms), tbc.hist.cpu().clone(), ms.stats()["held"]
    for _ in range(2):
        ms.step()
    assert ms.stats()["held"] == held + 2
    after = _march_state(ms)
    assert all(_same(after[k], before[k]) for k in before) and _same(tbc.hist, hist)
    assert tbc.read()["clock"].tolist() == [1, 2, 3, 4]
    # reset(): level 0's data again
    ms.reset()
    assert tbc.read()["clock"].tolist() == [1] and _same(ms.plan.y, tbc.evaluate(1)[0])


def test_state_dict_round_trip_resumes_the_march_and_its_boundary_data():
    _, _, _, whole = _whole_march()
    first = _march(None, _poly_bc())
    first.run(levels=2, max_ahead=0)
    sd = first.state_dict()
    assert sd["gfv_time_bc"] == {"clock": 2}
    torch.cuda.synchronize()
    model = _model()
    model.load_state_dict(first.model.state_dict())
    graphs = _graphs("poly", rollout=False)
    graphs[0].x.copy_(first.x_backup)                                    # the field is the caller's to carry over
    tbc = _poly_bc()
    second = _march(None, tbc, graphs=graphs, model=model)
    second.load_state_dict(sd)
    assert tbc.clock_offset == 2 and _same(second.plan.y, tbc.evaluate(3)[0])
    rows = second.run(levels=1, max_ahead=0)
    assert [r["inner"] for r in rows] == [MAX_INNER]
    got = _march_state(second)
    # the flat buffers by parameter: the alignment padding between tensors is not state and not part of a state_dict (its
    # gradient slots take what a shared workspace held - TrainStep.named_state, tests/test_march_gpu.py `_full_state`), so the
    # padding the uninterrupted march has stepped on starts from zero again in the new object
    ms = _whole_march()[0]
    for key in ("flat_p", "flat_m", "flat_v"):
        bad = [n for n in ms.G.off if not _same(ms.G.view_of(whole[key], n), second.G.view_of(got[key], n))]
        assert not bad, (key, bad[:4], len(bad))
    for k in ("adam_t", "x_backup", "y", "theta"):
        assert _same(got[k], whole[k]), k
    read = tbc.read()
    assert read["clock"].tolist() == [3, 4]
    assert second.state_dict()["gfv_time_bc"] == {"clock": 3}
    assert "gfv_time_bc" not in _march(None, None).state_dict()


# ---- 7. time_bc=None -----------------------------------------------------------------------------------------------------------------
def test_without_time_bc_the_step_is_the_step_it_was():
    from gfv import timebc as T
    from gfv.rollout import Rollout

    def run(time_bc):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        r = Rollout(_model(), _graphs("poly"), max_steps=6, time_bc=time_bc)
        for _ in range(5):
            outs = r.step()
        st = r._lists.stats()
        assert st["recorded"] == 1 and st["lists"] == 1
        ent = next(iter(r._lists.values()))
        return r, len(ent.cl), _snap(r, outs), r.history.cpu().clone(), torch.cuda.memory_allocated() - before

    plain, n_plain, end_plain, hist_plain, _ = run(None)
    assert plain.time_bc is None and not any(isinstance(v, T.TimeBC) for v in vars(plain).values())
    # Const(1.0) on both channels writes float32(1.0 * base) = base: the same run, one launch longer
    driven, n_driven, end_driven, hist_driven, _ = run(T.TimeBC(velocity=T.Const(1.0), source=T.Const(1.0)))
    assert n_driven == n_plain + 1, (n_plain, n_driven)
    assert _same(hist_plain, hist_driven) and all(_same(end_plain[k], end_driven[k]) for k in end_plain)


def test_march_without_time_bc_records_one_launch_less():
    lens = {}
    for name, tbc in (("plain", None), ("driven", _poly_bc())):
        ms = _march(None, tbc)
        for _ in range(4):
            ms.step()
        (entry,) = ms._lists.values()
        lens[name] = len(entry.cl)
    assert lens["driven"] == lens["plain"] + 1, lens


# ---- 8. refusals that need the device ---------------------------------------------------------------------------------------------
def test_refusals():
    from gfv import timebc as T
    from gfv.march import MarchStep
    from gfv.plan import get_plan
    from gfv.rollout import Rollout
    model = _model()
    tbc = T.TimeBC(velocity=T.Const(2.0))
    with pytest.raises(ValueError, match="anderson"):
        Rollout(model, _graphs("poly"), max_steps=4, anderson=2, time_bc=tbc)
    pooled = _graphs("poly")
    pooled[0]._gfv_pool_plan = get_plan(pooled)                         # what a DevicePool's batches carry
    with pytest.raises(ValueError, match="DevicePool"):
        Rollout(model, pooled, max_steps=4, time_bc=tbc)
    with pytest.raises(ValueError, match="DevicePool"):
        MarchStep(model, pooled, time_bc=tbc)
    with pytest.raises(ValueError, match="max_steps"):
        Rollout(model, _graphs("poly"), max_steps=0, time_bc=tbc)
    with pytest.raises(ValueError, match="2 waveforms for a batch of 1"):
        Rollout(model, _graphs("poly"), max_steps=4, time_bc=T.TimeBC(source=[T.Const(), T.Const()]))
    tbc.check_free()                                                     # a constructor that raised attached nothing
    r = Rollout(model, _graphs("poly"), max_steps=4, launch_mode="eager", time_bc=tbc)
    with pytest.raises(ValueError, match="already attached to a Rollout"):
        Rollout(model, _graphs("poly"), max_steps=4, time_bc=tbc)
    with pytest.raises(ValueError, match="already attached to a Rollout"):
        MarchStep(_model(), _graphs("poly", rollout=False), time_bc=tbc)
    assert not any(v is r for v in vars(tbc).values())                   # no strong reference back to the owner
    # attach() wrote field 1's data: twice the base on the inflow rows, every other row as it was
    y0, y = tbc.y0.cpu().numpy(), r.plan.y.cpu().numpy()
    nt = r.plan.node_type.cpu().numpy()
    m = (nt == 1) | (nt == 5)
    assert m.any() and np.abs(y0[m]).max() > 0
    assert _same(y[m], (2.0 * y0[m].astype(f64)).astype(f32)) and _same(y[~m], y0[~m])
    with pytest.raises(ValueError, match="clock"):
        tbc.evaluate(0)
    # rebase(): a base edited in place is read again
    r.graphs[0].y.mul_(0.5)
    tbc.rebase()
    want = r.graphs[0].y[:, 0:2].to(torch.float32).cpu().numpy()
    if r.plan.y.data_ptr() == r.graphs[0].y.data_ptr():
        want = y * f32(0.5)                                              # (aliased: the caller halved what the launch had written)
    assert _same(tbc.y0, want)
    assert _same(r.plan.y.cpu().numpy()[m], (2.0 * want[m].astype(f64)).astype(f32))
