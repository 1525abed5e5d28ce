"""CPU: the host side of the unsteady boundary data (gfv/timebc.py, csrc/timebc.hip): the reference the GPU tests compare the
kernel with (tests/timebc_ref.py) against closed forms, every refusal, the record packing, and the C ABI: the entry point is
declared, exported and bound, and bad arguments are refused before anything touches a device.  Nothing here touches a GPU.

The closed forms are exact where the arithmetic is: a ramp's ends (s = 0 and s = 1 multiply exactly), the smoothstep's midpoint
(0.25 * 2 = 0.5), a table's knots (the fraction is 0) and the periodic seam (fmod is exact).  `sin` at odd quarter periods is
+-1 to the last bit in numpy; at even ones the argument k pi carries the rounding of pi itself: |sin| <= k * 2^-51."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import cases
import timebc_ref as R
from gfv import timebc as T

f32, f64 = np.float32, np.float64


# ---- the reference against closed forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["linear", "smooth"])
def test_ramp_ends_midpoint_and_clamping(shape):
    w = R.ramp(0.25, 1.75, 1.0, 5.0, shape)
    assert R.wave(w, 1.0) == 0.25 and R.wave(w, 5.0) == 1.75
    assert R.wave(w, -3.0) == 0.25 and R.wave(w, 0.999) == 0.25 and R.wave(w, 5.001) == 1.75 and R.wave(w, 1e9) == 1.75
    assert R.wave(w, 3.0) == 1.0                                       # the midpoint of both shapes: s = 0.5 -> 0.5
    q = R.wave(w, 2.0)                                                 # s = 0.25: linear 0.25, smooth 0.0625 * 2.5 = 0.15625
    assert q == (0.25 + 1.5 * 0.25 if shape == "linear" else 0.25 + 1.5 * 0.15625)
    down = R.ramp(2.0, -1.0, 0.0, 0.5, shape)
    assert R.wave(down, 0.0) == 2.0 and R.wave(down, 0.5) == -1.0 and R.wave(down, 0.25) == 0.5


def test_table_knots_segments_clamping_and_the_periodic_seam():
    times, values = [0.5, 1.0, 2.5, 4.0], [1.0, -2.0, 3.0, 0.5]
    w = R.table(times, values)
    for t, v in zip(times, values):
        assert R.wave(w, t) == v
    assert R.wave(w, 0.0) == 1.0 and R.wave(w, 100.0) == 0.5           # clamped
    assert R.wave(w, 0.75) == -0.5 and R.wave(w, 1.75) == 0.5          # the middle of two segments
    p = R.table(times, values, periodic=True)                          # the period is 3.5, [0.5, 4.0)
    assert R.wave(p, 4.0) == 1.0                                       # the seam itself wraps to the first knot
    assert R.wave(p, 4.0 + 0.25) == R.wave(w, 0.75) and R.wave(p, 0.5 + 3.5 * 3 + 1.25) == R.wave(w, 1.75)
    below = np.nextafter(f64(4.0), f64(0.0))
    assert abs(R.wave(p, below) - 0.5) < 1e-14                         # just below the seam: the last segment's end
    assert R.wave(p, 0.0) == R.wave(w, 3.5) and R.wave(p, 0.25) == R.wave(w, 3.75)     # below the first knot wraps upwards
    assert R.wave(R.table([2.0], [7.0]), 5.0) == 7.0                   # one point: a constant


def test_sine_at_quarter_periods_and_before_its_start():
    w = R.sine(1.0, 0.5, 0.25)                                         # period 4: t = 1 is a quarter
    assert R.wave(w, 0.0) == 1.0 and R.wave(w, 1.0) == 1.5 and R.wave(w, 3.0) == 0.5
    for k, t in ((1, 2.0), (2, 4.0), (5, 10.0)):
        assert abs(R.wave(w, t) - 1.0) <= 0.5 * k * 2.0 ** -51, t
    late = R.sine(1.0, 0.5, 0.25, phase=0.0, start=10.0)
    assert R.wave(late, 3.0) == 1.0 and R.wave(late, 11.0) == 1.5      # at rest until `start`, then the same wave
    ph = R.sine(0.0, 2.0, 0.0, phase=np.pi / 2)                        # freq = 0: the phase alone
    assert R.wave(ph, 123.0) == 2.0
    assert R.wave(R.const(-3.5), 9.0) == -3.5


def test_the_launch_masks_rows_and_keeps_the_rest():
    rng = np.random.default_rng(5)
    N, B = 23, 2
    batch = np.sort(rng.integers(0, B, N)).astype(np.int32)
    nt = rng.integers(0, 6, N).astype(np.int32)
    y0 = rng.standard_normal((N, 2)).astype(f32)
    theta0 = np.array([0.5, -2.0], dtype=f32)
    dt = np.array([0.1, 0.25], dtype=f32)
    vel, src = [R.ramp(0.0, 2.0, 0.0, 1.0), R.const(3.0)], [R.const(0.5), R.ramp(1.0, 0.0, 0.0, 1.0)]
    y, th, c8, hist = np.full((N, 2), 9.0, f32), np.full(B, 9.0, f32), np.full(N, 9.0, f32), np.zeros((4, B, 3))
    t, gv, gs = R.launch(2, dt, batch, nt, y0, theta0, vel, src, ("inflow", "wall"), y, th, c8, hist)
    assert t.tolist() == [2 * f64(f32(0.1)), 0.5] and gv.tolist() == [2.0 * (2 * f64(f32(0.1))), 3.0] and gs.tolist() == [0.5, 0.5]
    m = (nt == 1) | (nt == 3)
    assert m.any() and (~m).any()
    assert (y[~m] == 9.0).all() and np.array_equal(y[m], (gv[batch[m]][:, None] * y0[m].astype(f64)).astype(f32))
    assert th.tolist() == [0.25, -1.0] and np.array_equal(c8, th[batch])
    assert np.array_equal(hist[1], np.stack([t, gv, gs], 1)) and not hist[[0, 2, 3]].any()
    # a channel that is off writes nothing
    y2, th2, c82 = np.full((N, 2), 9.0, f32), np.full(B, 9.0, f32), np.full(N, 9.0, f32)
    R.launch(2, dt, batch, nt, y0, theta0, None, src, ("inflow",), y2, th2, c82)
    assert (y2 == 9.0).all() and np.array_equal(th2, th)
    R.launch(2, dt, batch, nt, y0, theta0, vel, None, ("inflow",), y2, th2 := np.full(B, 9.0, f32), c82 := np.full(N, 9.0, f32))
    assert (th2 == 9.0).all() and (c82 == 9.0).all() and not (y2 == 9.0).all()
    assert R.next_clock(0) == 1 and R.next_clock(7) == 8 and R.next_clock(0, 2) == 3


# ---- the refusals ------------------------------------------------------------------------------------------------------------------
def test_waveform_refusals():
    nan, inf = float("nan"), float("inf")
    for bad in (lambda: T.Const(nan), lambda: T.Const(inf), lambda: T.Const("1"), lambda: T.Const(True),
                lambda: T.Ramp(0.0, nan, 0.0, 1.0), lambda: T.Ramp(0.0, 1.0, -inf, 1.0), lambda: T.Ramp(-1e308, 1e308, 0.0, 1.0),
                lambda: T.Sine(1.0, inf, 1.0), lambda: T.Sine(1.0, 0.1, 1.0, phase=nan), lambda: T.Sine(1.0, 0.1, 1.0, start=inf),
                lambda: T.Table([0.0, 1.0], [1.0, nan]), lambda: T.Table([0.0, inf], [1.0, 1.0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="t1 > t0"):
        T.Ramp(0.0, 1.0, 2.0, 2.0)
    with pytest.raises(ValueError, match="t1 > t0"):
        T.Ramp(0.0, 1.0, 2.0, 1.0)
    with pytest.raises(ValueError, match="shape"):
        T.Ramp(0.0, 1.0, 0.0, 1.0, "cubic")
    with pytest.raises(ValueError, match="freq"):
        T.Sine(1.0, 0.1, -0.5)
    with pytest.raises(ValueError, match="strictly increasing"):
        T.Table([0.0, 1.0, 1.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        T.Table([0.0, 2.0, 1.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="1024"):
        T.Table(list(range(1025)), [0.0] * 1025)
    with pytest.raises(ValueError, match="1024"):
        T.Table([], [])
    with pytest.raises(ValueError, match="times for"):
        T.Table([0.0, 1.0], [1.0])
    with pytest.raises(ValueError, match="periodic"):
        T.Table([0.0], [1.0], periodic=True)
    T.Table(list(range(1024)), [0.0] * 1024)                           # the longest table there is


def test_object_refusals():
    with pytest.raises(ValueError, match="drives nothing"):
        T.TimeBC()
    with pytest.raises(ValueError, match="drives nothing"):
        T.TimeBC(velocity=None, source=None)
    with pytest.raises(ValueError, match="unknown node names"):
        T.TimeBC(velocity=T.Const(), nodes=("inflow", "outflow"))
    with pytest.raises(ValueError, match="unknown node names"):
        T.TimeBC(velocity=T.Const(), nodes="lid")
    with pytest.raises(ValueError, match="at least one node"):
        T.TimeBC(velocity=T.Const(), nodes=())
    with pytest.raises(ValueError, match="waveform"):
        T.TimeBC(velocity=1.0)
    with pytest.raises(ValueError, match="one waveform per graph"):
        T.TimeBC(source=[T.Const(), 2.0])
    with pytest.raises(ValueError, match="one waveform per graph"):
        T.TimeBC(source=[])
    tbc = T.TimeBC(velocity=[T.Const(), T.Const(2.0), T.Const(3.0)], source=T.Const())
    assert tbc.type_mask == (1 << 1) | (1 << 5) and tbc.channels == 3           # the default nodes: inflow and in_wall
    assert T.TimeBC(source=T.Const(), nodes=()).channels == 2
    assert T.TimeBC(velocity=T.Const(), nodes=("wall",)).type_mask == 1 << 3
    with pytest.raises(ValueError, match="3 waveforms for a batch of 2"):
        tbc.resolve(2)
    assert [len(c) for c in tbc.resolve(3)] == [3, 3]
    with pytest.raises(RuntimeError, match="not attached"):
        tbc.read()
    with pytest.raises(RuntimeError, match="not attached"):
        tbc.set(velocity=T.Const())
    with pytest.raises(RuntimeError, match="not attached"):
        tbc.evaluate(1)


def test_owner_refusals_that_need_no_gpu():
    from FVMmodel.importer import NNmodel
    from gfv.march import MarchStep
    from gfv.params import default_params
    from gfv.rollout import Rollout
    graphs = cases.make_graphs("cyl_cavity_b2")                        # CPU graphs: every refusal below comes before the device
    model = NNmodel(default_params())
    tbc = T.TimeBC(velocity=T.Const())
    with pytest.raises(ValueError, match="anderson"):
        Rollout(model, graphs, max_steps=4, anderson=2, time_bc=tbc)
    with pytest.raises(ValueError, match="TimeBC"):
        Rollout(model, graphs, max_steps=4, time_bc=dict(velocity=1.0))
    with pytest.raises(ValueError, match="TimeBC"):
        MarchStep(model, graphs, time_bc="sine")
    three = T.TimeBC(velocity=[T.Const()] * 3)
    with pytest.raises(ValueError, match="3 waveforms for a batch of 2"):
        Rollout(model, graphs, max_steps=4, time_bc=three)
    with pytest.raises(ValueError, match="3 waveforms for a batch of 2"):
        MarchStep(model, graphs, time_bc=three)
    pooled = (types.SimpleNamespace(_gfv_pool_plan=object()),) + tuple(graphs[1:])
    with pytest.raises(ValueError, match="DevicePool"):
        Rollout(model, pooled, max_steps=4, time_bc=tbc)
    with pytest.raises(ValueError, match="DevicePool"):
        MarchStep(model, pooled, time_bc=tbc)
    taken = T.TimeBC(velocity=T.Const())
    taken._owner = "Rollout"                                           # (what attach() leaves behind)
    with pytest.raises(ValueError, match="already attached"):
        Rollout(model, graphs, max_steps=4, time_bc=taken)
    with pytest.raises(ValueError, match="already attached"):
        MarchStep(model, graphs, time_bc=taken)
    tbc.check_free()                                                   # constructors that raised attached nothing
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        Rollout(model, graphs, max_steps=4, time_bc=tbc)               # CPU graphs are refused as without time_bc
    tbc.check_free()


# ---- the records ----------------------------------------------------------------------------------------------------------------------
WAVES = [T.Const(), T.Const(-2.5), T.Ramp(0.0, 1.0, 0.0, 5.0), T.Ramp(1.5, -0.5, -1.0, 0.25, "smooth"), T.Sine(1.0, 0.3, 0.2),
         T.Sine(0.0, 1.0, 0.0, phase=0.5, start=3.0), T.Table([0.0, 1.0, 4.0], [1.0, 2.0, 0.0]), T.Table([0.5, 0.75], [3.0, 4.0], True),
         T.Table([2.0], [7.0]), T.Table(np.linspace(0.0, 1.0, 1024), np.arange(1024.0), periodic=True)]


@pytest.mark.parametrize("w", WAVES, ids=lambda w: type(w).__name__)
def test_pack_and_unpack_give_the_same_parameters(w):
    from gfv import lib as L
    rec, times, values = w.pack()
    assert len(rec) == L.TIME_BC_RECORD and all(isinstance(v, float) for v in rec) and rec[0] == int(rec[0])
    # through the device's storage format: float64 words, the table in a slot of TABLE_MAX points
    rec64 = torch.tensor(rec, dtype=torch.float64)
    slot = torch.zeros((2, L.TIME_BC_TABLE_MAX), dtype=torch.float64)
    if times is not None:
        slot[0, :len(times)] = torch.tensor(times, dtype=torch.float64)
        slot[1, :len(values)] = torch.tensor(values, dtype=torch.float64)
    back = T.unpack(rec64.tolist(), slot[0].tolist(), slot[1].tolist())
    assert back == w and type(back) is type(w) and back.pack() == (rec, times, values)
    assert R.from_object(back)[0] in ("const", "ramp", "sine", "table")
    assert (w != T.Const(123.0)) and not (w == 1.0)
    with pytest.raises(ValueError, match="not a waveform"):
        T.unpack([0.0] * 8)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_bound_and_refuses_bad_arguments_without_a_gpu():
    from gfv import lib as L
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    assert re.search(r"\bint gfv_time_bc_update\(", header)
    for name in ("RECORD", "CTL", "HIST", "TABLE_MAX", "NONE", "CONST", "RAMP_LINEAR", "RAMP_SMOOTH", "SINE", "TABLE", "TABLE_PERIODIC"):
        m = re.search(rf"#define GFV_TIME_BC_{name} (\d+)", header)
        assert m and int(m.group(1)) == getattr(L, "TIME_BC_" + name), name
    lib = L.load()
    assert "gfv_time_bc_update" in L.declared_symbols()
    a = (C.c_double * 64)()                                            # one 8-byte aligned host buffer stands in for every pointer:
    p = C.addressof(a)                                                 # each call below is refused before a launch
    q = p + 256

    def call(clock=p, ctl=p, rec=p, tab=p, dt=p, batch=p, nt=p, N=4, B=1, y0=p, y=q, th0=p, th5=q, ld=9, xb=None, x=None, hist=None,
             K=0, mask=2, ch=3):
        return lib.gfv_time_bc_update(clock, ctl, rec, tab, dt, batch, nt, N, B, y0, y, th0, th5, ld, xb, x, hist, K, mask, ch, None)

    for bad in (dict(clock=None), dict(ctl=None), dict(rec=None), dict(dt=None), dict(batch=None), dict(nt=None), dict(N=0), dict(B=0),
                dict(ch=0), dict(ch=4), dict(mask=64), dict(y0=None, ch=1), dict(y=None, ch=1), dict(y=p, ch=1), dict(y=q + 4, ch=1),
                dict(th0=None, ch=2), dict(th5=None, ch=2), dict(ld=0, ch=2), dict(hist=q, K=0), dict(rec=p + 4), dict(tab=p + 4),
                dict(hist=q + 4, K=3)):
        assert call(**bad) == -1, bad
