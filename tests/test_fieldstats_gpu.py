"""Field statistics on the device (gfv/fieldstats.py, csrc/fieldstats.hip; include/gfv.h gfv_field_stats_update).

1. the kernel alone through ctypes against tests/fieldstats_ref.py, launch by launch: record, sums and shift / extremes bit for bit
   (the test writes the clock word itself), one row with a NaN sample;
2. `Rollout` with statistics: the raw state is the reference over the fields a second `Rollout` WITHOUT statistics wrote, bit for
   bit, list mode and eager mode alike; history, fields and node state are those of the run without statistics;
3. `set_window()` in the middle of a list-mode run holds from the next step without a new recording; `reset()` starts over;
4. `MarchStep` (the constants of tests/test_march_gpu.py): one sample per completed level whatever its inner count, held steps
   sample nothing, the march itself is the march without statistics bit for bit;
5. `read()` against float64 two-pass statistics of the captured fields, within the derived bounds of tests/test_fieldstats_cpu.py;
6. the refusals that need the device.
"""
import functools

import numpy as np
import pytest
import torch

import cases
import fieldstats_ref as R
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
STEPS, START, STRIDE = 12, 3, 2


def _same(a, b):
    """Bit equality of two arrays / tensors (NaN and -0 included)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_raw(raw, ref, what):
    rec, sums, aux = raw
    assert rec.numpy().tolist() == ref.rec.tolist(), (what, rec.tolist(), ref.rec.tolist())
    assert int(rec[R.COUNTER]) == 0 and int(rec[7]) == 0, what
    assert _same(sums, ref.sums), (what, "sums")
    assert _same(aux, ref.aux), (what, "aux")


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
# (host words to write first, the clock, whether the launch samples); start = 2, stride = 2, no stop at first
SCRIPT = [
    (None, 1, False),                 # a clock before start
    (None, 2, True),                  # the first sample: every element of the state is written
    (None, 2, False),                 # an unchanged clock
    (None, 3, False),                 # a stride miss
    (None, 4, True),                  # n > 0: the sums move (one row holds a NaN)
    (dict(ENABLED=0), 6, False),      # paused: the clock is followed, nothing is sampled
    (dict(ENABLED=1), 8, True),
    (dict(STOP=10), 10, False),       # stop is exclusive
]


@pytest.mark.parametrize("N", [1, 179, 257, 1000])
def test_the_kernel_alone_follows_the_reference_launch_by_launch(N):
    from gfv import lib as L
    lib = L.load()
    rng = np.random.default_rng(1000 + N)
    ref = R.FieldStatsRef(N, start=2, stride=2, stop=-1, enabled=1)
    ref.sums[:], ref.aux[:] = -1.0, 7.0                  # stale state: a reset clears nothing, the first sample writes it all
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rec, sums, aux, clock = dev(ref.rec), dev(ref.sums), dev(ref.aux), torch.zeros(1, dtype=torch.int32, device="cuda")
    nan_row = N // 2
    assert len(SCRIPT) == 8
    for i, (words, c, expect) in enumerate(SCRIPT):
        for name, v in (words or {}).items():
            idx = getattr(R, name)
            ref.rec[idx] = v
            rec[idx:idx + 1].copy_(torch.tensor([v], dtype=torch.int32))
        field = (rng.standard_normal((N, 12)) * 10.0 ** rng.uniform(-1.5, 1.5, (N, 12))).astype(f32)
        if i == 4:
            field[nan_row, 1] = np.nan
        if i == 6:
            field[nan_row, 0:3] = (-1e30, 1e30, np.nan)   # the extremes still move where a NaN went through the sums
        xb = dev(field)
        clock.copy_(torch.tensor([c], dtype=torch.int32))
        before = (sums.cpu().clone(), aux.cpu().clone(), int(rec[R.N]))
        L.check(lib.gfv_field_stats_update(xb.data_ptr(), N, clock.data_ptr(), rec.data_ptr(), sums.data_ptr(), aux.data_ptr(),
                                           L.stream_ptr()), "gfv_field_stats_update")
        torch.cuda.synchronize()
        what = f"N = {N}, launch {i} (clock {c})"
        assert ref.launch(field, c) is expect, what
        _assert_raw((rec.cpu(), sums.cpu(), aux.cpu()), ref, what)
        assert _same(xb, field) and int(clock[0]) == c, what                           # inputs are inputs
        if not expect:
            assert _same(sums, before[0]) and _same(aux, before[1]) and int(rec[R.N]) == before[2], what
    assert int(rec[R.N]) == 3
    # the NaN went where the reference says: the v sums of that row, and u'v'; its extremes per fminf / fmaxf
    s, a = sums.cpu().numpy(), aux.cpu().numpy()
    assert np.isnan(s[[1, 4, 6], nan_row]).all() and np.isfinite(s[[0, 3], nan_row]).all()
    assert a[3, nan_row] == f32(-1e30) and a[7, nan_row] == f32(1e30) and np.isfinite(a[3:9, nan_row]).all()
    assert np.isfinite(np.delete(s, nan_row, axis=1)).all()


# ---- 2. Rollout ----------------------------------------------------------------------------------------------------------------------
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
    if which == "poly":
        from test_config5_gpu import _small_polygon_graphs
        return _small_polygon_graphs()
    return cases.make_graphs(which)


def _graphs(which):
    hg = tuple(g.clone().to("cuda") for g in _cpu_graphs(which))
    hg[0].norm_uvp, hg[0].norm_global = True, True
    return hg


def _end_state(r, outs):
    torch.cuda.synchronize()
    return {"history": r.history.cpu().clone(), "x_backup": r.x_backup.cpu().clone(), "x": r.x.cpu().clone(),
            "state": r._state.cpu().clone(), "losses": outs[0].cpu().clone(), "uvp_node": outs[1].cpu().clone(),
            "uvp_cell": outs[2].cpu().clone()}


@functools.lru_cache(maxsize=None)
def _plain(which):
    """A Rollout WITHOUT statistics, stepped with .step(): the field after every step (CPU copies) and its end state.  Once."""
    from gfv.rollout import Rollout
    r = Rollout(_model(), _graphs(which), max_steps=STEPS)
    assert r.field_stats is None
    fields = []
    for _ in range(STEPS):
        outs = r.step()
        fields.append(r.x_backup[:, 0:3].cpu().numpy().copy())
    return fields, _end_state(r, outs), r.plan.N


@functools.lru_cache(maxsize=None)
def _with_stats(which, mode):
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    fs = FieldStats(start=START, stride=STRIDE)
    r = Rollout(_model(), _graphs(which), max_steps=STEPS, launch_mode=mode, field_stats=fs)
    assert r.field_stats is fs
    for _ in range(STEPS):
        outs = r.step()                                  # (no synchronisation in the loop)
    end = _end_state(r, outs)
    if mode == "cmd_list":
        st = r._lists.stats()                            # (the warm-up steps are eager: both launch paths carry the launch)
        assert st["recorded"] == 1 and st["replayed"] >= 6 and st["eager"] >= 2, st
    return fs.raw(), fs.read(), fs.count(), end


@pytest.mark.parametrize("which", ["poly", "cyl_cavity_b2"])
def test_rollout_statistics_are_the_reference_over_the_fields_of_a_run_without_them(which):
    fields, plain_end, N = _plain(which)
    if which == "poly":
        assert N == 179
    else:
        assert len(cases.CASES[which]) == 2
    ref = R.over(fields, range(1, STEPS + 1), N, start=START, stride=STRIDE)
    assert ref.rec[R.N] == 5 and ref.rec[R.LAST] == STEPS                              # clocks 3, 5, 7, 9, 11
    for mode in ("cmd_list", "eager"):
        raw, _, count, end = _with_stats(which, mode)
        _assert_raw(raw, ref, f"{which} {mode}")
        assert count == 5
        # the run itself is the run without statistics
        for k, v in plain_end.items():
            assert _same(end[k], v), (which, mode, k)
    a, b = _with_stats(which, "cmd_list")[0], _with_stats(which, "eager")[0]
    assert all(_same(u, v) for u, v in zip(a, b))


# ---- 3. the window moves under a recorded list ------------------------------------------------------------------------------------
def test_set_window_holds_from_the_next_step_without_a_new_recording_and_reset_starts_over():
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    fields, _, N = _plain("poly")
    fs = FieldStats()                                                                  # start = 1, stride = 1
    r = Rollout(_model(), _graphs("poly"), max_steps=STEPS, field_stats=fs)
    ref = R.FieldStatsRef(N)
    k = 0

    def steps(n):
        nonlocal k
        for _ in range(n):
            r.step()
            k += 1
            ref.launch(fields[k - 1], k)

    steps(5)                                                                           # the warm-up, the recording, a replay
    replayed = r._lists.stats()["replayed"]
    assert r._lists.stats()["recorded"] == 1 and replayed >= 1 and fs.count() == 5
    _assert_raw(fs.raw(), ref, "every step")
    fs.set_window(stride=3)                                                            # clocks 1, 4, 7, 10: the next is 7
    ref.rec[R.STRIDE] = 3
    steps(3)
    assert fs.count() == 6
    _assert_raw(fs.raw(), ref, "stride 3")
    fs.set_window(enabled=False)
    ref.rec[R.ENABLED] = 0
    steps(1)
    fs.set_window(enabled=True, stop=10)
    ref.rec[R.ENABLED], ref.rec[R.STOP] = 1, 10
    steps(2)                                                                           # 10: on the stride, but stop; 11: a miss
    assert fs.count() == 6
    _assert_raw(fs.raw(), ref, "paused, then stopped")
    assert r._lists.stats()["recorded"] == 1 and r._lists.stats()["replayed"] == replayed + 6    # nothing was recorded again
    # reset(): the owner's, which resets the statistics with it - the same run again, the window as it stands
    r.reset()
    assert fs.count() == 0 and fs.raw()[0].tolist()[R.LAST] == -1
    ref.reset()
    k = 0
    steps(5)
    assert fs.count() == 2                                                             # clocks 1 and 4
    _assert_raw(fs.raw(), ref, "after reset")
    assert r._lists.stats()["recorded"] == 1
    got = fs.read()
    want = R.over([fields[0], fields[3]], [1, 2], N).moments()
    assert all(_same(got[key].numpy(), np.ascontiguousarray(want[key])) for key in ("mean", "var", "cov_uv", "min", "max"))


# ---- 4. MarchStep ------------------------------------------------------------------------------------------------------------------
LR, TOL, MAX_INNER, LEVELS = 5e-5, 0.96758, 5, 3      # the constants of tests/test_march_gpu.py (its docstring derives TOL)


def _march_graphs():
    return tuple(g.clone().to("cuda") for g in _cpu_graphs("poly"))


def _march_state(ts):
    """What a march with statistics must reproduce, as CPU copies (synchronises)."""
    torch.cuda.synchronize()
    return {"flat_p": ts.flat_p.cpu().clone(), "flat_m": ts.flat_m.cpu().clone(), "flat_v": ts.flat_v.cpu().clone(),
            "adam_t": ts.adam_state[0:1].cpu().clone(), "x_backup": ts.x_backup.cpu().clone()}


def _same_rows(a, b):
    """Decoded history rows, bit for bit."""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert _same(ra[k], rb[k]) if isinstance(ra[k], torch.Tensor) else ra[k] == rb[k], k


@functools.lru_cache(maxsize=None)
def _march(ahead):
    """ahead None: a march without statistics.  -> (rows, state, snapshots, raw, count after the run, held, raw after two more
    (held) steps)."""
    import test_march_gpu as TM
    from gfv.fieldstats import FieldStats
    from gfv.march import MarchStep
    assert (TM.LR, TM.TOL, TM.MAX_INNER, TM.LEVELS) == (LR, TOL, MAX_INNER, LEVELS)
    fs = None if ahead is None else FieldStats(start=1)
    ms = MarchStep(_model(), _march_graphs(), lr=LR, use_graph="list", tol=TOL, max_inner=MAX_INNER, max_levels=8, keep=3,
                   field_stats=fs)
    assert ms.field_stats is fs
    rows = ms.run(levels=LEVELS, max_ahead=64 if ahead is None else ahead)
    state, held = _march_state(ms), ms.stats()["held"]
    snaps = [ms.snapshot(level).cpu().numpy() for level in range(LEVELS)]
    if fs is None:
        return rows, state, snaps, None, None, held, None
    raw, count = fs.raw(), fs.count()
    for _ in range(2):
        ms.step()                                                                      # held for certain
    assert ms.stats()["held"] == held + 2
    return rows, state, snaps, raw, count, held, fs.raw()


def test_march_takes_one_sample_per_completed_level_and_none_on_held_steps():
    plain_rows, plain_state, plain_snaps, *_ = _march(None)
    assert [r["inner"] for r in plain_rows] == [4, 5, 5]
    raws = {}
    for ahead in (64, 0):
        rows, state, snaps, raw, count, held, raw_held = _march(ahead)
        print(f"max_ahead={ahead}: held {held}")
        assert [r["inner"] for r in rows] == [4, 5, 5]
        assert count == 3                                                              # one per level: not 14, not 4 + 5 + 5
        ref = R.over(snaps, [1, 2, 3], snaps[0].shape[0], start=1)
        _assert_raw(raw, ref, f"max_ahead={ahead}")
        _assert_raw(raw_held, ref, f"max_ahead={ahead}, two held steps later")
        assert state.keys() == plain_state.keys()
        for k in state:
            assert _same(state[k], plain_state[k]), (ahead, k)                         # parameters, moments, step count, x_backup
        _same_rows(rows, plain_rows)
        assert all(_same(a, b) for a, b in zip(snaps, plain_snaps))
        raws[ahead] = raw
    assert _march(0)[5] == 0                                                           # a synchronisation per step holds nothing
    assert all(_same(u, v) for u, v in zip(raws[64], raws[0]))


def test_march_reset_starts_the_statistics_over():
    from gfv.fieldstats import FieldStats
    from gfv.march import MarchStep
    fs = FieldStats(start=2)
    ms = MarchStep(_model(), _march_graphs(), lr=LR, use_graph=False, tol=-1, abs_tol=-1, min_inner=2, max_inner=2, max_levels=4,
                   keep=2, field_stats=fs)
    ms.run(levels=2)
    ref = R.over([ms.snapshot(0).cpu().numpy(), ms.snapshot(1).cpu().numpy()], [1, 2], ms.plan.N, start=2)
    assert fs.count() == 1
    _assert_raw(fs.raw(), ref, "eager march, start = 2")
    assert set(ms.stats()) == {"level", "inner", "target", "done", "seen", "held", "apply"}      # stats() keeps its meaning
    assert "field_stats" not in ms.state_dict()
    ms.reset()
    rec = fs.raw()[0].tolist()
    assert rec[R.N] == 0 and rec[R.LAST] == -1 and fs.count() == 0


# ---- 5. read() ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["poly", "cyl_cavity_b2"])
def test_read_against_float64_two_pass_statistics(which):
    fields, _, N = _plain(which)
    raw, got, count, _ = _with_stats(which, "cmd_list")
    x = np.stack([fields[c - 1] for c in range(START, STEPS + 1, STRIDE)])             # [5, N, 3]
    assert got["n"] == count == x.shape[0] == 5
    assert got["mean"].dtype == torch.float64 and tuple(got["mean"].shape) == (N, 3) and tuple(got["cov_uv"].shape) == (N,)
    assert got["min"].dtype == torch.float32 and not any(v.is_cuda for v in got.values() if isinstance(v, torch.Tensor))
    s2n = float((raw[1][3:6] / 5).max())
    R.check_against_two_pass({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}, x, s2n, which)
    assert float(got["var"].min()) >= -1e-12 * s2n


# ---- 6. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    model = _model()
    fs = FieldStats(start=100)
    with pytest.raises(ValueError, match="anderson"):
        Rollout(model, _graphs("poly"), max_steps=4, anderson=2, field_stats=fs)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        Rollout(model, tuple(g.clone() for g in _cpu_graphs("poly")), max_steps=4, field_stats=fs)               # CPU graphs
    with pytest.raises(ValueError, match="max_steps"):
        Rollout(model, _graphs("poly"), max_steps=0, field_stats=fs)
    fs.check_free()                                                                    # a constructor that raised attached nothing
    with pytest.raises(ValueError, match="GPU"):
        FieldStats().attach(object(), torch.zeros(8, 12), torch.zeros(1, dtype=torch.int32))     # a CPU tensor
    with pytest.raises(ValueError, match="FieldStats"):
        Rollout(model, _graphs("poly"), max_steps=4, field_stats=dict(start=1))
    r = Rollout(model, _graphs("poly"), max_steps=4, launch_mode="eager", field_stats=fs)
    with pytest.raises(ValueError, match="already attached"):
        Rollout(model, _graphs("poly"), max_steps=4, field_stats=fs)                    # one owner per object
    # no reference back to the owner: a cycle would keep a dead owner's recorded lists alive until a garbage collection
    assert not any(v is r for v in vars(fs).values())
    r.step()
    assert fs.count() == 0 and fs.raw()[0].tolist()[R.LAST] == 1
    with pytest.raises(RuntimeError, match="n == 0"):
        fs.read()
    fs.set_window(start=2)
    r.step()
    assert fs.count() == 1 and fs.read()["n"] == 1 and float(fs.read()["var"].abs().max()) == 0.0
    with pytest.raises(ValueError, match="stride"):
        fs.set_window(stride=0)
