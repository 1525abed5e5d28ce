"""Time march on the device (gfv/march.py, csrc/march.hip; include/gfv.h gfv_march_advance).

1. the kernel alone against tests/march_ref.py, launch by launch: record, r0, fields and snapshots bit for bit, the two norms of a
   history row within one fp32 spacing of the float64 reference (the bound of tests/test_evaluate_gpu.py: the two sides may differ
   in the order of a double sum, which moves the fp32 rounding by one step at most);
2. a fixed count is today's path: `TrainStep.step()` x 5 + `advance_time()`, bit for bit;
3. convergence is a host that synchronises after every step and decides by tests/march_ref.py, bit for bit, with both exits taken;
4. the result does not depend on how far the host ran ahead;   5. freeze at the target, and resume;
6. with the guard, averaged weights, groups and the log;       7. snapshots;   8. refusals that need the device.

The tolerance of 3 comes from the ORACLE's loop (oracle.fvgn_oracle.train_step on the CPU, small polygon mesh, lr 5e-5,
dataset_size 1, the march rule with max_inner = 5), whose ratios r_k / r_0 are
    level 0:  1.00000 0.98704 0.97343 0.96177          (ends at k = 4: CONVERGED)
    level 1:  1.00000 0.99149 0.98482 0.97808 0.97218  (k = 5: CAPPED)
    level 2:  1.00000 0.99325 0.98781 0.98273 0.97840  (k = 5: CAPPED)
TOL = sqrt(0.97343 * 0.96177) = 0.96758, the geometric mean of two consecutive ratios 1.2 % apart: every ratio the decisions see
is at least 0.47 % away from it, the HIP path is 1e-5 from the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases
import march_ref as R
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

f32 = np.float32
LR, TOL, MAX_INNER, LEVELS = 5e-5, 0.96758, 5, 3
TINY = 1e-6


def _model(hidden=128):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    if hidden == 128:
        P, m = O.init_parameters(cases.WEIGHT_SEED), NNmodel(default_params(dataset_size=1))
    else:
        P = O.init_parameters(cases.WEIGHT_SEED, {"hidden_size": hidden})
        m = NNmodel(default_params(dataset_size=1, hidden_size=hidden))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


@functools.lru_cache(maxsize=None)
def _cpu_graphs(which):
    if which == "poly":
        from test_config5_gpu import _small_polygon_graphs
        return _small_polygon_graphs()
    return cases.make_graphs(which)


def _graphs(which="poly"):
    return tuple(g.clone().to("cuda") for g in _cpu_graphs(which))


def _state(ts):
    """What a march must reproduce, as CPU copies (synchronises)."""
    torch.cuda.synchronize()
    return {"flat_p": ts.flat_p.cpu().clone(), "flat_m": ts.flat_m.cpu().clone(), "flat_v": ts.flat_v.cpu().clone(),
            "adam_t": ts.adam_state[0:1].cpu().clone(), "x_backup": ts.x_backup.cpu().clone()}


def _bits(t):
    if t.dtype in (torch.float32, torch.float64):
        return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return t


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _same_rows(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra.keys() == rb.keys()
        for k in ra:
            if isinstance(ra[k], torch.Tensor):
                assert torch.equal(_bits(ra[k]), _bits(rb[k])), k
            else:
                assert ra[k] == rb[k], k


def _within_one_spacing(got, want, what):
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    lo, hi = np.nextafter(want, f32(-np.inf)), np.nextafter(want, f32(np.inf))
    steps = got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
    print(f"{what}: got {got} want {want} fp32 steps apart {steps}")
    assert np.all((got == want) | (got == lo) | (got == hi)), (what, got, want)
    assert np.all(np.isfinite(got))


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
# B = 2: graph 0 of six chunks (a one-row chunk, one of more than 64 rows, a full 64), graph 1 a single chunk whose end lies past
# N; seven chunks = two workgroups of four waves, the second with an idle wave; N = 219 rows, no multiple of 64.
ROWS = [[1, 70, 33, 64, 5, 17], [29]]
W = (2.0, 0.5, 1.0)   # w_cont, w_mom, w_press


def _tables():
    rows = np.array([r for g in ROWS for r in g], dtype=np.int64)
    end = np.cumsum(rows)
    beg = end - rows
    N = int(end[-1])
    end[-1] += 5
    gcp = np.concatenate(([0], np.cumsum([len(g) for g in ROWS])))
    return beg.astype(np.int32), end.astype(np.int32), gcp.astype(np.int32), N


def _script():
    """(press residual of graph 0, of graph 1, host words to write first) per launch; max_inner 4, min_inner 3, tol 0.5.
    The small cont / momentum terms added below keep the fp32 order of the residual's sum in play without moving an outcome."""
    nan = float("nan")
    return [
        (8.0, 4.0, None, "open"),          # level 0, k = 1: r0
        (1.0, 1.0, None, "open"),          # converged at k = 2, held back by min_inner = 3
        (1.0, 1.0, None, "latched"),       # k = 3: CONVERGED
        (8.0, 4.0, None, "open"),          # level 1
        (3.9, 2.5, None, "open"),          # graph 0 converged, graph 1 not (k = 2 in any case)
        (3.9, nan, None, "open"),          # k = 3 >= min_inner, graph 0 converged: the NaN of graph 1 alone keeps the level open
        (8.0, 4.0, None, "latched"),       # k = 4: CAPPED
        (8.0, 4.0, dict(tol=-1.0, abs_tol=0.75), "open"),     # level 2: abs_tol alone
        (0.5, 0.5, None, "open"),          # converged at k = 2 < min_inner
        (0.5, 0.8, None, "open"),          # k = 3: graph 1 above abs_tol (0.8 <= 0.5 * 4 would have fired the relative test)
        (0.5, 0.5, None, "latched"),       # k = 4: CONVERGED and CAPPED; level 3 = target: done
        (9.0, 9.0, None, "held"),
        (9.0, 9.0, None, "held"),
        (8.0, 4.0, dict(target=4, done=0), "open"),           # what a later run() writes: the march resumes
    ]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_kernel_script():
    """-> (per launch: the device buffers after it, the reference's buffers after it, the outcome)."""
    from gfv import lib as L
    lib = L.load()
    cb, ce, gcp, N = _tables()
    B, nc, keep, max_levels = 2, len(cb), 2, 4
    rng = np.random.default_rng(20250311)
    spread = lambda shape: (rng.standard_normal(shape) * 10.0 ** rng.uniform(-1.5, 1.5, shape)).astype(f32)
    xb0 = spread((N, 12))
    ref = R.MarchRef(xb0, cb, ce, gcp, W, max_inner=4, min_inner=3, tol=0.5, abs_tol=-1.0, target=3, max_levels=max_levels,
                     keep=keep)
    d = dict(cb=_dev(cb), ce=_dev(ce), gcp=_dev(gcp), xb=_dev(xb0), x=torch.full((N, 12), 7.0, device="cuda"),
             partial=torch.full((nc, 2), -1.0, dtype=torch.float64, device="cuda"),
             hyper=_dev(np.array([1e-3, 0.9, 0.999, 1e-8, 1.0, *W], dtype=f32)), march=_dev(ref.rec.copy()),
             r0=torch.zeros(B, device="cuda"), hist=torch.zeros((max_levels, R.HEAD + R.GRAPH * B), dtype=torch.int32, device="cuda"),
             snap=torch.zeros((keep, N, 3), device="cuda"))
    ref.x[:] = 7.0
    host, devp = C.POINTER(C.c_int32)(), C.c_void_p()
    L.check(L.load(raw=True).gfv_sweep_mirror_create(3, C.byref(host), C.byref(devp)), "gfv_sweep_mirror_create")
    out = []
    try:
        for press0, press1, words, expect in _script():
            if words:
                for name, v in words.items():
                    idx = getattr(R, name.upper())
                    w = np.array([v], dtype=f32).view(np.int32)[0] if name in ("tol", "abs_tol") else np.int32(v)
                    ref.rec[idx] = w
                    d["march"][idx:idx + 1].copy_(torch.tensor([int(w)], dtype=torch.int32))
            losses = (rng.uniform(1e-5, 1e-4, (B, 4))).astype(f32)
            losses[:, 3] = (press0, press1)
            uvp = spread((N, 3))
            before = {k: d[k].cpu().clone() for k in ("xb", "x", "r0", "hist", "snap", "partial")}
            uvp_d, losses_d = _dev(uvp), _dev(losses)               # (held by name: the launch reads them after this statement)
            L.check(lib.gfv_march_advance(
                uvp_d.data_ptr(), d["xb"].data_ptr(), d["x"].data_ptr(), N, d["cb"].data_ptr(), d["ce"].data_ptr(),
                d["gcp"].data_ptr(), nc, B, losses_d.data_ptr(), d["partial"].data_ptr(), d["hyper"].data_ptr(),
                d["march"].data_ptr(), d["r0"].data_ptr(), d["hist"].data_ptr(), max_levels, 4, 3, d["snap"].data_ptr(), keep,
                devp.value, L.stream_ptr()), "gfv_march_advance")
            torch.cuda.synchronize()
            outcome = ref.launch(uvp, losses)
            assert outcome == expect, (len(out), outcome, expect)
            got = {k: d[k].cpu().clone() for k in ("march", "xb", "x", "r0", "hist", "snap", "partial")}
            got["mirror"] = [int(host[i]) for i in range(3)]
            want = dict(march=ref.rec.copy(), xb=ref.x_backup.copy(), x=ref.x.copy(), r0=ref.r0.copy(), hist=ref.hist.copy(),
                        snap=ref.snap.copy())
            out.append((got, want, outcome, before))
    finally:
        torch.cuda.synchronize()
        L.load(raw=True).gfv_sweep_mirror_free(host)
    return out


def test_the_kernel_alone_follows_the_reference_launch_by_launch():
    run = _run_kernel_script()
    assert [o for _, _, o, _ in run].count("latched") == 3 and [o for _, _, o, _ in run].count("held") == 2
    norm_cols = [R.HEAD + R.GRAPH * b + c for b in range(2) for c in (6, 7)]
    exact = np.ones(R.HEAD + R.GRAPH * 2, dtype=bool)
    exact[norm_cols] = False
    for i, (got, want, outcome, before) in enumerate(run):
        what = f"launch {i} ({outcome})"
        assert got["march"].numpy().tolist() == want["march"].tolist(), what          # every word, the arrival counter at zero
        assert got["march"][R.COUNTER] == 0
        for k in ("xb", "x", "r0", "snap"):
            assert got[k].numpy().tobytes() == want[k].tobytes(), (what, k)
        gh, wh = got["hist"].numpy(), want["hist"]
        assert gh[:, exact].tobytes() == wh[:, exact].tobytes(), what
        done = int(want["march"][R.LEVEL])
        if done:
            _within_one_spacing(gh[:done][:, norm_cols].view(f32), wh[:done][:, norm_cols].view(f32), what + " norms")
        assert (gh[done:] == 0).all()
        assert got["mirror"] == [int(want["march"][R.SEEN]), int(want["march"][R.LEVEL]), int(want["march"][R.DONE])], what
        if outcome in ("held", "open"):
            # no row of the state, the history, the snapshots or the workspace moves (r0 moves on a level's first iteration)
            for k in ("xb", "x", "hist", "snap", "partial") + (("r0",) if outcome == "held" else ()):
                assert torch.equal(_bits(got[k]), _bits(before[k])), (what, k)
    again = _run_kernel_script()
    for (a, _, _, _), (b, _, _, _) in zip(run, again):
        for k in ("march", "xb", "x", "r0", "hist", "snap"):
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k                # norms included: same inputs, same bits
        assert a["mirror"] == b["mirror"]


# ---- 2. a fixed count is today's path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [False, "list"], ids=["eager", "list"])
@pytest.mark.parametrize("which", ["poly", "cyl_cavity_b2"])
def test_a_fixed_count_is_trainstep_plus_advance_time(which, mode):
    from gfv.march import MarchStep
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(which), lr=LR, use_graph=mode)
    want_loss = []
    for _ in range(2):
        for _ in range(5):
            want_loss.append(ts.step().clone())
        ts.advance_time()
    ms = MarchStep(_model(), _graphs(which), lr=LR, use_graph=mode, tol=-1, abs_tol=-1, min_inner=5, max_inner=5, max_levels=4)
    got_loss = [ms.step().clone() for _ in range(10)]          # (no target but the history's size: the device ends the levels)
    _assert_same(_state(ms), _state(ts), f"{which} {mode}")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got_loss, want_loss))
    rows = ms.history()
    assert [(r["level"], r["inner"], r["converged"], r["capped"], r["seen"]) for r in rows] == [(0, 5, False, True, 5),
                                                                                                 (1, 5, False, True, 10)]
    st = ms.stats()
    assert (st["level"], st["inner"], st["seen"], st["held"], st["done"]) == (2, 0, 10, 0, False)
    # ... and through run(): two more levels, exactly 10 steps issued, none held
    rows = ms.run(levels=2, max_ahead=4)
    for _ in range(2):
        for _ in range(5):
            ts.step()
        ts.advance_time()
    _assert_same(_state(ms), _state(ts), f"{which} {mode} run()")
    assert [(r["level"], r["inner"], r["capped"]) for r in rows] == [(2, 5, True), (3, 5, True)]
    st = ms.stats()
    assert (st["seen"], st["held"], st["done"]) == (20, 0, True)


def test_a_padded_hidden_size_marches_like_trainstep():
    from gfv.march import MarchStep
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(64), _graphs(), lr=LR, use_graph=False)
    for _ in range(3):
        ts.step()
    ts.advance_time()
    ms = MarchStep(_model(64), _graphs(), lr=LR, use_graph=False, tol=-1, abs_tol=-1, min_inner=3, max_inner=3, max_levels=2)
    rows = ms.run(levels=1)
    assert ms.padded and [(r["inner"], r["capped"]) for r in rows] == [(3, True)]
    _assert_same(_state(ms), _state(ts), "hidden 64")


# ---- 3. convergence is a host that synchronises ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_loop(mode, tol, levels=LEVELS):
    """TrainStep.step(); losses to the host; the decision of tests/march_ref.py; advance_time().  Computed once per case."""
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=mode)
    w = ts.loss_weights
    counts, fields, losses = [], [], []
    for _ in range(levels):
        inner, r0 = 0, None
        while True:
            losses.append(ts.step().cpu().clone())
            r = R.residual(ts.losses.cpu().numpy(), *w)
            r0 = r if inner == 0 else r0
            inner, conv, cap = R.decide(inner, R.converged(r, r0, tol, -1.0).all(), 1, MAX_INNER)
            if conv or cap:
                ts.advance_time()
                break
        counts.append((inner, conv, cap))
        fields.append(ts.x_backup[:, 0:3].cpu().clone())
    return dict(state=_state(ts), counts=counts, fields=fields, losses=losses)


def _march(mode, tol, **kw):
    from gfv.march import MarchStep
    return MarchStep(_model(), _graphs(), lr=LR, use_graph=mode, tol=tol, max_inner=MAX_INNER, max_levels=8, **kw)


@pytest.mark.parametrize("mode,tol", [(False, TOL), ("list", TOL), ("list", TINY)], ids=["eager", "list", "list-tiny-tol"])
def test_convergence_is_a_host_that_synchronises_after_every_step(mode, tol):
    ref = _host_loop(mode, tol)
    ms = _march(mode, tol)
    rows = ms.run(levels=LEVELS, max_ahead=8)
    print([(r["inner"], r["converged"], r["capped"], (r["r"] / r["r0"]).tolist()) for r in rows])
    assert [(r["inner"], r["converged"], r["capped"]) for r in rows] == ref["counts"]
    _assert_same(_state(ms), ref["state"], f"{mode} {tol}")
    # the coverage this test exists for: both exits are taken
    if tol == TOL:
        assert any(r["converged"] and r["inner"] < MAX_INNER for r in rows)
    else:
        assert any(r["capped"] and not r["converged"] for r in rows)
    st = ms.stats()
    assert st["level"] == LEVELS and st["done"] and st["seen"] == sum(c[0] for c in ref["counts"])
    for r in rows:
        assert torch.equal(r["r"] <= torch.tensor(tol, dtype=torch.float32) * r["r0"], torch.tensor([r["converged"]]))


# ---- 4. run-ahead independence ---------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_how_far_the_host_ran_ahead():
    ref = _host_loop("list", TOL)
    outs = []
    for ahead in (0, 16):
        ms = _march("list", TOL, log=64)
        rows = ms.run(levels=LEVELS, max_ahead=ahead)
        st, log = ms.stats(), ms.log.read()
        applied = log.apply == 1
        assert int(applied.sum()) == st["seen"] and len(log.apply) == st["seen"] + st["held"]
        outs.append((_state(ms), rows, log.loss[applied].copy(), st))
    assert outs[0][3]["held"] == 0                                  # a synchronisation per step never issues a step too many
    for state, rows, loss, st in outs:
        _assert_same(state, ref["state"], "run-ahead")
        assert loss.view(np.int32).tolist() == [int(_bits(l)) for l in ref["losses"]]
    _same_rows(outs[0][1], outs[1][1])
    print("held with max_ahead=16:", outs[1][3]["held"])


# ---- 5. freeze and resume ---------------------------------------------------------------------------------------------------------
def _full_state(ms):
    """Everything a held step must leave alone.  The flat buffers by parameter: the alignment padding between tensors is not state
    (TrainStep.named_state: its gradient slots take what a shared workspace held, which a held step's backward leaves differently
    from an applied one's - one padding element behind the decoder's three biases moves with it; nothing reads it)."""
    torch.cuda.synchronize()
    named = lambda buf: torch.cat([ms.G.view_of(buf, n).reshape(-1) for n in ms.G.off]).cpu()
    return {"p": named(ms.flat_p), "m": named(ms.flat_m), "v": named(ms.flat_v), "ema": named(ms._ema.e),
            "x_backup": ms.x_backup.cpu().clone(), "adam_state": ms.adam_state.cpu().clone(), "ema_rec": ms._ema.rec.cpu().clone(),
            "guard": ms._guard.guard.cpu().clone(), "r0": ms._r0.cpu().clone(), "hist": ms._hist.cpu().clone()}


def test_steps_behind_the_target_are_held_and_a_later_run_resumes():
    kw = dict(max_grad_norm=1e-3, skip_nonfinite=True, ema_decay=0.9)
    ms = _march("list", TOL, **kw)
    ms.run(levels=2, max_ahead=8)
    before, st0 = _full_state(ms), ms.stats()
    for _ in range(3):
        ms.step()
    after, st1 = _full_state(ms), ms.stats()
    _assert_same(after, before, "held")                             # parameters, moments, count, EMA, guard counts, field, history
    assert st1["held"] == st0["held"] + 3 and st1["apply"] == 0 and st1["seen"] == st0["seen"] and st1["level"] == 2
    with pytest.raises(IndexError, match="max_levels"):
        ms.run(levels=7)
    rows = ms.run(levels=1, max_ahead=8)
    whole = _march("list", TOL, **kw)
    all_rows = whole.run(levels=3, max_ahead=8)
    a, b = _full_state(ms), _full_state(whole)
    _assert_same(a, b, "resumed")
    _same_rows(rows, all_rows[2:])
    assert ms.stats()["seen"] == whole.stats()["seen"]


# ---- 6. with the guard, averaged weights, groups and the log ---------------------------------------------------------------------
def test_guard_ema_groups_and_log_count_the_applied_steps_only():
    groups = [dict(params=["simulator.decoder"], lr_scale=0.5, weight_decay=0.01)]
    ms = _march("list", TOL, max_grad_norm=1e-3, ema_decay=0.9, param_groups=groups, weight_decay=0.001, log=64, keep=2)
    ms.run(levels=2, max_ahead=16)
    for _ in range(2):
        ms.step()                                                   # two held steps for certain
    st, log = ms.stats(), ms.log.read()
    seen, held = st["seen"], st["held"]
    assert held >= 2 and st["level"] == 2
    assert ms.ema_stats()["updates"] == seen and float(ms.adam_state[0]) == seen
    g = ms.guard_stats()
    assert g["clipped"] == seen and g["skipped_nonfinite"] == 0     # (max_grad_norm far below the gradient's norm: every step clips)
    assert log.apply.tolist() == [1] * seen + [0] * held            # 0 exactly on the held steps
    assert log.applied.tolist() == log.apply.tolist()
    assert log.adam_t[seen - 1] == seen and (log.adam_t[seen:] == seen).all()


# ---- 7. snapshots ---------------------------------------------------------------------------------------------------------------
def test_snapshots_are_the_fields_the_host_loop_saw_at_each_level():
    ref = _host_loop("list", TOL)
    ms = _march("list", TOL, keep=2)
    ms.run(levels=LEVELS, max_ahead=8)
    for level in (1, 2):
        assert torch.equal(_bits(ms.snapshot(level).cpu()), _bits(ref["fields"][level])), level
    for level in (0, 3, -1):
        with pytest.raises(IndexError):
            ms.snapshot(level)
    assert ms.level == LEVELS
    with pytest.raises(RuntimeError, match="keep=0"):
        _march(False, TOL).snapshot(0)


# ---- 8. the refusals and reset() ---------------------------------------------------------------------------------------------------
def test_refusals_and_reset():
    from gfv.march import MarchStep
    ms = _march(False, TINY)
    with pytest.raises(RuntimeError, match="device owns"):
        ms.advance_time()
    with pytest.raises(RuntimeError, match="one batch"):
        ms.set_batch(_graphs())
    with pytest.raises(ValueError, match="accum_steps"):
        ms.accum_steps = 2
    for bad in (dict(levels=0), dict(levels=1, max_ahead=-1)):
        with pytest.raises(ValueError):
            ms.run(**bad)
    with pytest.raises(IndexError, match="max_levels"):
        ms.run(levels=9)
    with pytest.raises(ValueError, match="min_inner"):
        ms.set_control(min_inner=MAX_INNER + 1)
    for kw, what in ((dict(use_graph=True), "use_graph"), (dict(accum_steps=2), "accum_steps"), (dict(distributed=True), "parallel"),
                     (dict(world_size=2), "parallel"), (dict(want_outputs=False), "want_outputs")):
        with pytest.raises(ValueError, match=what):
            MarchStep(ms.model, ms.graphs, **kw)
    x0 = ms.x_backup.cpu().clone()
    ms.set_control(max_inner=2, min_inner=2)
    rows = ms.run(levels=1)
    assert [(r["inner"], r["capped"]) for r in rows] == [(2, True)] and not torch.equal(ms.x_backup.cpu(), x0)
    ms.reset()
    st = ms.stats()
    assert (st["level"], st["inner"], st["seen"], st["held"], st["done"]) == (0, 0, 0, 0, False)
    assert torch.equal(ms.x_backup.cpu(), x0) and ms.history() == []
