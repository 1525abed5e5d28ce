"""CPU: the host side of the time march (gfv/march.py, csrc/march.hip): the entry point is declared, exported and bound, every
bad argument is refused before anything touches a device, the constructor's refusals, `optimizer_launches(hold=)`, the history
decode on hand-made words, and the rule itself - tests/march_ref.py, the reference the GPU tests compare the kernel with - on
hand-made loss sequences.  Nothing here touches a GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import cases
import march_ref as R

f32 = np.float32


def test_march_entry_point_is_declared_exported_and_bound():
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    name = "gfv_march_advance"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert len(getattr(handle, name).argtypes) == 22
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert name not in cmdlist._QUERIES                                    # it launches: part of a recorded list
    for macro, value in (("RECORD", lib.MARCH_RECORD), ("HEAD", lib.MARCH_HEAD), ("GRAPH", lib.MARCH_GRAPH),
                         ("CONVERGED", lib.MARCH_CONVERGED), ("CAPPED", lib.MARCH_CAPPED)):
        assert int(re.search(rf"#define GFV_MARCH_{macro} (\d+)", header).group(1)) == value == getattr(R, macro)
    from gfv import march as M
    assert [M.MAX_INNER, M.MIN_INNER, M.INNER, M.APPLY, M.TOL, M.ABS_TOL, M.LEVEL, M.COUNTER, M.TARGET, M.DONE, M.SEEN, M.HELD,
            M.KEEP] == list(range(13)) and M.APPLY == 3                    # where the Adam launch reads accum[3]


def test_march_advance_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 16 == 0
    ok = dict(uvp=p, xb=p, x=p, N=4, cb=p, ce=p, gp=p, nc=1, B=2, losses=p, ws=p, hyper=p, march=p, r0=p, hist=p, ml=3, mx=5,
              mn=2, snap=p, keep=2, mirror=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_march_advance(a["uvp"], a["xb"], a["x"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["losses"],
                                     a["ws"], a["hyper"], a["march"], a["r0"], a["hist"], a["ml"], a["mx"], a["mn"], a["snap"],
                                     a["keep"], a["mirror"], None)
    for name in ("uvp", "xb", "x", "cb", "ce", "gp", "losses", "ws", "hyper", "march", "r0", "hist", "snap"):
        assert call(**{name: None}) == -1, name
    for name in ("N", "nc", "B", "ml"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(keep=-1) == -1
    assert call(mx=0) == -1 and call(mx=-2) == -1                          # max_inner < 1
    assert call(mn=0) == -1 and call(mn=6) == -1 and call(mn=-1) == -1     # min_inner outside [1, max_inner]
    assert call(xb=p + 4) == -1 and call(xb=p + 8) == -1 and call(x=p + 4) == -1     # the state rows move 16 bytes at a time


def test_constructor_refusals_need_no_device():
    from gfv.march import MarchStep, check_march_args, check_step_args, NEVER
    assert check_march_args(20, 1, 1e-2, None, 1000, 0) == (20, 1, 1e-2, NEVER, 1000, 0)
    assert check_march_args(5, 5, -1, -1, 2, 2) == (5, 5, -1.0, -1.0, 2, 2)
    for bad in (dict(max_inner=0), dict(min_inner=0), dict(min_inner=6), dict(max_levels=0), dict(keep=-1), dict(tol=float("nan")),
                dict(abs_tol=float("inf")), dict(max_inner=2.5), dict(keep=True)):
        args = dict(max_inner=5, min_inner=1, tol=1e-2, abs_tol=None, max_levels=4, keep=0)
        args.update(bad)
        with pytest.raises(ValueError):
            check_march_args(**args)
    check_step_args("list", {})
    check_step_args(False, dict(accum_steps=1, world_size=1, distributed=False, want_outputs=True, max_grad_norm=1.0))
    for mode, kw, what in ((True, {}, "use_graph"), ("list", dict(accum_steps=2), "accum_steps"),
                           ("list", dict(world_size=2), "data parallelism"), (False, dict(distributed=True), "data parallelism"),
                           ("list", dict(want_outputs=False), "want_outputs")):
        with pytest.raises(ValueError, match=what):
            check_step_args(mode, kw)
        with pytest.raises(ValueError, match=what):
            MarchStep(None, None, use_graph=mode, **kw)                    # refused before the model or a device is looked at
    with pytest.raises(ValueError, match="min_inner"):
        MarchStep(None, None, max_inner=3, min_inner=4)
    ms = MarchStep.__new__(MarchStep)
    with pytest.raises(RuntimeError, match="device owns the time advance"):
        ms.advance_time()
    with pytest.raises(RuntimeError, match="one batch"):
        ms.set_batch(None)
    with pytest.raises(ValueError, match="accum_steps"):
        ms.accum_steps = 4
    assert ms.accum_steps == 1


class _NotingLib:
    """Stands in for the library: notes (entry point, arguments) and returns GFV_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _fake_step(monkeypatch):
    from gfv import lib as L
    noting = _NotingLib()
    monkeypatch.setattr(L, "load", lambda raw=False: noting)
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    t = lambda n: torch.zeros(n)
    guard = types.SimpleNamespace(active=True, guard=t(8), segs=t(2), n_seg=1, n_elems=4, ws=t(4))
    ema = types.SimpleNamespace(e=t(4), rec=t(8))
    accum = types.SimpleNamespace(rec=t(8), acc=t(4))
    return noting, (t(4), t(4), t(4), t(4), 4, t(16), t(8)), guard, ema, accum


def test_hold_takes_the_accumulation_records_place_and_issues_no_accumulate_launch(monkeypatch):
    from gfv.optstep import optimizer_launches
    noting, base, guard, ema, accum = _fake_step(monkeypatch)
    hold = torch.zeros(16, dtype=torch.int32)
    names = lambda: [n for n, _ in noting.calls]
    # hold=None: exactly what was issued before the argument existed
    optimizer_launches(*base)
    optimizer_launches(*base, guard=guard)
    optimizer_launches(*base, guard=guard, accum=accum, loss=torch.zeros(1))
    optimizer_launches(*base, ema=ema)
    assert names() == ["gfv_adam_step_dev", "gfv_grad_guard_dev", "gfv_adam_step_guarded_dev", "gfv_grad_accum_dev",
                       "gfv_grad_guard_accum_dev", "gfv_adam_step_accum_dev", "gfv_adam_step_ema_dev"]
    assert noting.calls[-1][1][9] is None                                  # no record where accum's goes
    noting.calls.clear()
    optimizer_launches(*base, hold=hold)
    optimizer_launches(*base, guard=guard, hold=hold)
    optimizer_launches(*base, guard=guard, ema=ema, hold=hold)
    assert names() == ["gfv_adam_step_accum_dev", "gfv_grad_guard_accum_dev", "gfv_adam_step_accum_dev", "gfv_grad_guard_accum_dev",
                       "gfv_adam_step_ema_dev"]
    rec = hold.data_ptr()
    assert noting.calls[0][1][8] == rec and noting.calls[0][1][7] is None  # (p, g, m, v, n, state, hyper, guard, accum, stream)
    assert noting.calls[1][1][7] == rec                                    # the guard's accum argument
    assert noting.calls[2][1][7] == guard.guard.data_ptr() and noting.calls[2][1][8] == rec
    assert noting.calls[4][1][9] == rec
    with pytest.raises(ValueError, match="hold= and accum="):
        optimizer_launches(*base, accum=accum, hold=hold)


def test_history_decode_on_hand_made_words():
    from gfv import lib as L
    from gfv.march import decode_history
    B = 2
    words = np.zeros((2, L.MARCH_HEAD + L.MARCH_GRAPH * B), dtype=np.int32)
    per0 = np.arange(1, 17, dtype=f32).reshape(B, 8) / f32(8)
    per1 = np.array([[np.nan, 1e-30, 3e38, -0.0, 5, 6, 7, 8], [9, 10, 11, 12, 13, 14, 15, np.inf]], dtype=f32)
    words[0, 0:4] = (0, 7, L.MARCH_CONVERGED, 7)
    words[1, 0:4] = (1, 20, L.MARCH_CONVERGED | L.MARCH_CAPPED, 27)
    words[0, L.MARCH_HEAD:] = per0.reshape(-1).view(np.int32)
    words[1, L.MARCH_HEAD:] = per1.reshape(-1).view(np.int32)
    rows = decode_history(torch.from_numpy(words), B)
    assert [(r["level"], r["inner"], r["converged"], r["capped"], r["seen"]) for r in rows] == [(0, 7, True, False, 7),
                                                                                                 (1, 20, True, True, 27)]
    for r, per in zip(rows, (per0, per1)):
        got = np.concatenate([r["losses"].numpy(), r["r0"].numpy()[:, None], r["r"].numpy()[:, None],
                              r["update_norm"].numpy()[:, None], r["field_norm"].numpy()[:, None]], axis=1)
        assert got.dtype == f32 and got.tobytes() == per.tobytes()         # bit copies, NaN and -0 included
    assert decode_history(torch.zeros((0, 24), dtype=torch.int32), B) == []
    with pytest.raises(ValueError, match="24 words"):
        decode_history(torch.zeros((1, 16), dtype=torch.int32), B)


# ---- the rule, the reference alone ------------------------------------------------------------------------------------------------
W = (2.0, 0.5, 1.0)   # w_cont, w_mom, w_press


def _ref(**kw):
    """Two graphs of 3 + 2 rows, one chunk each."""
    args = dict(max_inner=4, min_inner=1, tol=0.5, abs_tol=-1.0, target=3, max_levels=3, keep=0)
    args.update(kw)
    xb = np.arange(60, dtype=f32).reshape(5, 12)
    return R.MarchRef(xb, [0, 3], [3, 5], [0, 1, 2], W, **args)


def _losses(r_a, r_b):
    """Losses whose weighted residuals are r_a and r_b exactly (press alone, weight 1)."""
    return np.array([[0, 0, 0, r_a], [0, 0, 0, r_b]], dtype=f32)


def _uvp(seed):
    return np.random.default_rng(seed).standard_normal((5, 3)).astype(f32)


def test_the_residual_is_the_fp32_statement_of_the_training_loss():
    l = np.array([[1e-3, 2e-4, 3e-4, 5e-2], [7.0, 0.25, 0.125, 3.0]], dtype=f32)
    r = R.residual(l, *W)
    want = [f32(f32(f32(f32(1.0) * a[3] + f32(2.0) * a[0]) + f32(0.5) * a[1]) + f32(0.5) * a[2]) for a in l]
    assert r.dtype == f32 and r.tolist() == [float(v) for v in want]
    assert r[1] == f32(3.0 + 14.0 + 0.125 + 0.0625)


def test_an_early_convergence_is_held_back_by_min_inner():
    m = _ref(min_inner=3)
    assert m.launch(_uvp(1), _losses(8.0, 4.0)) == "open" and m.r0.tolist() == [8.0, 4.0]
    assert m.launch(_uvp(2), _losses(1.0, 1.0)) == "open"                  # converged at k = 2 < min_inner
    assert m.rec[R.INNER] == 2 and m.rec[R.LEVEL] == 0 and (m.x_backup == np.arange(60, dtype=f32).reshape(5, 12)).all()
    u = _uvp(3)
    assert m.launch(u, _losses(1.0, 1.0)) == "latched"
    assert m.hist[0, 0:4].tolist() == [0, 3, R.CONVERGED, 3]
    assert m.rec[R.INNER] == 0 and m.rec[R.LEVEL] == 1 and m.rec[R.DONE] == 0 and m.rec[R.APPLY] == 1
    assert (m.x_backup[:, 0:3] == u).all() and (m.x_backup[:, 3:] == np.arange(60, dtype=f32).reshape(5, 12)[:, 3:]).all()
    assert (m.x == m.x_backup).all()
    per = m.hist[0, R.HEAD:].view(f32).reshape(2, 8)
    assert per[:, 4].tolist() == [8.0, 4.0] and per[:, 5].tolist() == [1.0, 1.0] and per[:, 3].tolist() == [1.0, 1.0]


def test_one_graph_converged_and_one_not_is_no_latch():
    m = _ref()
    assert m.launch(_uvp(1), _losses(8.0, 4.0)) == "open"
    assert m.launch(_uvp(2), _losses(4.0, 2.5)) == "open"                  # 4 <= 0.5 * 8, but 2.5 > 0.5 * 4
    assert m.launch(_uvp(3), _losses(4.0, 2.0)) == "latched"               # the bound itself converges: <=
    assert m.hist[0, 0:4].tolist() == [0, 3, R.CONVERGED, 3]


def test_the_cap_ends_a_level_that_does_not_converge():
    m = _ref()
    for k in range(3):
        assert m.launch(_uvp(k), _losses(8.0, 4.0)) == "open"
    assert m.launch(_uvp(9), _losses(8.0, 4.0)) == "latched"
    assert m.hist[0, 0:4].tolist() == [0, 4, R.CAPPED, 4]
    m = _ref(max_inner=2, min_inner=2)
    assert m.launch(_uvp(1), _losses(8.0, 4.0)) == "open"
    assert m.launch(_uvp(2), _losses(1.0, 1.0)) == "latched"
    assert m.hist[0, 2] == R.CONVERGED | R.CAPPED                          # both exits at once


def test_a_nan_never_converges_and_negative_tolerances_never_fire():
    m = _ref()
    assert m.launch(_uvp(1), _losses(8.0, np.nan)) == "open"               # r0 = (8, NaN)
    assert np.isnan(m.r0[1]) and m.r0[0] == 8.0
    assert m.launch(_uvp(2), _losses(1.0, np.nan)) == "open"               # NaN <= anything is false
    assert m.launch(_uvp(3), _losses(1.0, 1.0)) == "open"                  # 1 <= 0.5 * NaN is false too: graph 1 cannot converge
    assert m.launch(_uvp(4), _losses(1.0, 1.0)) == "latched"
    assert m.hist[0, 0:4].tolist() == [0, 4, R.CAPPED, 4]                  # the cap alone, though graph 0 had converged
    # ... unless the absolute tolerance takes over for the graph whose r0 is NaN
    assert R.converged(R.residual(_losses(1.0, 1.0), *W), m.hist[0, R.HEAD:].view(f32).reshape(2, 8)[:, 4], 0.5, 10.0).tolist() \
        == [True, True]
    assert R.converged(np.array([np.nan, np.inf], dtype=f32), np.array([1.0, 1.0], dtype=f32), 0.5, 10.0).tolist() == [False, False]
    m = _ref(tol=-1.0, abs_tol=-1.0)
    for k in range(3):
        assert m.launch(_uvp(k), _losses(0.0, 0.0)) == "open"              # 0 <= -1 * 0 = -0 would be true: a negative tol is off
    assert m.launch(_uvp(9), _losses(0.0, 0.0)) == "latched" and m.hist[0, 2] == R.CAPPED


def test_abs_tol_alone():
    m = _ref(tol=-1.0, abs_tol=0.75, min_inner=1)
    assert m.launch(_uvp(1), _losses(8.0, 4.0)) == "open"
    assert m.launch(_uvp(2), _losses(0.75, 0.76)) == "open"
    assert m.launch(_uvp(3), _losses(0.75, 0.75)) == "latched"
    assert m.hist[0, 0:4].tolist() == [0, 3, R.CONVERGED, 3]
    m = _ref(tol=-1.0, abs_tol=100.0)
    assert m.launch(_uvp(1), _losses(8.0, 4.0)) == "latched"               # the first iteration may end a level (min_inner = 1)
    assert m.hist[0, 0:4].tolist() == [0, 1, R.CONVERGED, 1] and m.r0.tolist() == [8.0, 4.0]


def test_the_freeze_at_the_target():
    m = _ref(max_inner=1, target=2, keep=2)
    u0, u1 = _uvp(1), _uvp(2)
    assert m.launch(u0, _losses(8.0, 4.0)) == "latched" and m.rec[R.DONE] == 0
    assert m.launch(u1, _losses(7.0, 3.0)) == "latched" and m.rec[R.DONE] == 1 and m.rec[R.LEVEL] == 2
    assert (m.snap[0] == u0).all() and (m.snap[1] == u1).all()
    before = (m.rec.copy(), m.r0.copy(), m.hist.copy(), m.x_backup.copy(), m.x.copy(), m.snap.copy())
    for k in range(3):
        assert m.launch(_uvp(5 + k), _losses(1.0, 1.0)) == "held"
    want = before[0].copy()
    want[R.APPLY], want[R.HELD] = 0, 3
    assert (m.rec == want).all()
    for a, b in zip(before[1:], (m.r0, m.hist, m.x_backup, m.x, m.snap)):
        assert a.tobytes() == b.tobytes()
    m.rec[R.TARGET], m.rec[R.DONE] = 3, 0                                  # what a later run() writes
    assert m.launch(_uvp(8), _losses(1.0, 1.0)) == "latched" and m.rec[R.LEVEL] == 3 and m.rec[R.DONE] == 1
    assert m.hist[2, 0:4].tolist() == [2, 1, R.CAPPED, 3]                  # held launches are not `seen`
