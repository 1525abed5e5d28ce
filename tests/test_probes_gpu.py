"""Probes on the device (gfv/probes.py, csrc/probes.hip; include/gfv.h gfv_probe_sample).

1. `gfv_probe_sample` alone on synthetic tables (0, 1, 63, 64, 65 and 200 entries per probe; 1, 4 and 5 probes: the workgroup's edge),
   keep = 4, the clock script of the window tests past a ring wrap: record and `hist_clock` as integers, the values under the bound
   (nnz_p + 16) 2^-53 sum |w| |phi|, two launches on the same inputs the same bits, the inputs unchanged, a poisoned ring untouched by
   launches that do not sample; the bound rejects a restatement that accumulates in fp32;
2. `sample()` on `cyl_b3` at 2nd order, 16 probes per graph with a rake behind each cylinder, against the restatement under
   `probes_ref.combined_bound`;
3. `Rollout` on `cyl_cavity_b2`, 12 steps, list mode and eager mode: the two histories bit for bit the same; fields and state bit for
   bit those of a run without probes; the same with `field_stats` and `wall_forces` beside it, whose rows stay bitwise too; every row
   bitwise `sample()` of the field captured after that step;
4. `set_window()` in the middle of a list-mode run holds from the next step with no new recording; `reset()` starts over;
5. `MarchStep` (the constants of tests/test_march_gpu.py): one row per completed level, none on held steps, the march bit for bit
   the march without probes;
6. the two known answers of tests/test_probes_cpu.py through `sample()`, within the same tolerances;
7. the refusals that need the device.
"""
import functools

import numpy as np
import pytest
import torch

import cases
import probes_ref as R
import test_fieldstats_gpu as TF
import test_probes_cpu as TC
import test_wallforce_gpu as TW
import wallforce_ref as W

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
STEPS = TF.STEPS
_same = TF._same
_dev = TW._dev
_record = TW._record
SCRIPT = TW.SCRIPT


def _launch(L, xb, dim, batch, ptr, node, w, P, clock, rec, hist, hclock, keep):
    ptr_of = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    return L.load().gfv_probe_sample(ptr_of(xb), ptr_of(dim), ptr_of(batch), ptr_of(ptr), ptr_of(node), ptr_of(w), P, ptr_of(clock),
                                     ptr_of(rec), ptr_of(hist), ptr_of(hclock), keep, L.stream_ptr())


# ---- 1. the launch alone, on synthetic tables --------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", [(65,), (0, 1, 63, 64), (200, 65, 0, 64, 1)])
def test_the_launch_alone_follows_the_reference_launch_by_launch(entries):
    from gfv import lib as L
    KEEP, N, B, P = 4, 300, 2, len(entries)
    rng = np.random.default_rng(20 + P)
    batch = np.sort(rng.integers(0, B, N)).astype(np.int32)
    dim = rng.uniform(0.5, 2.0, (B, 3)).astype(f32)
    ptr = np.concatenate(([0], np.cumsum(entries))).astype(np.int32)
    node = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in entries] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    w = rng.standard_normal((int(ptr[-1]), 3)) * 10.0 ** rng.uniform(-2.0, 1.0, (int(ptr[-1]), 3))
    assert node.min() >= 0 and node.max() < N and len(node) == len(w) == ptr[-1]
    ref = R.ProbesRef(ptr, node, w, dim, batch, KEEP, start=2, stride=2)
    POISON = -9.0
    ref.hist[:], ref.hist_clock[:] = POISON, -5                                                    # (stale rows: read only up to n)
    const = {"dim": _dev(dim), "batch": _dev(batch), "ptr": _dev(ptr), "node": _dev(node), "w": _dev(w)}
    state = [{"rec": _dev(ref.rec), "hist": torch.full((KEEP, P, 9), POISON, dtype=torch.float64, device="cuda"),
              "hclock": torch.full((KEEP,), -5, dtype=torch.int32, device="cuda")} for _ in range(2)]
    clock = torch.zeros(1, dtype=torch.int32, device="cuda")
    taken, rejected = 0, 0.0
    for i, (words, c, expect) in enumerate(SCRIPT):
        for name, v in (words or {}).items():
            idx = getattr(R, name)
            ref.rec[idx] = v
            for s in state:
                s["rec"][idx:idx + 1].copy_(torch.tensor([v], dtype=torch.int32))
        field = (rng.standard_normal((N, 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (N, 12))).astype(f32)
        xb = _dev(field)
        clock.copy_(torch.tensor([c], dtype=torch.int32))
        before = (state[0]["hist"].cpu().clone(), state[0]["hclock"].cpu().clone())
        for s in state:                                                                            # the same inputs, twice
            L.check(_launch(L, xb, const["dim"], const["batch"], const["ptr"], const["node"], const["w"], P, clock, s["rec"],
                            s["hist"], s["hclock"], KEEP), "gfv_probe_sample")
        torch.cuda.synchronize()
        what = f"entries {entries}, launch {i} (clock {c})"
        assert ref.launch(field, c) is expect, what
        a, b = state
        for k in a:
            assert _same(a[k], b[k]), (what, k)                                                    # the same bits, run after run
        assert a["rec"].cpu().numpy().tolist() == ref.rec.tolist(), (what, a["rec"].tolist(), ref.rec.tolist())
        assert a["hclock"].cpu().numpy().tolist() == ref.hist_clock.tolist(), what
        assert _same(xb, field) and int(clock[0]) == c, what                                       # inputs are inputs
        for k, v in (("dim", dim), ("batch", batch), ("ptr", ptr), ("node", node), ("w", w)):
            assert _same(const[k], v), (what, k)
        hist = a["hist"].cpu().numpy()
        if expect:
            row = taken % KEEP
            taken += 1
            nnz = np.asarray(entries, dtype=f64)[:, None]
            bound = (nnz + 16.0) * R.U * ref.mag[row]
            err = np.abs(hist[row] - ref.hist[row])
            print(f"{what}: largest error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3g}")
            assert (err <= bound).all(), (what, err, bound)
            assert (hist[row][np.asarray(entries) == 0] == 0).all()                               # a probe without entries: zeros
            other = [r for r in range(KEEP) if r != row]
            assert _same(hist[other], before[0].numpy()[other]), what
            # the bound REJECTS a restatement that multiplies and accumulates in fp32
            low, _ = R.dot_rows(ptr, node, w, ref.phi(field), dtype=f32)
            rejected = max(rejected, float((np.abs(low - ref.hist[row])[bound > 0] / bound[bound > 0]).max()))
        else:
            assert _same(hist, before[0]) and _same(a["hclock"], before[1]), what                  # the poison and the rows stay
    assert taken == 6 and int(state[0]["rec"][R.N]) == 6
    assert ref.rows()[0].tolist() == [8, 12, 14, 16]
    print(f"fp32 accumulation: largest error / bound {rejected:.3g}")
    assert rejected > 1e3


# ---- 2. sample() against the restatement -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(which, order="2nd"):
    """-> (CPU graphs, device graphs, CPU plan, the restatement's arrays).  Once."""
    cpu, plan, m = TC.setup(which, order)
    dev = tuple(g.clone().to("cuda") for g in cpu)
    dev[0].norm_uvp, dev[0].norm_global = True, True
    return cpu, dev, plan, m


def test_sample_on_three_graphs_against_the_restatement():
    from gfv import probes as PR
    _, graphs, plan, m = _case("cyl_b3")
    pts, gr = TC.accepted_points("cyl_b3", 10, 1300)
    pts, gr = list(pts), list(gr)
    for b in range(3):                                                                             # a rake behind each cylinder
        rake = PR.line((0.3, 0.12), (0.3, 0.28), 6).numpy()
        pts += list(rake)
        gr += [b] * 6
    pts = np.array(pts)
    assert len(gr) == 48
    rng = np.random.default_rng(77)
    field = (rng.standard_normal((m["N"], 3)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 3))).astype(f32)
    got = PR.sample(graphs, _dev(field), pts, gr)
    assert tuple(got["value"].shape) == (48, 3) and tuple(got["gradient"].shape) == (48, 3, 2) and got["value"].dtype == torch.float64
    cell, outside, _ = PR.locate(plan, pts, gr)
    assert got["cell"].tolist() == cell.tolist() == [R.locate(m, x, b)[0] for x, b in zip(pts, gr)]
    assert _same(got["outside"], outside)
    t = PR.build_tables(plan, pts, cell)
    _, mag = R.dot_rows(t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy(), W.node_values(m, field))
    nnz = np.diff(t.pw_ptr.numpy())
    rows = torch.cat((got["value"][:, :, None], got["gradient"]), 2).numpy().reshape(48, 9)
    worst = 0.0
    for p in range(48):
        val, g = R.value_gradient(m, int(cell[p]), pts[p], field)
        want = np.concatenate((val[:, None], g), 1).reshape(-1)
        bound = R.combined_bound(m, int(cell[p]), pts[p], field, int(nnz[p]), mag[p])
        err = np.abs(rows[p] - want)
        assert (err <= bound).all(), (p, err, bound)
        assert (np.abs(want) > 1e4 * bound).any()                                                  # the bound decides something
        worst = max(worst, float((err / bound).max()))
    print(f"sample() against the restatement: largest error / bound {worst:.3g}")


# ---- 3. Rollout ----------------------------------------------------------------------------------------------------------------------
WHICH = "cyl_cavity_b2"


@functools.lru_cache(maxsize=None)
def _points():
    """A rake behind the cylinder of graph 0, two points up- and downstream, the centreline of the cavity (graph 1)."""
    from gfv import probes as PR
    pts = torch.cat((PR.line((0.32, 0.1), (0.32, 0.3), 5), torch.tensor([[0.1, 0.2], [1.5, 0.21]], dtype=torch.float64),
                     PR.line((0.5, 0.04), (0.5, 0.96), 6)))
    return pts, [0] * 7 + [1] * 6


def _probes(**kw):
    from gfv.probes import Probes
    pts, gr = _points()
    return Probes(pts, graph=gr, **dict(dict(keep=16), **kw))


@functools.lru_cache(maxsize=None)
def _with_probes(mode, others):
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    pr = _probes()
    extra = dict(field_stats=FieldStats(start=TF.START, stride=TF.STRIDE), wall_forces=TW._forces()) if others else {}
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, launch_mode=mode, probes=pr, **extra)
    assert r.probes is pr and r._followers == [f for f in (r.field_stats, r.wall_forces, pr) if f is not None]
    for _ in range(STEPS):
        outs = r.step()                                                                            # (no synchronisation in the loop)
    end = TF._end_state(r, outs)
    if mode == "cmd_list":
        st = r._lists.stats()                              # (the warm-up steps are eager: both launch paths carry the launch)
        assert st["recorded"] == 1 and st["replayed"] >= 6 and st["eager"] >= 2, st
    beside = (r.field_stats.raw(), r.wall_forces.raw()) if others else None
    return pr.raw(), pr.read(), end, beside


@functools.lru_cache(maxsize=None)
def _sampled():
    """sample() on the field a run WITHOUT probes left after every step: rows [STEPS, P, 9].  Once."""
    from gfv import probes as PR
    fields, _, _ = TF._plain(WHICH)
    graphs = TF._graphs(WHICH)
    pts, gr = _points()
    out = []
    for f in fields:
        s = PR.sample(graphs, _dev(f), pts, gr)
        out.append(torch.cat((s["value"][:, :, None], s["gradient"]), 2).numpy().reshape(len(gr), 9))
    return np.stack(out)


def test_rollout_history_is_sample_of_every_field_and_the_run_is_unchanged():
    from gfv import probes as PR
    fields, plain_end, N = TF._plain(WHICH)
    want = _sampled()
    P = len(_points()[1])
    assert want.shape == (STEPS, P, 9) and np.isfinite(want).all() and np.abs(want[:, :, 0]).min() > 0
    raws = {}
    for mode in ("cmd_list", "eager"):
        for others in (False, True):
            raw, h, end, beside = _with_probes(mode, others)
            rec, hist, hclock = raw
            what = (mode, others)
            assert rec.tolist() == [1, 1, -1, STEPS, STEPS, 0, 1, 0], (what, rec.tolist())
            assert hclock[:STEPS].tolist() == list(range(1, STEPS + 1))
            assert h["n"] == STEPS and h["clock"].tolist() == list(range(1, STEPS + 1))
            assert _same(hist[:STEPS].numpy(), want), what                                         # bitwise sample() of every field
            for k, v in plain_end.items():                                                         # the run itself is the run without
                assert _same(end[k], v), (what, k)
            raws[what] = raw
            if others:                                                                             # the neighbours' rows stay bitwise
                assert all(_same(a, b) for a, b in zip(beside[0], TF._with_stats(WHICH, mode)[0])), what
                assert all(_same(a, b) for a, b in zip(beside[1], TW._with_forces(mode)[0])), what
    first = raws[("cmd_list", False)]
    assert all(_same(a, b) for raw in raws.values() for a, b in zip(raw, first))
    # what read() hands out
    h = _with_probes("eager", False)[1]
    pts, gr = _points()
    _, _, plan, m = _case(WHICH)
    assert tuple(h["value"].shape) == (STEPS, P, 3) and tuple(h["gradient"].shape) == (STEPS, P, 3, 2)
    r = want.reshape(STEPS, P, 3, 3)
    assert _same(h["value"].numpy(), np.ascontiguousarray(r[..., 0])) and _same(h["gradient"].numpy(), np.ascontiguousarray(r[..., 1:3]))
    assert _same(h["points"], pts) and h["graph"].tolist() == gr and h["cell"].tolist() == [R.locate(m, x, b)[0] for x, b in zip(pts.numpy(), gr)]
    assert _same(h["uvp_dim"].numpy(), m["uvp_dim"][gr]) and (h["outside"].numpy() <= 0).all()
    assert _same(PR.vorticity(h).numpy(), r[:, :, 1, 1] - r[:, :, 0, 2]) and _same(PR.divergence(h).numpy(), r[:, :, 0, 1] + r[:, :, 1, 2])
    # ... and a row is the restatement's, under its bound
    t = PR.build_tables(plan, pts, h["cell"])
    nnz = np.diff(t.pw_ptr.numpy())
    worst = 0.0
    for k in (0, STEPS - 1):
        _, mag = R.dot_rows(t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy(), W.node_values(m, fields[k]))
        for p in range(P):
            val, g = R.value_gradient(m, int(h["cell"][p]), pts[p].numpy(), fields[k])
            bound = R.combined_bound(m, int(h["cell"][p]), pts[p].numpy(), fields[k], int(nnz[p]), mag[p])
            err = np.abs(want[k, p] - np.concatenate((val[:, None], g), 1).reshape(-1))
            assert (err <= bound).all(), (k, p, err, bound)
            worst = max(worst, float((err / bound).max()))
    print(f"rollout rows against the restatement: largest error / bound {worst:.3g}")


# ---- 4. the window moves under a recorded list ------------------------------------------------------------------------------------
def test_set_window_holds_from_the_next_step_without_a_new_recording_and_reset_starts_over():
    from gfv.rollout import Rollout
    want = _sampled()
    pr = _probes()
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, probes=pr)
    rec = _record()
    clocks, k = [], 0

    def steps(n):
        nonlocal k
        for _ in range(n):
            r.step()
            k += 1
            if R.take(rec, k):
                clocks.append(k)
                rec[R.N] += 1
            rec[R.LAST] = k

    def check(what):
        got, hist, hclock = pr.raw()
        assert got.tolist() == rec.tolist(), (what, got.tolist(), rec.tolist())
        assert hclock[:len(clocks)].tolist() == clocks, what
        assert _same(hist[:len(clocks)].numpy(), want[[c - 1 for c in clocks]]), what

    steps(5)                                                                                       # the warm-up, the recording, a replay
    replayed = r._lists.stats()["replayed"]
    assert r._lists.stats()["recorded"] == 1 and replayed >= 1 and pr.count() == 5
    check("every step")
    pr.set_window(stride=3)                                                                        # clocks 1, 4, 7, 10: the next is 7
    rec[R.STRIDE] = 3
    steps(3)
    assert pr.count() == 6 and clocks[-1] == 7
    check("stride 3")
    pr.set_window(enabled=False)
    rec[R.ENABLED] = 0
    steps(1)
    pr.set_window(enabled=True, stop=10)
    rec[R.ENABLED], rec[R.STOP] = 1, 10
    steps(2)                                                                                       # 10: on the stride, but stop; 11: a miss
    assert pr.count() == 6
    check("paused, then stopped")
    assert r._lists.stats()["recorded"] == 1 and r._lists.stats()["replayed"] == replayed + 6      # nothing was recorded again
    r.reset()                                                                                      # the owner's: the probes start over
    assert pr.count() == 0 and pr.raw()[0].tolist()[R.LAST] == -1 and pr.read()["clock"].shape == (0,)
    assert tuple(pr.read()["value"].shape) == (0, pr.P, 3)
    rec[R.LAST], rec[R.N] = -1, 0
    clocks.clear()
    k = 0
    steps(5)
    assert pr.count() == 2 and clocks == [1, 4]
    check("after reset")
    assert r._lists.stats()["recorded"] == 1


# ---- 5. MarchStep ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march_points():
    """Centroids of a few cells of the polygon mesh (its extent is the mesh's own business)."""
    cpu = TF._cpu_graphs("poly")
    from gfv.plan import build_plan
    plan = build_plan(*cpu)
    return plan.centroid[:: max(1, plan.C // 6)].to(torch.float64).clone()


@functools.lru_cache(maxsize=None)
def _march(ahead):
    from gfv.march import MarchStep
    from gfv.probes import Probes
    pr = Probes(_march_points(), keep=8)                                                           # B == 1: graph=None
    ms = MarchStep(TF._model(), TF._march_graphs(), lr=TF.LR, use_graph="list", tol=TF.TOL, max_inner=TF.MAX_INNER, max_levels=8,
                   keep=3, probes=pr)
    assert ms.probes is pr and ms._followers == [pr] and "probes" not in ms.state_dict()
    rows = ms.run(levels=TF.LEVELS, max_ahead=ahead)
    state, held = TF._march_state(ms), ms.stats()["held"]
    snaps = [ms.snapshot(level).cpu().numpy() for level in range(TF.LEVELS)]
    raw, h = pr.raw(), pr.read()
    for _ in range(2):
        ms.step()                                                                                  # held for certain
    assert ms.stats()["held"] == held + 2
    return rows, state, snaps, raw, h, pr.raw()


def test_march_adds_one_row_per_completed_level_and_none_on_held_steps():
    from gfv import probes as PR
    plain_rows, plain_state, plain_snaps, *_ = TF._march(None)
    assert [r["inner"] for r in plain_rows] == [4, 5, 5]
    pts = _march_points()
    raws = {}
    for ahead in (64, 0):
        rows, state, snaps, raw, h, raw_held = _march(ahead)
        assert [r["inner"] for r in rows] == [4, 5, 5]
        assert h["n"] == 3 and h["clock"].tolist() == [1, 2, 3] and h["graph"].tolist() == [0] * len(pts)     # one per level: not 14
        assert raw[0].tolist() == [1, 1, -1, 3, 3, 0, 1, 0]
        assert all(_same(a, b) for a, b in zip(raw, raw_held))                                     # held steps add nothing
        graphs = TF._march_graphs()
        want = []
        for s in snaps:
            got = PR.sample(graphs, _dev(s), pts)
            want.append(torch.cat((got["value"][:, :, None], got["gradient"]), 2).numpy().reshape(len(pts), 9))
        assert _same(raw[1][0:3].numpy(), np.stack(want)) and np.abs(np.stack(want)[:, :, 0]).min() > 0
        assert state.keys() == plain_state.keys()
        for k in state:
            assert _same(state[k], plain_state[k]), (ahead, k)                                     # the march without probes
        TF._same_rows(rows, plain_rows)
        assert all(_same(a, b) for a, b in zip(snaps, plain_snaps))
        raws[ahead] = raw
    assert all(_same(a, b) for a, b in zip(raws[64], raws[0]))


# ---- 6. the known answers, on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", TC.CASES3)
@pytest.mark.parametrize("quadratic", [False, True], ids=["linear", "quadratic"])
def test_known_answers_through_sample(which, quadratic):
    from gfv import probes as PR
    _, graphs, plan, m = _case(which)
    k = TC.known_case(which, quadratic)
    got = PR.sample(graphs, _dev(k["field"]), k["points"], k["graph"] if m["B"] > 1 else None)
    assert got["cell"].tolist() == k["cell"]
    t = PR.build_tables(plan, k["points"], got["cell"])
    _, mag = R.dot_rows(t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy(), W.node_values(m, k["field"]))
    room = ((np.diff(t.pw_ptr.numpy())[:, None] + 16.0) * R.U * mag).reshape(-1, 3, 3)            # the device's double arithmetic
    TC.check_known(k, got["value"].numpy(), got["gradient"].numpy(), room[:, :, 0], room[:, :, 1:3].max(2), f"{which} sample()")
    if quadratic:
        assert (np.abs(k["correction"]) > 100.0 * (k["tol_value"] + room[:, :, 0])).any()


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gfv import lib as L
    from gfv import probes as PR
    from gfv.plan import get_plan
    from gfv.probes import Probes
    from gfv.rollout import Rollout
    model = TF._model()
    pts, gr = _points()
    r0 = Rollout(model, TF._graphs(WHICH), max_steps=4, launch_mode="eager")
    assert r0.probes is None and r0._followers == []                                               # the default: nothing attached
    pr = _probes(start=2)
    with pytest.raises(ValueError, match="anderson"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, anderson=2, probes=pr)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        Rollout(model, tuple(g.clone() for g in TF._cpu_graphs(WHICH)), max_steps=4, probes=pr)    # CPU graphs
    with pytest.raises(ValueError, match="Probes"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, probes=dict(points=pts))
    with pytest.raises(ValueError, match=r"point 0 \(0.2, 0.2\) of graph 0"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, probes=Probes([[0.2, 0.2], [1.0, 0.2]], graph=0))       # inside the cylinder
    with pytest.raises(ValueError, match="graph=None needs a batch of one graph"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, probes=Probes(pts))
    pr.check_free()                                                                                # a constructor that raised attached nothing
    graphs = TF._graphs(WHICH)
    plan = get_plan(graphs)
    with pytest.raises(ValueError, match="GPU"):
        pr.attach(object(), graphs, plan, torch.zeros(plan.N, 12), torch.zeros(1, dtype=torch.int32))          # a CPU node state
    pr.check_free()
    assert pr.rec is None and pr.tables is None
    r = Rollout(model, graphs, max_steps=4, launch_mode="eager", probes=pr)
    with pytest.raises(ValueError, match="already attached"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, probes=pr)                                  # one owner per object
    assert not any(v is r for v in vars(pr).values())                                              # no reference back to the owner
    r.step()
    assert pr.count() == 0 and pr.raw()[0].tolist()[R.LAST] == 1
    h = pr.read()
    assert h["n"] == 0 and tuple(h["value"].shape) == (0, len(gr), 3) and tuple(h["gradient"].shape) == (0, len(gr), 3, 2)
    r.step()
    assert pr.count() == 1 and pr.read()["clock"].tolist() == [2]
    with pytest.raises(ValueError, match="rows"):
        PR.sample(graphs, torch.zeros(plan.N + 1, 3, device="cuda"), pts, gr)
    # the entry point: GFV_ERR_ARG, nothing launched
    t = pr.tables
    clock, rec = torch.ones(1, dtype=torch.int32, device="cuda"), _dev(_record())
    xb = torch.zeros((plan.N + 1, 12), dtype=torch.float32, device="cuda")
    w1 = torch.zeros(t.pw_w.numel() + 1, dtype=torch.float64, device="cuda")
    ERR = -1

    def args(**over):
        a = dict(xb=xb, dim=plan.uvp_dim, batch=plan.batch, ptr=t.pw_ptr, node=t.pw_node, w=t.pw_w, P=pr.P, clock=clock, rec=rec,
                 hist=pr.hist, hclock=pr.hist_clock, keep=pr.keep)
        a.update(over)
        return a

    before = pr.raw()
    assert _launch(L, **args()) == 0                                                               # (the arguments as they stand: accepted)
    torch.cuda.synchronize()
    assert int(rec[R.N]) == 1
    rec.copy_(_dev(_record()))
    pr.hist.copy_(before[1].cuda())
    pr.hist_clock.copy_(before[2].cuda())
    for over in ([dict([(k, None)]) for k in ("xb", "dim", "batch", "ptr", "node", "w", "clock", "rec", "hist", "hclock")]
                 + [dict(P=0), dict(P=-1), dict(keep=0), dict(keep=-3), dict(xb=xb.data_ptr() + 4), dict(xb=xb.data_ptr() + 8),
                    dict(w=w1.data_ptr() + 4), dict(hist=pr.hist.data_ptr() + 4)]):
        assert _launch(L, **args(**over)) == ERR, over
    torch.cuda.synchronize()
    assert rec.cpu().numpy().tolist() == _record().tolist()
    assert all(_same(a, b) for a, b in zip(pr.raw(), before))
