"""Flow integrals on the device (gfv/integrals.py, csrc/integrals.hip; include/gfv.h gfv_flow_integrals).

1. `gfv_flow_integrals` alone on synthetic tables (cells per graph (65,), (0, 1, 63, 64) and (200, 65, 0, 64, 1); polygons of 3 to 9
   incidences with random vectors, areas, boundary kinds and uvp_dim), keep = 4, the clock script of the window tests past a ring
   wrap: record and `hist_clock` as integers, every column under `integrals_ref.bound`, two launches on the same inputs the same bits
   (`cell_out` included), the inputs unchanged, a poisoned ring and a poisoned `cell_out` untouched by launches that do not sample,
   `cell_out = NULL` accepted; the bound rejects a restatement that forms and sums the terms in fp32;
2. `evaluate(fields=True)` on `cyl_b3` at a seeded random field against the restatement under the same bound, and at the known
   answers of tests/test_integrals_cpu.py within its tolerances;
3. `Rollout` on `cyl_cavity_b2`, 12 steps, list mode and eager mode: the two histories bit for bit the same; fields and state bit for
   bit those of a run without integrals; the same with `field_stats`, `wall_forces` and `probes` beside it, whose raw state stays
   bitwise too; every row bitwise `evaluate()` of the field captured after that step;
4. `set_window()` in the middle of a list-mode run holds from the next step with no new recording; `reset()` starts over;
5. `MarchStep` (the constants of tests/test_march_gpu.py): one row per completed level, none on held steps, the march bit for bit
   the march without integrals;
6. the refusals that need the device, and every GFV_ERR_ARG case.
"""
import functools

import numpy as np
import pytest
import torch

import integrals_ref as R
import test_fieldstats_gpu as TF
import test_integrals_cpu as TC
import test_probes_gpu as TP
import test_wallforce_gpu as TW

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
STEPS = TF.STEPS
_same = TF._same
_dev = TW._dev
_record = TW._record
SCRIPT = TW.SCRIPT
NAMES = ("xb", "dim", "crow", "kface", "knode", "kS", "btype", "es", "er", "area", "beg", "end", "gptr", "nch", "C", "B", "clock", "rec",
         "partial", "hist", "hclock", "keep", "cell_out")


def _launch(L, **a):
    ptr_of = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    assert tuple(a) == NAMES
    return L.load().gfv_flow_integrals(*[ptr_of(a[k]) for k in NAMES], L.stream_ptr())


# ---- 1. the launch alone, on synthetic tables --------------------------------------------------------------------------------------
def _synthetic(cells_per_graph, seed):
    """A batch made for the launch only: per graph a handful of nodes and `cells` polygons of 3 to 9 incidences, every incidence
    with a face of its own between two random nodes of the graph (stored in a shuffled order), a random vertex, vector and kind."""
    rng = np.random.default_rng(seed)
    B = len(cells_per_graph)
    nodes = [max(4, n // 2 + 3) for n in cells_per_graph]
    noff = np.concatenate(([0], np.cumsum(nodes)))
    C = int(sum(cells_per_graph))
    n = rng.integers(3, 10, C)
    n[: min(C, 7)] = np.arange(3, 10)[: min(C, 7)]                                                 # every count occurs
    crow = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    Sg = int(crow[-1])
    gcell_ptr = np.concatenate(([0], np.cumsum(cells_per_graph))).astype(np.int64)
    kgraph = np.repeat(np.repeat(np.arange(B), cells_per_graph), n)
    pick = lambda: noff[kgraph] + rng.integers(0, 10 ** 6, Sg) % np.asarray(nodes)[kgraph]
    kface = rng.permutation(Sg).astype(np.int64)
    es, er = np.zeros(Sg, dtype=np.int64), np.zeros(Sg, dtype=np.int64)
    es[kface], er[kface] = pick(), pick()
    return {"B": B, "C": C, "N": int(noff[-1]), "crow": crow, "kface": kface, "knode": pick().astype(np.int64), "es": es, "er": er,
            "kS": (rng.standard_normal((Sg, 2)) * 0.1).astype(f32), "area": rng.uniform(0.5e-2, 2e-2, C).astype(f32),
            "btype": rng.integers(0, 4, Sg).astype(np.int32), "gcell_ptr": gcell_ptr, "batch": np.repeat(np.arange(B), nodes),
            "uvp_dim": rng.uniform(0.5, 2.0, (B, 3)).astype(f32)}


@pytest.mark.parametrize("cells_per_graph", [(65,), (0, 1, 63, 64), (200, 65, 0, 64, 1)])
def test_the_launch_alone_follows_the_reference_launch_by_launch(cells_per_graph):
    from gfv import lib as L
    KEEP = 4
    m = _synthetic(cells_per_graph, 30 + len(cells_per_graph))
    B, C = m["B"], m["C"]
    assert set(np.diff(m["crow"]).tolist()) <= set(range(3, 10)) and R.k_max(m) == 9
    beg, end, gptr = R.chunks(m["gcell_ptr"])
    assert (end - beg).tolist() == {1: [64, 1], 4: [1, 63, 64], 5: [64, 64, 64, 8, 64, 1, 64, 1]}[B]
    nch = len(beg)
    ref = R.FlowRef(m, KEEP, start=2, stride=2)
    POISON = -9.0
    ref.hist[:], ref.hist_clock[:] = POISON, -5                                                    # (stale rows: read only up to n)
    i32 = lambda a: _dev(np.asarray(a).astype(np.int32))
    const = {"dim": _dev(m["uvp_dim"]), "crow": i32(m["crow"]), "kface": i32(m["kface"]), "knode": i32(m["knode"]), "kS": _dev(m["kS"]),
             "btype": i32(m["btype"]), "es": i32(m["es"]), "er": i32(m["er"]), "area": _dev(m["area"]), "beg": _dev(beg),
             "end": _dev(end), "gptr": _dev(gptr)}
    kept = {k: v.cpu().clone() for k, v in const.items()}

    def fresh(cells):
        return {"rec": _dev(ref.rec), "partial": torch.full((nch, 12), 3.5, dtype=torch.float64, device="cuda"),
                "hist": torch.full((KEEP, B, 12), POISON, dtype=torch.float64, device="cuda"),
                "hclock": torch.full((KEEP,), -5, dtype=torch.int32, device="cuda"),
                "cell_out": torch.full((C, 2), POISON, dtype=torch.float64, device="cuda") if cells else None}

    state = [fresh(True), fresh(True), fresh(False)]                                               # the third: cell_out = NULL
    clock = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(99)
    taken, rejected, worst = 0, 0.0, 0.0
    for i, (words, c, expect) in enumerate(SCRIPT):
        for name, v in (words or {}).items():
            idx = getattr(R, name)
            ref.rec[idx] = v
            for s in state:
                s["rec"][idx:idx + 1].copy_(torch.tensor([v], dtype=torch.int32))
        field = (rng.standard_normal((m["N"], 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 12))).astype(f32)
        xb = _dev(field)
        clock.copy_(torch.tensor([c], dtype=torch.int32))
        before = {k: v.cpu().clone() for k, v in state[0].items()}
        for s in state:                                                                            # the same inputs, three times
            L.check(_launch(L, xb=xb, **const, nch=nch, C=C, B=B, clock=clock, rec=s["rec"], partial=s["partial"], hist=s["hist"],
                            hclock=s["hclock"], keep=KEEP, cell_out=s["cell_out"]), "gfv_flow_integrals")
        torch.cuda.synchronize()
        what = f"cells {cells_per_graph}, launch {i} (clock {c})"
        assert ref.launch(field, c) is expect, what
        a, b, null = state
        for k in a:
            assert _same(a[k], b[k]), (what, k)                                                    # the same bits, run after run
            assert k == "cell_out" or _same(a[k], null[k]), (what, k)                              # ... and without the cell fields
        assert a["rec"].cpu().numpy().tolist() == ref.rec.tolist(), (what, a["rec"].tolist(), ref.rec.tolist())
        assert a["hclock"].cpu().numpy().tolist() == ref.hist_clock.tolist(), what
        assert _same(xb, field) and int(clock[0]) == c, what                                       # inputs are inputs
        for k, v in kept.items():
            assert _same(const[k], v), (what, k)
        hist, cells = a["hist"].cpu().numpy(), a["cell_out"].cpu().numpy()
        if expect:
            row = taken % KEEP
            taken += 1
            bound = R.bound(m, ref.mag[row])
            err = np.abs(hist[row] - ref.hist[row])
            assert (err <= bound).all(), (what, err, bound)
            assert (hist[row][np.asarray(cells_per_graph) == 0] == 0).all()                       # a graph without a cell: zeros
            cb = R.cell_bound(m, ref.cell_mag)
            cerr = np.abs(cells - ref.cell_out)
            assert (cerr <= cb).all(), (what, cerr.max(), cb.max())
            ok = bound > 0
            worst = max(worst, float((err[ok] / bound[ok]).max()), float((cerr / cb).max()))
            other = [r for r in range(KEEP) if r != row]
            assert _same(hist[other], before["hist"].numpy()[other]), what
            # the bound REJECTS a restatement that forms and sums the terms in fp32
            low, _, _ = R.graph_rows(m, R.node_values(m, field), dtype=f32)
            rejected = max(rejected, float((np.abs(low - ref.hist[row])[ok] / bound[ok]).max()))
        else:
            for k in ("partial", "hist", "hclock", "cell_out"):                                    # the poison and the rows stay
                assert _same(a[k], before[k]), (what, k)
    assert taken == 6 and int(state[0]["rec"][R.N]) == 6
    assert ref.rows()[0].tolist() == [8, 12, 14, 16]
    print(f"cells {cells_per_graph}: largest error / bound {worst:.3g}; fp32 terms and sums: largest error / bound {rejected:.3g}")
    assert rejected > 1e3


# ---- 2. evaluate() against the restatement and the known answers -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(which):
    """-> (CPU graphs, device graphs, CPU plan, the restatement's arrays).  Once."""
    cpu, plan, m = TC.setup(which)
    dev = tuple(g.clone().to("cuda") for g in cpu)
    dev[0].norm_uvp, dev[0].norm_global = True, True
    return cpu, dev, plan, m


def _cells(e):
    return torch.stack((e["vorticity"], e["divergence"]), 1).numpy()


def test_evaluate_on_three_graphs_against_the_restatement():
    from gfv import integrals as FI
    _, graphs, plan, m = _case("cyl_b3")
    rng = np.random.default_rng(77)
    field = (rng.standard_normal((m["N"], 3)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 3))).astype(f32)
    e = FI.evaluate(graphs, _dev(field), fields=True)
    assert tuple(e["columns"].shape) == (3, 12) and e["columns"].dtype == torch.float64 and tuple(e["vorticity"].shape) == (m["C"],)
    phi = R.node_values(m, field)
    rows, mag, cell_out = R.graph_rows(m, phi)
    bound, cb = R.bound(m, mag), R.cell_bound(m, R.cell_terms(m, phi)[1])
    err, cerr = np.abs(e["columns"].numpy() - rows), np.abs(_cells(e) - cell_out)
    print(f"evaluate() against the restatement: largest error / bound {float((err / bound).max()):.3g} (columns), "
          f"{float((cerr / cb).max()):.3g} (cells)")
    assert (err <= bound).all() and (cerr <= cb).all()
    assert (np.abs(rows[:, [0, 1, 2, 3, 6, 10, 11]]) > 1e6 * bound[:, [0, 1, 2, 3, 6, 10, 11]]).all()      # the bound decides something
    plain = FI.evaluate(graphs, _dev(field))                                                       # without the cell fields: the same bits
    assert "vorticity" not in plain and _same(plain["columns"], e["columns"])
    c = e["columns"].numpy()
    assert _same(e["div_l2"].numpy(), np.sqrt(c[:, 3] / c[:, 0])) and _same(e["mean_pressure"].numpy(), c[:, 6] / c[:, 0])
    assert _same(e["vort_max"].numpy(), np.ascontiguousarray(c[:, 11])) and _same(e["inflow"].numpy(), np.ascontiguousarray(c[:, 7]))
    gp = m["gcell_ptr"]
    for b in range(3):                                                                             # a row's maxima ARE its cells'
        assert c[b, 10] == np.abs(_cells(e)[gp[b]:gp[b + 1], 1]).max() and c[b, 11] == np.abs(_cells(e)[gp[b]:gp[b + 1], 0]).max()


@pytest.mark.parametrize("which", TC.CASES3)
@pytest.mark.parametrize("name", list(TC.FIELDS))
def test_known_answers_through_evaluate(which, name):
    from gfv import integrals as FI
    _, graphs, _, m = _case(which)
    k = TC.linear_case(which, name)
    e = FI.evaluate(graphs, _dev(k["field"]), fields=True)
    phi = R.node_values(m, k["field"])
    _, mag, _ = R.graph_rows(m, phi)
    worst = TC.check_known(k, e["columns"].numpy(), _cells(e), R.bound(m, mag), R.cell_bound(m, R.cell_terms(m, phi)[1]),
                           f"{which} {name} evaluate()")
    print(f"{which} {name} evaluate(): largest error / tolerance {worst:.3g}")


# ---- 3. Rollout ----------------------------------------------------------------------------------------------------------------------
WHICH = "cyl_cavity_b2"


def _integrals(**kw):
    from gfv.integrals import FlowIntegrals
    return FlowIntegrals(**dict(dict(keep=16), **kw))


@functools.lru_cache(maxsize=None)
def _with_integrals(mode, others):
    """others: `field_stats`, `wall_forces` and `probes` beside it, and the cell fields kept."""
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    fi = _integrals(fields=others)
    extra = dict(field_stats=FieldStats(start=TF.START, stride=TF.STRIDE), wall_forces=TW._forces(), probes=TP._probes()) if others else {}
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, launch_mode=mode, integrals=fi, **extra)
    assert r.integrals is fi and r._followers == [f for f in (r.field_stats, r.wall_forces, fi, r.probes) if f is not None]
    for _ in range(STEPS):
        outs = r.step()                                                                            # (no synchronisation in the loop)
    end = TF._end_state(r, outs)
    if mode == "cmd_list":
        st = r._lists.stats()                              # (the warm-up steps are eager: both launch paths carry the launch)
        assert st["recorded"] == 1 and st["replayed"] >= 6 and st["eager"] >= 2, st
    beside = (r.field_stats.raw(), r.wall_forces.raw(), r.probes.raw()) if others else None
    return fi.raw(), fi.read(), end, beside, fi.cell_fields() if others else None


@functools.lru_cache(maxsize=None)
def _evaluated():
    """evaluate() on the field a run WITHOUT integrals left after every step: rows [STEPS, B, 12], and the last field's cells.  Once."""
    from gfv import integrals as FI
    fields, _, _ = TF._plain(WHICH)
    graphs = TF._graphs(WHICH)
    out = [FI.evaluate(graphs, _dev(f))["columns"].numpy() for f in fields]
    return np.stack(out), _cells(FI.evaluate(graphs, _dev(fields[-1]), fields=True))


def test_rollout_history_is_evaluate_of_every_field_and_the_run_is_unchanged():
    fields, plain_end, N = TF._plain(WHICH)
    want, want_cells = _evaluated()
    assert want.shape == (STEPS, 2, 12) and np.isfinite(want).all() and (want[:, :, [0, 1, 2, 3, 10, 11]] > 0).all()
    raws = {}
    for mode in ("cmd_list", "eager"):
        for others in (False, True):
            raw, h, end, beside, cells = _with_integrals(mode, others)
            rec, hist, hclock = raw
            what = (mode, others)
            assert rec.tolist() == [1, 1, -1, STEPS, STEPS, 0, 1, 0], (what, rec.tolist())
            assert hclock[:STEPS].tolist() == list(range(1, STEPS + 1))
            assert h["n"] == STEPS and h["clock"].tolist() == list(range(1, STEPS + 1)) and h["cells"].tolist() == [624, 36]
            assert _same(hist[:STEPS].numpy(), want), what                                         # bitwise evaluate() of every field
            for k, v in plain_end.items():                                                         # the run itself is the run without
                assert _same(end[k], v), (what, k)
            raws[what] = raw
            if others:                                                                             # the neighbours' state stays bitwise
                assert all(_same(a, b) for a, b in zip(beside[0], TF._with_stats(WHICH, mode)[0])), what
                assert all(_same(a, b) for a, b in zip(beside[1], TW._with_forces(mode)[0])), what
                assert all(_same(a, b) for a, b in zip(beside[2], TP._with_probes(mode, False)[0])), what
                assert cells[0] == STEPS and _same(torch.stack(cells[1:], 1).numpy(), want_cells), what
    first = raws[("cmd_list", False)]
    assert all(_same(a, b) for raw in raws.values() for a, b in zip(raw, first))
    # what read() hands out
    h = _with_integrals("eager", False)[1]
    assert _same(h["columns"].numpy(), want) and tuple(h["kinetic_energy"].shape) == (STEPS, 2)
    assert _same(h["div_l2"].numpy(), np.sqrt(want[:, :, 3] / want[:, :, 0])) and _same(h["outflow"].numpy(), np.ascontiguousarray(want[:, :, 8]))
    _, _, _, m = _case(WHICH)
    cavity = m["btype"][m["crow"][m["gcell_ptr"][1]]:]
    assert 2 not in cavity.tolist() and (want[:, 1, 8] == 0).all() and (want[:, 0, 7:9] != 0).all()       # the cavity: no outflow face
    # ... and a row is the restatement's, under its bound
    worst = 0.0
    for k in (0, STEPS - 1):
        rows, mag, _ = R.graph_rows(m, R.node_values(m, fields[k]))
        err, bound = np.abs(want[k] - rows), R.bound(m, mag)
        assert (err <= bound).all(), (k, err, bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"rollout rows against the restatement: largest error / bound {worst:.3g}")


# ---- 4. the window moves under a recorded list ------------------------------------------------------------------------------------
def test_set_window_holds_from_the_next_step_without_a_new_recording_and_reset_starts_over():
    from gfv.rollout import Rollout
    want, _ = _evaluated()
    fi = _integrals()
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, integrals=fi)
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
        got, hist, hclock = fi.raw()
        assert got.tolist() == rec.tolist(), (what, got.tolist(), rec.tolist())
        assert hclock[:len(clocks)].tolist() == clocks, what
        assert _same(hist[:len(clocks)].numpy(), want[[c - 1 for c in clocks]]), what

    steps(5)                                                                                       # the warm-up, the recording, a replay
    replayed = r._lists.stats()["replayed"]
    assert r._lists.stats()["recorded"] == 1 and replayed >= 1 and fi.count() == 5
    check("every step")
    fi.set_window(stride=3)                                                                        # clocks 1, 4, 7, 10: the next is 7
    rec[R.STRIDE] = 3
    steps(3)
    assert fi.count() == 6 and clocks[-1] == 7
    check("stride 3")
    fi.set_window(enabled=False)
    rec[R.ENABLED] = 0
    steps(1)
    fi.set_window(enabled=True, stop=10)
    rec[R.ENABLED], rec[R.STOP] = 1, 10
    steps(2)                                                                                       # 10: on the stride, but stop; 11: a miss
    assert fi.count() == 6
    check("paused, then stopped")
    assert r._lists.stats()["recorded"] == 1 and r._lists.stats()["replayed"] == replayed + 6      # nothing was recorded again
    r.reset()                                                                                      # the owner's: the integrals start over
    assert fi.count() == 0 and fi.raw()[0].tolist()[R.LAST] == -1 and fi.read()["clock"].shape == (0,)
    assert tuple(fi.read()["columns"].shape) == (0, 2, 12)
    rec[R.LAST], rec[R.N] = -1, 0
    clocks.clear()
    k = 0
    steps(5)
    assert fi.count() == 2 and clocks == [1, 4]
    check("after reset")
    assert r._lists.stats()["recorded"] == 1


# ---- 5. MarchStep ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march(ahead):
    from gfv.integrals import FlowIntegrals
    from gfv.march import MarchStep
    fi = FlowIntegrals(keep=8, fields=True)
    ms = MarchStep(TF._model(), TF._march_graphs(), lr=TF.LR, use_graph="list", tol=TF.TOL, max_inner=TF.MAX_INNER, max_levels=8,
                   keep=3, integrals=fi)
    assert ms.integrals is fi and ms._followers == [fi] and "integrals" not in ms.state_dict()
    rows = ms.run(levels=TF.LEVELS, max_ahead=ahead)
    state, held = TF._march_state(ms), ms.stats()["held"]
    snaps = [ms.snapshot(level).cpu().numpy() for level in range(TF.LEVELS)]
    raw, h, cells = fi.raw(), fi.read(), fi.cell_fields()
    for _ in range(2):
        ms.step()                                                                                  # held for certain
    assert ms.stats()["held"] == held + 2
    return rows, state, snaps, raw, h, fi.raw(), cells, fi.cell_fields()


def test_march_adds_one_row_per_completed_level_and_none_on_held_steps():
    from gfv import integrals as FI
    plain_rows, plain_state, plain_snaps, *_ = TF._march(None)
    assert [r["inner"] for r in plain_rows] == [4, 5, 5]
    raws = {}
    for ahead in (64, 0):
        rows, state, snaps, raw, h, raw_held, cells, cells_held = _march(ahead)
        assert [r["inner"] for r in rows] == [4, 5, 5]
        assert h["n"] == 3 and h["clock"].tolist() == [1, 2, 3]                                    # one per level: not 14
        assert raw[0].tolist() == [1, 1, -1, 3, 3, 0, 1, 0]
        assert all(_same(a, b) for a, b in zip(raw, raw_held))                                     # held steps add nothing
        assert cells[0] == cells_held[0] == 3 and all(_same(a, b) for a, b in zip(cells[1:], cells_held[1:]))
        graphs = TF._march_graphs()
        want = np.stack([FI.evaluate(graphs, _dev(s))["columns"].numpy() for s in snaps])
        assert _same(raw[1][0:3].numpy(), want) and (want[:, :, [0, 1, 2, 3]] > 0).all()
        last = FI.evaluate(graphs, _dev(snaps[-1]), fields=True)
        assert _same(cells[1], last["vorticity"]) and _same(cells[2], last["divergence"])
        assert state.keys() == plain_state.keys()
        for k in state:
            assert _same(state[k], plain_state[k]), (ahead, k)                                     # the march without integrals
        TF._same_rows(rows, plain_rows)
        assert all(_same(a, b) for a, b in zip(snaps, plain_snaps))
        raws[ahead] = raw
    assert all(_same(a, b) for a, b in zip(raws[64], raws[0]))


# ---- 6. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gfv import integrals as FI
    from gfv import lib as L
    from gfv.plan import get_plan
    from gfv.rollout import Rollout
    model = TF._model()
    r0 = Rollout(model, TF._graphs(WHICH), max_steps=4, launch_mode="eager")
    assert r0.integrals is None and r0._followers == []                                            # the default: nothing attached
    fi = _integrals(start=2, fields=True)
    with pytest.raises(ValueError, match=r"anderson > 0 together with integrals.*evaluate\(\)"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, anderson=2, integrals=fi)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        Rollout(model, tuple(g.clone() for g in TF._cpu_graphs(WHICH)), max_steps=4, integrals=fi)  # CPU graphs
    with pytest.raises(ValueError, match="FlowIntegrals"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, integrals=dict(keep=4))
    fi.check_free()                                                                                # a constructor that raised attached nothing
    graphs = TF._graphs(WHICH)
    plan = get_plan(graphs)
    with pytest.raises(ValueError, match="GPU"):
        fi.attach(object(), graphs, plan, torch.zeros(plan.N, 12), torch.zeros(1, dtype=torch.int32))          # a CPU node state
    fi.check_free()
    assert fi.rec is None and fi.tables is None
    r = Rollout(model, graphs, max_steps=4, launch_mode="eager", integrals=fi)
    with pytest.raises(ValueError, match="already attached"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, integrals=fi)                               # one owner per object
    assert not any(v is r for v in vars(fi).values())                                              # no reference back to the owner
    with pytest.raises(RuntimeError, match="no sample"):
        fi.cell_fields()
    r.step()
    assert fi.count() == 0 and fi.raw()[0].tolist()[R.LAST] == 1
    h = fi.read()
    assert h["n"] == 0 and tuple(h["columns"].shape) == (0, 2, 12) and tuple(h["div_l2"].shape) == (0, 2)
    r.step()
    assert fi.count() == 1 and fi.read()["clock"].tolist() == [2] and fi.cell_fields()[0] == 2
    with pytest.raises(RuntimeError, match="fields=True"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, launch_mode="eager", integrals=_integrals()).integrals.cell_fields()
    with pytest.raises(ValueError, match="rows"):
        FI.evaluate(graphs, torch.zeros(plan.N + 1, 3, device="cuda"))
    # the entry point: GFV_ERR_ARG, nothing launched
    t = fi.tables
    clock, rec = torch.ones(1, dtype=torch.int32, device="cuda"), _dev(_record())
    xb = torch.zeros((plan.N + 1, 12), dtype=torch.float32, device="cuda")
    ERR = -1

    def args(**over):
        a = dict(xb=xb, dim=plan.uvp_dim, crow=plan.crow, kface=plan.kface, knode=plan.knode, kS=plan.kS, btype=t.btype, es=plan.es,
                 er=plan.er, area=plan.area, beg=t.cchunk_beg, end=t.cchunk_end, gptr=t.gcchunk_ptr, nch=t.n_cchunks, C=t.C, B=t.B,
                 clock=clock, rec=rec, partial=fi.partial, hist=fi.hist, hclock=fi.hist_clock, keep=fi.keep, cell_out=fi.cell_out)
        a.update(over)
        return a

    def snapshot():
        return fi.raw() + (fi.partial.cpu().clone(), fi.cell_out.cpu().clone())

    before = snapshot()
    assert _launch(L, **args()) == 0                                                               # (the arguments as they stand: accepted)
    assert _launch(L, **args(cell_out=None)) == 0                                                  # (an unchanged clock: nothing sampled)
    torch.cuda.synchronize()
    assert int(rec[R.N]) == 1
    rec.copy_(_dev(_record()))
    fi.hist.copy_(before[1].cuda())
    fi.hist_clock.copy_(before[2].cuda())
    fi.partial.copy_(before[3].cuda())
    fi.cell_out.copy_(before[4].cuda())
    nullable = ("xb", "dim", "crow", "kface", "knode", "kS", "btype", "es", "er", "area", "beg", "end", "gptr", "clock", "rec", "partial",
                "hist", "hclock")
    for over in ([dict([(k, None)]) for k in nullable]
                 + [dict(C=0), dict(C=-1), dict(B=0), dict(B=-2), dict(nch=0), dict(nch=-1), dict(keep=0), dict(keep=-3),
                    dict(xb=xb.data_ptr() + 4), dict(xb=xb.data_ptr() + 8), dict(partial=fi.partial.data_ptr() + 4),
                    dict(hist=fi.hist.data_ptr() + 4), dict(cell_out=fi.cell_out.data_ptr() + 4), dict(kS=plan.kS.data_ptr() + 4)]):
        assert _launch(L, **args(**over)) == ERR, over
    torch.cuda.synchronize()
    assert rec.cpu().numpy().tolist() == _record().tolist()
    assert all(_same(a, b) for a, b in zip(snapshot(), before))
