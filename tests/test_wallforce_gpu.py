"""Wall forces on the device (gfv/wallforce.py, csrc/wallforce.hip; include/gfv.h gfv_wall_force_grad, gfv_wall_force_sum).

1. `gfv_wall_force_grad` alone on `cyl_b3` at all four orders, against tests/wallforce_ref.py under the bound of `_grad_bound`; at 2nd
   order against `gfv_wlsq_fwd_ex` to one fp32 rounding, and the bound rejects a restatement whose elimination runs in fp32; a launch
   that does not sample leaves a poisoned `gb` untouched;
2. `gfv_wall_force_sum` alone on synthetic tables (0, 1, 64, 65 faces per graph; 63 and 200), keep = 4, the clock script of
   tests/test_fieldstats_gpu.py extended past a ring wrap: record, `hist_clock` and the sample count as integers, the sums under the
   bound of `_sum_bound`, two launches on the same inputs the same bits, the inputs unchanged;
3. `Rollout` on `cyl_cavity_b2`, 12 steps, list mode and eager mode: the two histories bit for bit the same; fields, history and node
   state bit for bit those of a run without `wall_forces`; every row bitwise what `evaluate()` gives for the field captured after that
   step, and within the bounds of 1 and 2 of the restatement;
4. `set_window()` in the middle of a list-mode run holds from the next step with no new recording; `reset()` starts over;
5. `MarchStep` (the constants of tests/test_march_gpu.py): one row per completed level whatever its inner count, held steps add
   nothing, the march is bit for bit the march without forces;
6. the two known answers of tests/test_wallforce_cpu.py on the device through `evaluate()`, within the same bounds;
7. the refusals that need the device.
"""
import functools

import numpy as np
import pytest
import torch

import cases
import test_fieldstats_gpu as TF
import test_wallforce_cpu as TC
import wallforce_ref as R

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
U = 2.0 ** -53
BOX, ORIGIN = TC.BOX, (0.2, 0.2)
STEPS = TF.STEPS
_same = TF._same


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _record(start=1, stride=1, stop=-1, enabled=1):
    rec = np.zeros(R.RECORD, dtype=np.int32)
    rec[[R.START, R.STRIDE, R.STOP, R.ENABLED]] = (start, stride, stop, enabled)
    rec[R.LAST] = -1
    return rec


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def _grad_bound(m, bnode, field):
    """Per entry gb[j, c, 0:2]: 64 * kappa * 2^-53 * || sum_s |B_s| |dphi_s| / rn ||_2, kappa the largest cond_2(A / rn) of the body
    nodes, in float64.  Why this form: the rows of A / rn have unit norm, so || (A / rn)^-1 ||_2 <= kappa; the right-hand side is a
    sum of products each rounded once, off by at most (S + 1) 2^-53 times the vector in the norm; a backward-stable elimination of
    a 5 x 5 system moves the solution by a small multiple of kappa 2^-53 times its own size, which the same vector times kappa
    bounds; 64 covers both sides' (the kernel's and np.linalg.solve's) constants with room.  -> (bound [Nb, 3], kappa)"""
    q, cond = R.gradient_bounds(m, bnode, field)
    kappa = float(cond.max())
    return 64.0 * kappa * U * q, kappa


def _sum_bound(faces_b, mag):
    """Per graph and sum: (Nf_b + 16) * 2^-53 * sum |term|, |term| the term's expression with every operand replaced by its absolute
    value (tests/wallforce_ref.py face_terms).  Derivation: a term is an expression tree of depth <= 9 over exact inputs (Mp: a
    product, a sum, the node value added, the two sides added, theta3, S, the arm's own subtraction, the arm's product, the final
    difference), each operation rounded once, so it is off by at most 9 * 2^-53 (1 + o(1)) of its magnitude; any order of adding
    Nf_b terms - lane sums, the butterfly, the chunk fold - adds at most (Nf_b - 1) * 2^-53 (1 + o(1)) of the sum of magnitudes.
    9 + Nf_b - 1 < Nf_b + 16, the rest is room for the second-order terms; the restatement's own math.fsum is correctly rounded."""
    return (np.asarray(faces_b, dtype=f64)[:, None] + 16.0) * U * mag


# ---- 1. the gradient launch alone ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(which, order="2nd"):
    """-> (CPU graphs, device graphs, plan on the device, the restatement's arrays).  Once."""
    from gfv.plan import get_plan
    cpu = cases.make_graphs(which, order=order)
    dev = tuple(g.clone().to("cuda") for g in cpu)
    dev[0].norm_uvp, dev[0].norm_global = True, True
    plan = get_plan(dev)
    return cpu, dev, plan, R.mesh_arrays(cpu, plan)


def _launch_grad(L, plan, xb, bnode, clock, rec, gb, terms=None):
    return L.load().gfv_wall_force_grad(xb.data_ptr(), plan.uvp_dim.data_ptr(), plan.batch.data_ptr(), plan.x_rowptr.data_ptr(),
                                        plan.x_out.data_ptr(), plan.x_B.data_ptr(), plan.An.data_ptr(), plan.rn.data_ptr(),
                                        bnode.data_ptr(), int(bnode.shape[0]), int(plan.M) if terms is None else terms,
                                        clock.data_ptr(), rec.data_ptr(), gb.data_ptr(), L.stream_ptr())


@pytest.mark.parametrize("order, terms", [("1st", 2), ("2nd", 5), ("3rd", 9), ("4th", 14)])
def test_the_gradient_launch_alone_against_the_restatement(order, terms):
    from gfv import lib as L
    _, graphs, plan, m = _case("cyl_b3", order)
    assert plan.M == terms
    t = R.build_tables(m, R.select_faces(m))                                                       # every wall face: 204 faces
    assert t["faces"].tolist() == [65, 78, 61]
    bnode = _dev(t["bnode"])
    Nb = len(t["bnode"])
    rng = np.random.default_rng(40 + terms)
    field = (rng.standard_normal((m["N"], 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 12))).astype(f32)
    xb = _dev(field)
    POISON = -777.25
    gb = torch.full((Nb, 3, 2), POISON, dtype=torch.float64, device="cuda")
    clock = torch.tensor([1], dtype=torch.int32, device="cuda")
    # a launch that does not sample leaves the poison: clock before start, an unchanged clock, paused
    for rec_np in (_record(start=2), _record(), _record(enabled=0)):
        if rec_np[R.START] == 1 and rec_np[R.ENABLED] == 1:
            rec_np[R.LAST] = 1
        rec = _dev(rec_np)
        L.check(_launch_grad(L, plan, xb, bnode, clock, rec, gb), "gfv_wall_force_grad")
        torch.cuda.synchronize()
        assert bool((gb == POISON).all()) and rec.cpu().numpy().tolist() == rec_np.tolist()
    rec_np = _record()
    rec = _dev(rec_np)
    L.check(_launch_grad(L, plan, xb, bnode, clock, rec, gb), "gfv_wall_force_grad")
    torch.cuda.synchronize()
    assert rec.cpu().numpy().tolist() == rec_np.tolist()                                           # the first launch writes no word of it
    assert _same(xb, field)
    got = gb.cpu().numpy()
    want = R.gradients(m, t["bnode"], field)
    bound, kappa = _grad_bound(m, t["bnode"], field)
    err = np.abs(got - want)
    worst = float((err / bound[:, :, None]).max())
    print(f"{order}: kappa {kappa:.3g}, largest error / bound {worst:.3g}, largest |g| {np.abs(want).max():.3g}")
    assert np.isfinite(got).all() and worst <= 1.0, (order, worst)
    if order == "2nd":
        assert 5e2 < kappa < 2e3                                                                   # the bound carries weight here
        # the same arithmetic as the forward's reconstruction: (float)gb is its gradient to one fp32 rounding
        phi = np.zeros((m["N"], 8), dtype=f32)
        phi[:, 0:3] = R.node_values(m, field)
        grad = torch.zeros((m["N"], 16), dtype=torch.float32, device="cuda")
        L.check(L.load().gfv_wlsq_fwd_ex(_dev(phi).data_ptr(), plan.x_rowptr.data_ptr(), plan.x_out.data_ptr(),
                                         plan.x_B.data_ptr(), plan.An.data_ptr(), plan.rn.data_ptr(), grad.data_ptr(), None,
                                         m["N"], 5, L.stream_ptr()), "gfv_wlsq_fwd_ex")
        g32 = grad.cpu().numpy()[t["bnode"].astype(np.int64), 0:6].reshape(Nb, 3, 2)
        assert (np.abs(got.astype(f32) - g32) <= np.spacing(np.abs(g32))).all()
        # the bound REJECTS a restatement whose elimination runs in fp32
        low = R.gradients(m, t["bnode"], field, solve_dtype=f32)
        ratio = float((np.abs(low - want) / bound[:, :, None]).max())
        print(f"fp32 elimination: largest error / bound {ratio:.3g}")
        assert ratio > 1.0


# ---- 2. the sum launch alone, on synthetic tables ----------------------------------------------------------------------------------
def _synthetic(faces_per_graph, seed):
    """A batch made for the second launch only: per graph a handful of nodes and `faces` faces between random pairs of them, one
    incidence per face (stored in a shuffled order), random positions, vectors, coefficients.  -> the restatement's arrays."""
    rng = np.random.default_rng(seed)
    B = len(faces_per_graph)
    nodes = [max(3, n // 2 + 2) for n in faces_per_graph]
    noff = np.concatenate(([0], np.cumsum(nodes)))
    es, er, batch = [], [], np.repeat(np.arange(B), nodes)
    for b, n in enumerate(faces_per_graph):
        a = rng.integers(0, nodes[b], n)
        es.append(noff[b] + a)
        er.append(noff[b] + (a + 1 + rng.integers(0, nodes[b] - 1, n)) % nodes[b])
    es, er = np.concatenate(es).astype(np.int64), np.concatenate(er).astype(np.int64)
    E, N = len(es), int(noff[-1])
    kface = rng.permutation(E).astype(np.int64)                                                   # incidence k belongs to face kface[k]
    return {"B": B, "N": N, "E": E, "es": es, "er": er, "batch": batch, "kface": kface,
            "pos": rng.standard_normal((N, 2)).astype(f32), "fpos": rng.standard_normal((E, 2)).astype(f32),
            "kS": (rng.standard_normal((E, 2)) * 0.1).astype(f32), "theta": rng.uniform(0.2, 2.0, (B, 9)).astype(f32),
            "uvp_dim": rng.uniform(0.5, 2.0, (B, 3)).astype(f32)}


# (host words to write first, the clock, whether the launch samples); start = 2, stride = 2, no stop at first: the script of
# tests/test_fieldstats_gpu.py, then past the wrap of a ring of 4
SCRIPT = TF.SCRIPT + [
    (dict(STOP=-1), 12, True),
    (None, 14, True),                 # the fifth sample: slot 0 again
    (None, 14, False),
    (None, 16, True),
]


@pytest.mark.parametrize("faces_per_graph", [(0, 1, 64, 65), (63, 200)])
def test_the_sum_launch_alone_follows_the_reference_launch_by_launch(faces_per_graph):
    from gfv import lib as L
    lib = L.load()
    KEEP = 4
    m = _synthetic(faces_per_graph, 7 + len(faces_per_graph))
    B = m["B"]
    t = R.build_tables(m, np.arange(m["E"]))
    assert t["faces"].tolist() == list(faces_per_graph)
    assert (t["wchunk_end"] - t["wchunk_beg"]).tolist() == ([1, 64, 64, 1] if B == 4 else [63, 64, 64, 64, 8])
    rng = np.random.default_rng(99)
    origin = rng.standard_normal((B, 2)).astype(f32)
    ref = R.WallForcesRef(m, t, origin, KEEP, start=2, stride=2)
    Nb, nch = len(t["bnode"]), len(t["wchunk_beg"])
    const = {k: _dev(m[k].astype(np.int32) if m[k].dtype == np.int64 else m[k]) for k in ("es", "er", "pos", "fpos", "kS", "theta",
                                                                                         "uvp_dim")}
    tab = {k: _dev(t[k]) for k in ("wface", "wchunk_beg", "wchunk_end", "gwchunk_ptr")}
    org = _dev(origin)
    state = [{"rec": _dev(ref.rec), "partial": torch.full((nch, 6), 3.5, dtype=torch.float64, device="cuda"),
              "hist": torch.full((KEEP, B, 6), -9.0, dtype=torch.float64, device="cuda"),
              "hclock": torch.full((KEEP,), -5, dtype=torch.int32, device="cuda")} for _ in range(2)]
    ref.hist[:], ref.hist_clock[:] = -9.0, -5                                                     # (stale rows: read only up to n)
    clock = torch.zeros(1, dtype=torch.int32, device="cuda")
    taken = 0
    for i, (words, c, expect) in enumerate(SCRIPT):
        for name, v in (words or {}).items():
            idx = getattr(R, name)
            ref.rec[idx] = v
            for s in state:
                s["rec"][idx:idx + 1].copy_(torch.tensor([v], dtype=torch.int32))
        field = (rng.standard_normal((m["N"], 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 12))).astype(f32)
        gb_np = rng.standard_normal((Nb, 3, 2)) * 10.0 ** rng.uniform(-1.0, 1.0, (Nb, 3, 2))
        xb, gb = _dev(field), _dev(gb_np)
        clock.copy_(torch.tensor([c], dtype=torch.int32))
        before = (state[0]["hist"].cpu().clone(), state[0]["hclock"].cpu().clone(), state[0]["partial"].cpu().clone())
        for s in state:                                                                            # the same inputs, twice
            L.check(lib.gfv_wall_force_sum(
                xb.data_ptr(), const["uvp_dim"].data_ptr(), const["theta"].data_ptr(), 9, const["pos"].data_ptr(),
                const["fpos"].data_ptr(), const["kS"].data_ptr(), const["es"].data_ptr(), const["er"].data_ptr(),
                tab["wface"].data_ptr(), tab["wchunk_beg"].data_ptr(), tab["wchunk_end"].data_ptr(), tab["gwchunk_ptr"].data_ptr(),
                nch, m["E"], B, org.data_ptr(), gb.data_ptr(), clock.data_ptr(), s["rec"].data_ptr(), s["partial"].data_ptr(),
                s["hist"].data_ptr(), s["hclock"].data_ptr(), KEEP, L.stream_ptr()), "gfv_wall_force_sum")
        torch.cuda.synchronize()
        what = f"faces {faces_per_graph}, launch {i} (clock {c})"
        assert ref.launch(field, c, gb=gb_np) is expect, what
        a, b = state
        for k in a:
            assert _same(a[k], b[k]), (what, k)                                                    # the same bits, run after run
        assert a["rec"].cpu().numpy().tolist() == ref.rec.tolist(), (what, a["rec"].tolist(), ref.rec.tolist())
        assert a["hclock"].cpu().numpy().tolist() == ref.hist_clock.tolist(), what
        assert _same(xb, field) and _same(gb, gb_np) and int(clock[0]) == c and _same(tab["wface"], t["wface"]), what
        hist = a["hist"].cpu().numpy()
        if expect:
            row = taken % KEEP
            taken += 1
            bound = _sum_bound(t["faces"], ref.mag[row])
            err = np.abs(hist[row] - ref.hist[row])
            print(f"{what}: largest error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3g}")
            assert (err <= bound).all(), (what, err, bound)
            assert (hist[row][np.asarray(faces_per_graph) == 0] == 0).all()                       # a graph without a face: zeros
            other = [r for r in range(KEEP) if r != row]
            assert _same(hist[other], before[0].numpy()[other]), what
        else:
            assert _same(hist, before[0]) and _same(a["hclock"], before[1]) and _same(a["partial"], before[2]), what
    assert taken == 6 and int(state[0]["rec"][R.N]) == 6
    assert ref.rows()[0].tolist() == [8, 12, 14, 16]


# ---- 3. Rollout ----------------------------------------------------------------------------------------------------------------------
WHICH = "cyl_cavity_b2"


def _forces():
    from gfv.wallforce import WallForces
    return WallForces(box=BOX, origin=ORIGIN, keep=16)


@functools.lru_cache(maxsize=None)
def _with_forces(mode):
    from gfv.rollout import Rollout
    wf = _forces()
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, launch_mode=mode, wall_forces=wf)
    assert r.wall_forces is wf and r.field_stats is None
    fields = []
    for _ in range(STEPS):
        outs = r.step()
        if mode == "eager":
            fields.append(r.x_backup[:, 0:3].cpu().numpy().copy())                                 # (list mode: no synchronisation)
    end = TF._end_state(r, outs)
    if mode == "cmd_list":
        st = r._lists.stats()                              # (the warm-up steps are eager: both launch paths carry the pair)
        assert st["recorded"] == 1 and st["replayed"] >= 6 and st["eager"] >= 2, st
    return wf.raw(), wf.read(), end, fields


@functools.lru_cache(maxsize=None)
def _evaluated():
    """evaluate() on the field a run WITHOUT forces left after every step: [STEPS, B, 6].  Once."""
    from gfv import wallforce as WF
    fields, _, _ = TF._plain(WHICH)
    graphs = TF._graphs(WHICH)
    return np.stack([WF.evaluate(graphs, _dev(f), box=BOX, origin=ORIGIN).numpy() for f in fields])


def _restated(field):
    """-> (the restatement's sums [B, 6], the bound on a device row's distance from them): the bound of 2 for the sums given the
    gradients, plus what the bound of 1 on every gradient entry can move the sums by."""
    _, _, _, m = _case(WHICH)
    t = R.build_tables(m, R.select_faces(m, None, BOX))
    gb = R.gradients(m, t["bnode"], field)
    sums, mag = R.graph_sums(m, t["wface"], ORIGIN, field, gb)
    gbound, _ = _grad_bound(m, t["bnode"], field)
    move = R.gradient_sensitivity(m, t["wface"], ORIGIN, field, np.repeat(gbound[:, :, None], 2, axis=2))
    return sums, _sum_bound(t["faces"], mag) + move * (1.0 + 1e-6)


def test_rollout_history_is_evaluate_of_every_field_and_the_run_is_unchanged():
    fields, plain_end, N = TF._plain(WHICH)
    want = _evaluated()
    assert want.shape == (STEPS, 2, 6) and (want[:, 1] == 0).all() and np.abs(want[:, 0]).min() > 0    # the cavity holds no body
    raws = {}
    for mode in ("cmd_list", "eager"):
        raw, h, end, captured = _with_forces(mode)
        rec, hist, hclock = raw
        assert rec.tolist() == [1, 1, -1, STEPS, STEPS, 0, 1, 0], (mode, rec.tolist())
        assert hclock[:STEPS].tolist() == list(range(1, STEPS + 1))
        assert h["n"] == STEPS and h["clock"].tolist() == list(range(1, STEPS + 1)) and h["faces"].tolist() == [8, 0]
        rows = torch.cat((h["pressure"], h["viscous"], h["moment"]), 2).numpy()
        assert rows.dtype == f64 and _same(rows, want), mode                                       # bitwise evaluate() of every field
        for k, v in plain_end.items():                                                             # the run itself is the run without
            assert _same(end[k], v), (mode, k)
        if mode == "eager":
            assert all(_same(a, b) for a, b in zip(captured, fields))
        raws[mode] = raw
    assert all(_same(a, b) for a, b in zip(raws["cmd_list"], raws["eager"]))
    worst = 0.0
    for k in range(STEPS):
        sums, bound = _restated(fields[k])
        err = np.abs(want[k] - sums)
        assert (err <= bound).all(), (k, err, bound)
        worst = max(worst, float((err[0] / bound[0]).max()))
        assert (np.abs(sums[0, 0:2]) > 1e3 * bound[0, 0:2]).all()                                  # the bound decides something
    print(f"rollout rows against the restatement: largest error / bound {worst:.3g}")
    c = _with_forces("eager")[1]
    from gfv import wallforce as WF
    co = WF.coefficients(c, ref_length=0.1, ref_speed=1.0)
    assert tuple(co["cd"].shape) == (STEPS, 2) and _same(co["cd"].numpy(), (want[:, :, 0] + want[:, :, 2]) / 0.05)


# ---- 4. the window moves under a recorded list ------------------------------------------------------------------------------------
def test_set_window_holds_from_the_next_step_without_a_new_recording_and_reset_starts_over():
    from gfv.rollout import Rollout
    want = _evaluated()
    wf = _forces()
    r = Rollout(TF._model(), TF._graphs(WHICH), max_steps=STEPS, wall_forces=wf)
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
        got, hist, hclock = wf.raw()
        assert got.tolist() == rec.tolist(), (what, got.tolist(), rec.tolist())
        assert hclock[:len(clocks)].tolist() == clocks, what
        assert _same(hist[:len(clocks)].numpy(), want[[c - 1 for c in clocks]]), what

    steps(5)                                                                                       # the warm-up, the recording, a replay
    replayed = r._lists.stats()["replayed"]
    assert r._lists.stats()["recorded"] == 1 and replayed >= 1 and wf.count() == 5
    check("every step")
    wf.set_window(stride=3)                                                                        # clocks 1, 4, 7, 10: the next is 7
    rec[R.STRIDE] = 3
    steps(3)
    assert wf.count() == 6 and clocks[-1] == 7
    check("stride 3")
    wf.set_window(enabled=False)
    rec[R.ENABLED] = 0
    steps(1)
    wf.set_window(enabled=True, stop=10)
    rec[R.ENABLED], rec[R.STOP] = 1, 10
    steps(2)                                                                                       # 10: on the stride, but stop; 11: a miss
    assert wf.count() == 6
    check("paused, then stopped")
    assert r._lists.stats()["recorded"] == 1 and r._lists.stats()["replayed"] == replayed + 6      # nothing was recorded again
    r.reset()                                                                                      # the owner's: the forces start over
    assert wf.count() == 0 and wf.raw()[0].tolist()[R.LAST] == -1 and wf.read()["clock"].shape == (0,)
    rec[R.LAST], rec[R.N] = -1, 0
    clocks.clear()
    k = 0
    steps(5)
    assert wf.count() == 2 and clocks == [1, 4]
    check("after reset")
    assert r._lists.stats()["recorded"] == 1


# ---- 5. MarchStep ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march(ahead):
    from gfv.march import MarchStep
    from gfv.wallforce import WallForces
    wf = WallForces(origin=(0.1, 0.15), keep=8)                                                    # every wall face of the mesh
    ms = MarchStep(TF._model(), TF._march_graphs(), lr=TF.LR, use_graph="list", tol=TF.TOL, max_inner=TF.MAX_INNER, max_levels=8,
                   keep=3, wall_forces=wf)
    assert ms.wall_forces is wf and "wall_forces" not in ms.state_dict()
    rows = ms.run(levels=TF.LEVELS, max_ahead=ahead)
    state, held = TF._march_state(ms), ms.stats()["held"]
    snaps = [ms.snapshot(level).cpu().numpy() for level in range(TF.LEVELS)]
    raw, h = wf.raw(), wf.read()
    for _ in range(2):
        ms.step()                                                                                  # held for certain
    assert ms.stats()["held"] == held + 2
    return rows, state, snaps, raw, h, wf.raw()


def test_march_adds_one_row_per_completed_level_and_none_on_held_steps():
    from gfv import wallforce as WF
    plain_rows, plain_state, plain_snaps, *_ = TF._march(None)
    assert [r["inner"] for r in plain_rows] == [4, 5, 5]
    raws = {}
    for ahead in (64, 0):
        rows, state, snaps, raw, h, raw_held = _march(ahead)
        assert [r["inner"] for r in rows] == [4, 5, 5]
        assert h["n"] == 3 and h["clock"].tolist() == [1, 2, 3] and h["faces"].tolist() == [49]    # one per level: not 14
        assert raw[0].tolist() == [1, 1, -1, 3, 3, 0, 1, 0]
        assert all(_same(a, b) for a, b in zip(raw, raw_held))                                     # held steps add nothing
        graphs = TF._march_graphs()
        want = np.stack([WF.evaluate(graphs, _dev(s), origin=(0.1, 0.15)).numpy() for s in snaps])
        assert _same(raw[1][0:3].numpy(), want) and np.abs(want[:, 0, 0:4]).min() > 0
        assert state.keys() == plain_state.keys()
        for k in state:
            assert _same(state[k], plain_state[k]), (ahead, k)                                     # the march without forces
        TF._same_rows(rows, plain_rows)
        assert all(_same(a, b) for a, b in zip(snaps, plain_snaps))
        raws[ahead] = raw
    assert all(_same(a, b) for a, b in zip(raws[64], raws[0]))


# ---- 6. the known answers, on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cyl_b3", "cyl_cavity_b2"])
def test_known_answers_through_evaluate(which):
    from gfv import wallforce as WF
    _, graphs, _, _ = _case(which)
    for box in (TC.BOX, TC.HALF):
        k = TC.linear_case(which, box)
        m, t = k["m"], k["t"]
        got = WF.evaluate(graphs, _dev(k["field"]), box=box).numpy()
        assert got.shape == (m["B"], 6) and got.dtype == f64
        # the device against the restatement: the bounds of 1 and 2; the restatement against the answer: the CPU test's tolerance
        gb = R.gradients(m, t["bnode"], k["field"])
        _, mag = R.graph_sums(m, t["wface"], (0.0, 0.0), k["field"], gb)
        gbound, _ = _grad_bound(m, t["bnode"], k["field"])
        dev_tol = (_sum_bound(t["faces"], mag)
                   + R.gradient_sensitivity(m, t["wface"], (0.0, 0.0), k["field"], np.repeat(gbound[:, :, None], 2, axis=2)))
        for g in range(m["B"]):
            if not t["faces"][g]:
                assert (got[g] == 0).all()
                continue
            err, tol = np.abs(got[g, 0:4] - k["exact"][g]), k["tol"][g] + dev_tol[g, 0:4]
            print(f"{which} box={box} graph {g}: err {err}, tol {tol}")
            assert (err[2:4] <= tol[2:4]).all(), (which, g, "viscous")
            if k["closed"][g]:
                assert (err[0:2] <= tol[0:2]).all() and abs(k["exact"][g, 0]) > 100 * tol[0], (which, g, "pressure")


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gfv import lib as L
    from gfv import wallforce as WF
    from gfv.fieldstats import FieldStats
    from gfv.rollout import Rollout
    from gfv.wallforce import WallForces
    model = TF._model()
    r0 = Rollout(model, TF._graphs(WHICH), max_steps=4, launch_mode="eager")
    assert r0.wall_forces is None                                                                  # the default: nothing attached
    wf = WallForces(box=BOX, start=2)
    with pytest.raises(ValueError, match="anderson"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, anderson=2, wall_forces=wf)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        Rollout(model, tuple(g.clone() for g in TF._cpu_graphs(WHICH)), max_steps=4, wall_forces=wf)           # CPU graphs
    with pytest.raises(ValueError, match="WallForces"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, wall_forces=dict(box=BOX))
    with pytest.raises(ValueError, match="no face"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, wall_forces=WallForces(box=(10, 11, 10, 11)))
    wf.check_free()                                                                                # a constructor that raised attached nothing
    fs = FieldStats()
    r = Rollout(model, TF._graphs(WHICH), max_steps=4, launch_mode="eager", wall_forces=wf, field_stats=fs)    # beside field_stats
    with pytest.raises(ValueError, match="already attached"):
        Rollout(model, TF._graphs(WHICH), max_steps=4, wall_forces=wf)                             # one owner per object
    assert not any(v is r for v in vars(wf).values())                                              # no reference back to the owner
    r.step()
    assert wf.count() == 0 and wf.raw()[0].tolist()[R.LAST] == 1 and fs.count() == 1
    h = wf.read()
    assert h["n"] == 0 and tuple(h["pressure"].shape) == (0, 2, 2)
    r.step()
    assert wf.count() == 1 and wf.read()["clock"].tolist() == [2]
    # the entry points: GFV_ERR_ARG, nothing launched
    _, _, plan, m = _case(WHICH)
    t = wf.tables
    clock, rec = torch.ones(1, dtype=torch.int32, device="cuda"), _dev(_record())
    xb = torch.zeros((plan.N + 1, 12), dtype=torch.float32, device="cuda")
    gb = torch.full((t.Nb * 6 + 1,), 5.0, dtype=torch.float64, device="cuda")
    ERR = -1
    assert _launch_grad(L, plan, xb, t.bnode, clock, rec, gb, terms=3) == ERR
    assert _launch_grad(L, plan, xb, t.bnode[:0], clock, rec, gb) == ERR                           # Nb = 0
    assert _launch_grad(L, plan, xb.reshape(-1)[1:], t.bnode, clock, rec, gb) == ERR               # x_backup not 16-byte aligned
    assert _launch_grad(L, plan, xb, t.bnode, clock, rec, gb.view(torch.float32)[1:]) == ERR       # gb not 8-byte aligned
    lib = L.load()
    assert lib.gfv_wall_force_grad(None, *([xb.data_ptr()] * 8), t.Nb, 5, clock.data_ptr(), rec.data_ptr(), gb.data_ptr(),
                                   L.stream_ptr()) == ERR

    def sum_args(**over):
        a = dict(x_backup=xb.data_ptr(), uvp_dim=plan.uvp_dim.data_ptr(), theta=plan.theta.data_ptr(), ld_theta=9,
                 pos=plan.pos.data_ptr(), fpos=plan.fpos.data_ptr(), kS=plan.kS.data_ptr(), es=plan.es.data_ptr(),
                 er=plan.er.data_ptr(), wface=t.wface.data_ptr(), wchunk_beg=t.wchunk_beg.data_ptr(),
                 wchunk_end=t.wchunk_end.data_ptr(), gwchunk_ptr=t.gwchunk_ptr.data_ptr(), n_wchunks=t.n_wchunks, Nf=t.Nf, B=t.B,
                 origin=wf.origin.data_ptr(), gb=gb.data_ptr(), clock=clock.data_ptr(), rec=rec.data_ptr(),
                 partial=wf.partial.data_ptr(), hist=wf.hist.data_ptr(), hist_clock=wf.hist_clock.data_ptr(), keep=wf.keep)
        a.update(over)
        return list(a.values()) + [L.stream_ptr()]

    hist_before = wf.raw()
    for over in (dict(x_backup=None), dict(hist_clock=None), dict(Nf=0), dict(B=0), dict(keep=0), dict(n_wchunks=0),
                 dict(x_backup=xb.data_ptr() + 4), dict(gb=gb.data_ptr() + 4), dict(partial=wf.partial.data_ptr() + 4),
                 dict(hist=wf.hist.data_ptr() + 4)):
        assert lib.gfv_wall_force_sum(*sum_args(**over)) == ERR, over
    torch.cuda.synchronize()
    assert rec.cpu().numpy().tolist() == _record().tolist() and bool((gb == 5.0).all())
    assert all(_same(a, b) for a, b in zip(wf.raw(), hist_before))
