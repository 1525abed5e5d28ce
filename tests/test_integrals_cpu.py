"""Flow integrals, the part that needs no GPU (gfv/integrals.py; tests/integrals_ref.py is the float64 restatement).

1. the tables on `cyl_cavity_b2`, `cavity_mixed_b1` and `cyl_b3` against a brute-force restatement: the boundary kind of every
   incidence (136, 32 and 242 one-incidence faces; interior faces of `cyl_b3` that carry a boundary type stay 0), the cell chunks
   (full chunks, a 48-cell tail, a graph smaller than one chunk), and every cell's face ends are exactly its vertices;
2. known answers through the restatement: a linear field (divergence 1.6, vorticity 0.9 on every cell), a rigid rotation
   (vorticity 2 Omega, no divergence, enstrophy 2 Omega^2 area), a uniform stream (kinetic energy U^2 area / 2, no net outflow); the
   tolerances are derived in `linear_case` from the precision of the data alone;
3. the identity net outflow = inflow + outflow + other flux per graph, and the exact antisymmetry of kS it rests on;
4. the record and the ring over the clock script of the window tests, past a wrap of a ring of 4;
5. every refusal that needs no GPU, in `check_handed`'s order, and `check_followers` with six followers.
"""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import cases
import integrals_ref as R
import window_ref

f32, f64 = np.float32, np.float64
U, U32 = R.U, R.U32
CASES3 = ("cyl_cavity_b2", "cavity_mixed_b1", "cyl_b3")
CELLS = {"cyl_cavity_b2": [624, 36], "cavity_mixed_b1": [80], "cyl_b3": [357, 362, 389]}
ONE_INCIDENCE = {"cyl_cavity_b2": (136, {1, 2, 3}), "cavity_mixed_b1": (32, {1, 3}), "cyl_b3": (242, {1, 2, 3})}


@functools.lru_cache(maxsize=None)
def setup(which):
    """-> (graphs, plan, the restatement's arrays) of a case, on the CPU.  Once."""
    from gfv.plan import build_plan
    graphs = cases.make_graphs(which)
    plan = build_plan(*graphs)
    return graphs, plan, R.mesh_arrays(graphs, plan)


@functools.lru_cache(maxsize=None)
def module_arrays(which):
    """The restatement's arrays with the boundary kinds and the graphs' cell ranges as gfv.integrals builds them (the tables the
    launch is handed): what the known answers and the identity run on.  Once."""
    from gfv import integrals as FI
    graphs, plan, m = setup(which)
    t = FI.build_tables(plan, graphs[2].face_type)
    ptr, end = t.gcchunk_ptr.numpy(), t.cchunk_end.numpy()
    gcell_ptr = np.concatenate(([0], [int(end[ptr[b + 1] - 1]) if ptr[b + 1] > ptr[b] else 0 for b in range(t.B)]))
    gcell_ptr = np.maximum.accumulate(gcell_ptr).astype(np.int64)              # (a graph without a chunk ends where the last ended)
    assert (np.diff(gcell_ptr) == t.cells.numpy()).all() and int(t.cchunk_beg[0]) == 0
    return dict(m, btype=t.btype.numpy().copy(), gcell_ptr=gcell_ptr)


def named(rows):
    """A [B, 12] block through the module's `split_columns`: the names read() and evaluate() hand out, as numpy."""
    from gfv import integrals as FI
    return {k: v.numpy() for k, v in FI.split_columns(torch.from_numpy(np.ascontiguousarray(rows))).items()}


# ---- 1. the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES3)
def test_tables_are_the_brute_force_restatement(which):
    from gfv import integrals as FI
    from gfv import lib as L
    graphs, plan, m = setup(which)
    assert np.diff(m["gcell_ptr"]).tolist() == CELLS[which]
    # the boundary kinds
    t = FI.build_tables(plan, graphs[2].face_type)
    assert t.btype.dtype == torch.int32 and t.btype.is_contiguous() and tuple(t.btype.shape) == (len(m["kface"]),)
    assert t.btype.numpy().tolist() == m["btype"].tolist()
    inc = np.bincount(m["kface"], minlength=m["E"])
    assert set(inc.tolist()) == {1, 2}
    one = m["btype"] > 0
    assert (inc[m["kface"]][one] == 1).all() and (inc[m["kface"]][~one] == 2).all()
    count, kinds = ONE_INCIDENCE[which]
    assert int(one.sum()) == int((inc == 1).sum()) == count and set(m["btype"][one].tolist()) == kinds
    ft = m["face_type"][m["kface"]]
    assert ((m["btype"] == 1) == (one & (ft == 1))).all() and ((m["btype"] == 2) == (one & (ft == 2))).all()
    typed_inside = (inc == 2) & np.isin(m["face_type"], (1, 2))                 # an interior edge between two boundary nodes
    if which == "cyl_b3":
        assert int(typed_inside.sum()) >= 1 and 2 in m["face_type"][inc == 2].tolist()
    assert (m["btype"][np.isin(m["kface"], np.nonzero(typed_inside)[0])] == 0).all()
    assert t.cells.tolist() == CELLS[which] and (t.n_cchunks, t.C, t.B) == (len(t.cchunk_beg), m["C"], m["B"])
    # the cell chunks
    beg, end, ptr = R.chunks(m["gcell_ptr"])
    assert L.FLOW_CHUNK == R.CHUNK == 64
    for got, want in ((t.cchunk_beg, beg), (t.cchunk_end, end), (t.gcchunk_ptr, ptr)):
        assert got.dtype == torch.int32 and got.numpy().tolist() == want.tolist()
    sizes = (end - beg).tolist()
    assert sizes == {"cyl_cavity_b2": [64] * 9 + [48, 36], "cavity_mixed_b1": [64, 16],
                     "cyl_b3": [64] * 5 + [37] + [64] * 5 + [42] + [64] * 6 + [5]}[which]
    assert ptr.tolist() == {"cyl_cavity_b2": [0, 10, 11], "cavity_mixed_b1": [0, 2], "cyl_b3": [0, 6, 12, 19]}[which]
    covered = np.concatenate([np.arange(a, b) for a, b in zip(beg, end)])
    assert covered.tolist() == list(range(m["C"]))
    # every cell's face ends are exactly its vertices, each the end of two of its faces
    for C in range(m["C"]):
        k = slice(m["crow"][C], m["crow"][C + 1])
        ends = np.concatenate((m["es"][m["kface"][k]], m["er"][m["kface"][k]]))
        V = m["knode"][k]
        assert len(set(V.tolist())) == len(V) >= 3 and sorted(ends.tolist()) == sorted(V.tolist() * 2), C


# ---- 2. known answers --------------------------------------------------------------------------------------------------------------
# u = A[0, 0] + A[0, 1] x + A[0, 2] y, v = A[1, 0] + A[1, 1] x + A[1, 2] y, p = A[2, ...]; the node state holds fl32(dim_c * phi_c):
# what the launch divides again.
LINEAR = np.array([[0.3, 0.7, -0.4], [-0.2, 0.5, 0.9], [0.1, -0.3, 0.2]])
OMEGA, CENTRE = 1.7, (0.4, 0.25)
ROTATION = np.array([[OMEGA * CENTRE[1], 0.0, -OMEGA], [-OMEGA * CENTRE[0], OMEGA, 0.0], [0.5, 0.0, 0.0]])
SPEED = 1.3
STREAM = np.array([[SPEED * 0.8, 0.0, 0.0], [SPEED * 0.6, 0.0, 0.0], [0.25, 0.0, 0.0]])       # |(u, v)| = SPEED (0.8, 0.6)
FIELDS = {"linear": LINEAR, "rotation": ROTATION, "stream": STREAM}


@functools.lru_cache(maxsize=None)
def linear_case(which, name):
    """-> dict: the mesh arrays, graphs, the field [N, 12] fp32 and per cell the exact integrals D [C] and Gamma [C] (area times the
    field's divergence and vorticity) with their tolerances, from the precision of the data alone (u = 2^-24).

    The answers.  With the positions the plan holds taken as exact (the field is DEFINED on them), the trapezoid face value of a
    linear field is its value at the midpoint m_k of the face's ends, and with c = sum_k kS[k] and T = sum_k m_k (x) kS[k] (2 x 2)
        D     = sum_k u(m_k) . S_k           = a0 c_x + b0 c_y + a1 T_xx + a2 T_yx + b1 T_xy + b2 T_yy
        Gamma = sum_k v(m_k) S_kx - u(m_k) S_ky = b0 c_x - a0 c_y + b1 T_xx + b2 T_yx - a1 T_xy - a2 T_yy
    exactly.  A closed polygon with exact outward vectors has c = 0 and T = area * I (the divergence theorem for x and y), which gives
    D = (a1 + b2) area and Gamma = (b1 - a2) area.

    The tolerances.  The data are fp32: kS, the positions and area[C] are roundings, made independently of one another.  What they
    miss the two identities by is measured ON THE DATA, in float64: the closure defect c, and the moment defect M = T - area[C] * I
    (half its trace is the gap between area[C] and 0.5 sum_k m_k . kS[k]; the rest is the same gap for x and y apart and across).
    Neither involves the field or the code under test.  So
        |D - (a1 + b2) area[C]|     <= |a0| |c_x| + |b0| |c_y| + |a1| |M_xx| + |a2| |M_yx| + |b1| |M_xy| + |b2| |M_yy| + e_D
        |Gamma - (b1 - a2) area[C]| <= |b0| |c_x| + |a0| |c_y| + |b1| |M_xx| + |b2| |M_yx| + |a1| |M_xy| + |a2| |M_yy| + e_G
    where e is the node values' rounding: the launch sees fl32(fl32(dim * phi) / dim) = phi (1 + d), |d| <= 2.01 u, so a face value
    is off by at most 2.01 u * 0.5 (|phi_s| + |phi_r|) and e_D = sum_k 2.01 u (|u_f| |S_kx| + |v_f| |S_ky|), e_G likewise with the
    vector's components swapped.  The mean over a cell's vertices is off by at most 2.01 u times the mean of |phi|.
    """
    graphs, plan, _ = setup(which)
    m = module_arrays(which)
    A = FIELDS[name]
    pos = m["pos"].astype(f64)
    phi = A[:, 0][None, :] + pos[:, 0:1] * A[:, 1][None, :] + pos[:, 1:2] * A[:, 2][None, :]           # [N, 3]
    field = np.zeros((m["N"], 12), dtype=f32)
    field[:, 0:3] = (m["uvp_dim"][m["batch"]].astype(f64) * phi).astype(f32)
    crow, kface = m["crow"], m["kface"]
    first = crow[:-1]
    s, r = m["es"][kface], m["er"][kface]
    S = m["kS"].astype(f64)
    mid = 0.5 * (pos[s] + pos[r])
    seg = lambda x: np.add.reduceat(x, first)
    a = m["area"].astype(f64)
    c = np.stack((seg(S[:, 0]), seg(S[:, 1])), 1)                                                   # [C, 2]
    T = np.stack([seg(mid[:, i] * S[:, j]) for i in (0, 1) for j in (0, 1)], 1).reshape(-1, 2, 2)   # T[C, i, j] = sum m_i S_j
    M = np.abs(T - a[:, None, None] * np.eye(2))
    absphi = np.abs(phi)
    uf, vf = 0.5 * (absphi[s, 0] + absphi[r, 0]), 0.5 * (absphi[s, 1] + absphi[r, 1])
    aS = np.abs(S)
    e_D = 2.01 * U32 * seg(uf * aS[:, 0] + vf * aS[:, 1])
    e_G = 2.01 * U32 * seg(vf * aS[:, 0] + uf * aS[:, 1])
    (a0, a1, a2), (b0, b1, b2) = np.abs(A[0]), np.abs(A[1])
    ac = np.abs(c)
    tol_D = a0 * ac[:, 0] + b0 * ac[:, 1] + a1 * M[:, 0, 0] + a2 * M[:, 1, 0] + b1 * M[:, 0, 1] + b2 * M[:, 1, 1] + e_D
    tol_G = b0 * ac[:, 0] + a0 * ac[:, 1] + b1 * M[:, 0, 0] + b2 * M[:, 1, 0] + a1 * M[:, 0, 1] + a2 * M[:, 1, 1] + e_G
    n = np.diff(crow).astype(f64)
    return {"m": m, "graphs": graphs, "plan": plan, "field": field, "A": A, "area": a, "div": A[0, 1] + A[1, 2],
            "vort": A[1, 1] - A[0, 2], "tol_D": tol_D, "tol_G": tol_G, "closure": float(np.abs(c).max() / np.sqrt(a).min()),
            "mean_abs": np.stack([seg(absphi[m["knode"], ch]) / n for ch in range(3)], 1)}


def check_known(k, rows, cell_out, room_rows=0.0, room_cells=0.0, what=""):
    """rows [B, 12] and cell_out [C, 2] = (vorticity, divergence) of a linear_case against its exact answers within its tolerances
    (+ `room`, the caller's own double rounding).  Prints the figures, then asserts.  -> the largest error / tolerance."""
    m, a = k["m"], k["area"]
    signal = np.abs(np.array([k["vort"], k["div"]]))                 # per component: vorticity, divergence
    tol = np.stack((k["tol_G"] / a, k["tol_D"] / a), 1) + room_cells
    err = np.abs(cell_out - np.array([k["vort"], k["div"]]))
    rel = lambda v: " / ".join(f"{v[:, j].max() / signal[j]:.3g}" if signal[j] else "-" for j in (0, 1))
    print(f"{what}: per cell, largest error / tolerance: vorticity {(err[:, 0] / tol[:, 0]).max():.3g}, divergence "
          f"{(err[:, 1] / tol[:, 1]).max():.3g}; largest tolerance / signal (vorticity / divergence) {rel(tol)}; "
          f"largest error / signal {rel(err)}")
    assert (err <= tol).all(), (what, err.max(0), tol.max(0))
    # the condition, per component against its OWN signal: a wrong sign stands hundreds of tolerances tall.  A component whose exact
    # answer is zero (a rotation's divergence, both of a stream's) has no signal to compare with: its tolerance is still asserted
    # above, and the other fields pin that component.
    for j in (0, 1):
        if signal[j]:
            assert tol[:, j].max() < 1e-3 * signal[j], (what, j)
    worst = float((err / tol).max())
    gp = m["gcell_ptr"]
    room = np.zeros((m["B"], R.COLS)) + room_rows
    for b in range(m["B"]):
        cs = slice(gp[b], gp[b + 1])
        area = float(a[cs].sum())
        tD, tG = float(k["tol_D"][cs].sum()), float(k["tol_G"][cs].sum())
        want = {0: (area, 0.0), 4: (k["div"] * area, tD), 5: (k["vort"] * area, tG),
                2: (0.5 * k["vort"] ** 2 * area, float((abs(k["vort"]) * k["tol_G"][cs] + 0.5 * k["tol_G"][cs] ** 2 / a[cs]).sum())),
                3: (k["div"] ** 2 * area, float((2.0 * abs(k["div"]) * k["tol_D"][cs] + k["tol_D"][cs] ** 2 / a[cs]).sum())),
                10: (abs(k["div"]), float((k["tol_D"][cs] / a[cs]).max())), 11: (abs(k["vort"]), float((k["tol_G"][cs] / a[cs]).max()))}
        if not k["A"][:, 1:3].any():                                 # a uniform field: the vertex means are the field itself
            speed2, pbar = float(k["A"][0, 0] ** 2 + k["A"][1, 0] ** 2), float(k["A"][2, 0])
            want[1] = (0.5 * speed2 * area, 0.5 * speed2 * area * (2.0 * 2.01 * U32 + (2.01 * U32) ** 2))
            want[6] = (pbar * area, abs(pbar) * area * 2.01 * U32)
        for col, (value, t) in want.items():
            t = t + room[b, col] + 4.0 * U * abs(value)              # (the answer's own float64 arithmetic)
            e = abs(float(rows[b, col]) - value)
            assert e <= t, (what, b, col, float(rows[b, col]), value, e, t)
            worst = max(worst, e / t)
    return worst


@pytest.mark.parametrize("which", CASES3)
@pytest.mark.parametrize("name", list(FIELDS))
def test_known_answers(which, name):
    k = linear_case(which, name)
    m = k["m"]
    rows, mag, cell_out = R.graph_rows(m, R.node_values(m, k["field"]))
    cmag = R.cell_terms(m, R.node_values(m, k["field"]))[1]
    worst = check_known(k, rows, cell_out, R.bound(m, mag), R.cell_bound(m, cmag), f"{which} {name} restatement")
    print(f"{which} {name}: largest error / tolerance {worst:.3g}; closure defect / cell size {k['closure']:.3g}")
    if name == "linear":
        assert k["div"] == pytest.approx(1.6) and k["vort"] == pytest.approx(0.9)
        # the tolerance decides something: a lost 0.5 in the face value, or a vorticity of the wrong sign, is refused
        with pytest.raises(AssertionError):
            check_known(k, rows, cell_out * np.array([1.0, 2.0]))
        with pytest.raises(AssertionError):
            check_known(k, rows, cell_out * np.array([-1.0, 1.0]))
        tol = np.stack((k["tol_G"], k["tol_D"]), 1) / k["area"][:, None]
        assert (np.array([k["vort"], k["div"]]) > 500.0 * tol).all()
    h = named(rows)                                                  # ... and under the names the module hands out
    if name == "linear":
        assert np.allclose(h["div_l2"], 1.6, rtol=1e-4, atol=0) and np.allclose(h["div_max"], 1.6, rtol=1e-4, atol=0)
        assert np.allclose(h["vort_max"], 0.9, rtol=1e-4, atol=0) and np.allclose(h["net_outflow"], 1.6 * h["area"], rtol=1e-4, atol=0)
        assert np.allclose(h["circulation"], 0.9 * h["area"], rtol=1e-4, atol=0)
        assert np.allclose(h["inflow"] + h["outflow"] + h["other_flux"], h["net_outflow"], rtol=1e-9, atol=0)
    if name == "rotation":
        assert k["div"] == 0.0 and k["vort"] == 2.0 * OMEGA
        assert np.allclose(h["enstrophy"], 2.0 * OMEGA ** 2 * h["area"], rtol=1e-3, atol=0)      # enstrophy 2 Omega^2 area, spelt out
        assert (h["div_l2"] < 1e-4 * 2.0 * OMEGA).all() and np.allclose(h["vort_max"], 2.0 * OMEGA, rtol=1e-4, atol=0)
    if name == "stream":
        assert k["div"] == 0.0 and k["vort"] == 0.0 and (np.abs(h["net_outflow"]) < 1e-5 * SPEED * np.sqrt(h["area"])).all()
        assert np.allclose(h["kinetic_energy"], 0.5 * SPEED ** 2 * h["area"], rtol=1e-6, atol=0)
        assert np.allclose(h["mean_pressure"], 0.25, rtol=1e-6, atol=0)


# ---- 3. the identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES3)
def test_net_outflow_is_the_sum_of_the_boundary_fluxes(which):
    m = module_arrays(which)                                         # the boundary kinds as gfv.integrals builds them
    # kS is exactly antisymmetric across every interior face
    worst = 0.0
    for f in np.nonzero(np.bincount(m["kface"], minlength=m["E"]) == 2)[0]:
        k = np.nonzero(m["kface"] == f)[0]
        worst = max(worst, float(np.abs(m["kS"][k[0]].astype(f64) + m["kS"][k[1]].astype(f64)).max()))
    assert worst == 0.0
    rng = np.random.default_rng(11)
    field = (rng.standard_normal((m["N"], 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 12))).astype(f32)
    rows, mag, _ = R.graph_rows(m, R.node_values(m, field))
    # with it the interior faces' d_k cancel in pairs exactly (u_f is the same double on both sides), so column 4 and columns
    # 7 + 8 + 9 differ by the rounding of their sums alone: each under the bound, plus the two additions
    b = R.bound(m, mag)
    gap = np.abs(rows[:, 4] - (rows[:, 7] + rows[:, 8] + rows[:, 9]))
    room = b[:, 4] + b[:, 7] + b[:, 8] + b[:, 9] + 2.0 * U * (np.abs(rows[:, 7]) + np.abs(rows[:, 8]) + np.abs(rows[:, 9]))
    print(f"{which}: largest |col 4 - (7 + 8 + 9)| / bound {float((gap / room).max()):.3g}")
    assert (gap <= room).all() and (np.abs(rows[:, 7:10]).sum(1) > 1e6 * room).all()
    h = named(rows)
    assert np.array_equal(np.abs(h["net_outflow"] - (h["inflow"] + h["outflow"] + h["other_flux"])), gap)
    if 2 not in set(m["btype"].tolist()):
        assert (h["outflow"] == 0).all()                              # the cavity has no outflow face


# ---- 4. the record and the ring ----------------------------------------------------------------------------------------------------
def test_record_and_ring_over_the_clock_script_past_a_wrap():
    from gfv import integrals as FI
    from test_wallforce_gpu import SCRIPT                                      # the window tests' script, then past a ring of 4
    _, _, m = setup("cavity_mixed_b1")
    KEEP = 4
    ref = R.FlowRef(m, KEEP, start=2, stride=2)
    rec = ref.rec.copy()                                                       # window_ref alone, beside it
    rng = np.random.default_rng(3)
    taken = []
    for words, c, expect in SCRIPT:
        for name, v in (words or {}).items():
            ref.rec[getattr(R, name)] = rec[getattr(window_ref, name)] = v
        field = rng.standard_normal((m["N"], 12)).astype(f32)
        before = (ref.hist.copy(), ref.hist_clock.copy(), ref.cell_out.copy())
        want = window_ref.take(rec, c)
        assert ref.launch(field, c) is want is expect, (c, expect)
        window_ref.commit(rec, c, want)
        assert ref.rec.tolist() == rec.tolist()
        if want:
            slot = len(taken) % KEEP
            taken.append((c, R.graph_rows(m, R.node_values(m, field))[0]))
            assert ref.hist_clock[slot] == c and ref.hist[slot].tobytes() == taken[-1][1].tobytes()
        else:
            assert all(x.tobytes() == y.tobytes() for x, y in zip((ref.hist, ref.hist_clock, ref.cell_out), before))
    assert [c for c, _ in taken] == [2, 4, 8, 12, 14, 16] and rec[window_ref.N] == 6
    clock, rows, _ = ref.rows()
    assert clock.tolist() == [8, 12, 14, 16] and ref.hist_clock.tolist() == [14, 16, 8, 12]
    # the module's readers put the device's ring in the same order, and name a row's columns as read() documents
    got_clock, got = FI.split_history(int(ref.rec[R.N]), KEEP, torch.from_numpy(ref.hist), torch.from_numpy(ref.hist_clock))
    assert got_clock.tolist() == clock.tolist() and got.numpy().tobytes() == rows.tobytes()
    h = FI.split_columns(got)
    assert set(h) == {"area", "kinetic_energy", "enstrophy", "div_l2", "div_max", "vort_max", "net_outflow", "circulation",
                      "mean_pressure", "inflow", "outflow", "other_flux", "columns"}
    for name, col in (("area", 0), ("kinetic_energy", 1), ("enstrophy", 2), ("net_outflow", 4), ("circulation", 5), ("inflow", 7),
                      ("outflow", 8), ("other_flux", 9), ("div_max", 10), ("vort_max", 11)):
        assert tuple(h[name].shape) == (4, 1) and np.array_equal(h[name].numpy(), rows[:, :, col]), name
    assert np.array_equal(h["div_l2"].numpy(), np.sqrt(rows[:, :, 3] / rows[:, :, 0]))
    assert np.array_equal(h["mean_pressure"].numpy(), rows[:, :, 6] / rows[:, :, 0]) and np.array_equal(h["columns"].numpy(), rows)
    ref.reset()
    assert ref.rec[R.N] == 0 and ref.rec[R.LAST] == -1 and ref.rows()[1].shape == (0, 1, 12)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    from gfv import integrals as FI
    from gfv import lib as L
    from gfv.follow import Follower
    from gfv.integrals import FlowIntegrals
    graphs, plan, m = setup("cyl_cavity_b2")
    assert issubclass(FlowIntegrals, Follower) and FlowIntegrals.KEYWORD == "integrals" and "evaluate()" in FlowIntegrals.NO_ANDERSON
    assert L.FLOW_RECORD == L.WINDOW_RECORD == R.RECORD == 8
    assert (L.FLOW_SUMS, L.FLOW_MAXS, L.FLOW_CHUNK) == (R.SUMS, R.MAXS, R.CHUNK) == (10, 2, 64) and FI.COLUMNS == 12
    # the symbol is declared and bound
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    name = "gfv_flow_integrals"
    assert re.search(r"\bint " + name + r"\(", header) and name in L.declared_symbols()
    assert len(L._SIGNATURES[name][1]) == 24
    for macro, value in (("RECORD", 8), ("SUMS", 10), ("MAXS", 2), ("CHUNK", 64)):
        assert int(re.search(rf"#define GFV_FLOW_{macro} (\d+)", header).group(1)) == value
    pooled = (types.SimpleNamespace(_gfv_pool_plan=object()),) + tuple(graphs[1:])
    # check_handed's order: the type, a follower that is taken, anderson, the graphs
    with pytest.raises(ValueError, match="Rollout: integrals must be a gfv.integrals.FlowIntegrals or None"):
        FlowIntegrals.check_handed("Rollout", dict(keep=4), pooled, 2)
    taken = FlowIntegrals()
    taken._owner = "Rollout"
    with pytest.raises(ValueError, match="this FlowIntegrals is already attached to a Rollout"):
        FlowIntegrals.check_handed("MarchStep", taken, pooled, 2)
    with pytest.raises(ValueError, match=r"Rollout: anderson > 0 together with integrals.*evaluate\(\)"):
        FlowIntegrals.check_handed("Rollout", FlowIntegrals(), pooled, 2)
    with pytest.raises(ValueError, match="DevicePool"):
        FlowIntegrals.check_handed("Rollout", FlowIntegrals(), pooled, 0)
    FlowIntegrals.check_handed("Rollout", None, pooled, 2)
    FlowIntegrals.check_handed("MarchStep", FlowIntegrals(fields=True), graphs, 0)
    # the constructor's arguments
    for keep in (0, -1, 2.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="keep"):
            FlowIntegrals(keep=keep)
    for fields in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="fields"):
            FlowIntegrals(fields=fields)
    for kw, what in ((dict(start=0), "start"), (dict(stride=0), "stride"), (dict(stop=-1), "stop"), (dict(start=1.5), "start")):
        with pytest.raises(ValueError, match=what):
            FlowIntegrals(**kw)
    fi = FlowIntegrals(start=3, stride=2, stop=9, keep=7, fields=True)
    assert (fi.start, fi.stride, fi.stop, fi.enabled, fi.keep, fi.fields) == (3, 2, 9, True, 7, True)
    assert (FlowIntegrals().start, FlowIntegrals().stride, FlowIntegrals().stop, FlowIntegrals().keep, FlowIntegrals().fields) == \
        (1, 1, None, 4096, False)
    fi.set_window(stride=4, stop=None, enabled=False)
    assert (fi.start, fi.stride, fi.stop, fi.enabled) == (3, 4, None, False)
    with pytest.raises(ValueError, match="stride"):
        fi.set_window(stride=0)
    # an object that is not attached; an attach that raised leaves it free
    for call in (fi.read, fi.count, fi.raw, fi.reset, fi.cell_fields):
        with pytest.raises(RuntimeError, match=r"this FlowIntegrals is not attached yet: hand it to Rollout\(..., integrals=\) or "
                                               r"MarchStep\(..., integrals=\)"):
            call()
    xb, clock, owner = torch.zeros(plan.N, 12), torch.zeros(2, dtype=torch.int32), types.SimpleNamespace()
    with pytest.raises(ValueError, match="GPU"):
        fi.attach(owner, graphs, plan, xb, clock, 0)                           # a CPU node state: there is no CPU path
    with pytest.raises(ValueError, match="DevicePool"):
        fi.attach(owner, pooled, plan, xb, clock, 0)
    fi.check_free()
    assert fi.rec is None and fi.tables is None and fi.hist is None and fi.cell_out is None and fi._owner is None
    with pytest.raises(ValueError, match="field"):
        FI.evaluate(graphs, torch.zeros(plan.N, 4))
    with pytest.raises(ValueError, match="fields"):
        FI.evaluate(graphs, torch.zeros(plan.N, 3), fields=1)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        FI.evaluate(graphs, torch.zeros(plan.N, 3))
    with pytest.raises(ValueError, match="face_type has"):
        FI.build_btype(plan, graphs[2].face_type[:-1])


def test_check_followers_with_six_followers_refuses_in_launch_order():
    import inspect
    from gfv import follow
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.integrals import FlowIntegrals
    from gfv.march import MarchStep
    from gfv.probes import Probes
    from gfv.rollout import Rollout
    from gfv.timescheme import TimeScheme
    from gfv.wallforce import WallForces
    graphs, _, _ = setup("cyl_cavity_b2")
    X = [[1.0, 0.2]]
    names = list(inspect.signature(follow.check_followers).parameters)
    assert names[-1] == "probes" and names[-2] == "integrals"                  # probes stays last: every existing call holds
    for owner in (Rollout, MarchStep):
        assert inspect.signature(owner.__init__).parameters["integrals"].default is None
    follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=WallForces(), integrals=FlowIntegrals(),
                           probes=Probes(X, graph=0), time_bc=T.TimeBC(velocity=T.Const()), time_scheme=TimeScheme())
    follow.check_followers("Rollout", graphs, 2)
    # among several, the launch order decides: field_stats, wall_forces, integrals, probes, time_bc, time_scheme
    with pytest.raises(ValueError, match="wall_forces must be"):
        follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=1, integrals=5, probes=2, time_bc=3,
                               time_scheme=4)
    with pytest.raises(ValueError, match="MarchStep: integrals must be"):
        follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=WallForces(), integrals=5, probes=2,
                               time_bc=3, time_scheme=4)
    with pytest.raises(ValueError, match="MarchStep: probes must be"):
        follow.check_followers("MarchStep", graphs, 0, integrals=FlowIntegrals(), probes=2, time_bc=3, time_scheme=4)
    with pytest.raises(ValueError, match="anderson > 0 together with integrals"):
        follow.check_followers("Rollout", graphs, 1, integrals=FlowIntegrals(), probes=Probes(X, graph=0), time_bc=3)
    with pytest.raises(ValueError, match="anderson > 0 together with wall_forces"):
        follow.check_followers("Rollout", graphs, 1, wall_forces=WallForces(), integrals=FlowIntegrals())
    assert "sixth" in follow.__doc__ and "wall_forces, integrals" in follow.__doc__
