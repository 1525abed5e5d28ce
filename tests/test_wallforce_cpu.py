"""Wall forces, the part that needs no GPU (gfv/wallforce.py; tests/wallforce_ref.py is the float64 restatement).

1. selection and launch tables against the restatement on `cyl_b3` and `cyl_cavity_b2`: the default selection holds no
   two-incidence face, the box (0.05, 0.35, 0.08, 0.32) gives 5, 6, 5 and 8, 0 faces per graph, the bodies' surfaces are closed to
   fp32 rounding;
2. every refusal and every window argument;
3. two known answers of the restatement itself on the 2nd-order meshes, where WLSQ reproduces a linear field (the tolerances are
   derived in `linear_case`);
4. the ring at keep = 4 over 11 samples.
"""
import functools

import numpy as np
import pytest
import torch

import cases
import wallforce_ref as R

f32, f64 = np.float32, np.float64
BOX = (0.05, 0.35, 0.08, 0.32)
HALF = (0.05, 0.2, 0.08, 0.32)           # the upstream half of the bodies in BOX: an OPEN selection, sum S != 0
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def setup(which, order="2nd"):
    """-> (graphs, plan, the restatement's arrays) of a case, on the CPU.  Once."""
    from gfv.plan import build_plan
    graphs = cases.make_graphs(which, order=order)
    plan = build_plan(*graphs)
    return graphs, plan, R.mesh_arrays(graphs, plan)


def _tables_equal(t, want):
    for k in ("bnode", "wface", "wchunk_beg", "wchunk_end", "gwchunk_ptr"):
        got = getattr(t, k)
        assert got.dtype == torch.int32 and got.is_contiguous(), k
        assert got.numpy().shape == want[k].shape and (got.numpy() == want[k]).all(), k
    assert t.faces.tolist() == want["faces"].tolist()
    assert (t.Nb, t.Nf, t.n_wchunks) == (len(want["bnode"]), len(want["wface"]), len(want["wchunk_beg"]))


# ---- 1. selection and tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which, box_faces", [("cyl_b3", [5, 6, 5]), ("cyl_cavity_b2", [8, 0])])
def test_selection_and_tables_are_the_restatement(which, box_faces):
    from gfv import wallforce as WF
    graphs, plan, m = setup(which)
    inc = R.incidences(m)
    for box in (None, BOX):
        sel = WF.select_faces(graphs, None, box)
        want = R.select_faces(m, None, box)
        assert sel.dtype == torch.int64 and sel.tolist() == want.tolist()
        assert (m["face_type"][want] == R.WALL_BOUNDARY).all() and (inc[want] == 1).all()          # no two-incidence face
        t = WF.build_tables(plan, sel)
        ref = R.build_tables(m, want)
        _tables_equal(t, ref)
        # the tables' own invariants: end nodes found in bnode, the one incidence is the face's, chunks of <= 64 rows in one graph
        w = ref["wface"].astype(np.int64)
        assert (ref["bnode"][w[:, 2]] == m["es"][w[:, 0]]).all() and (ref["bnode"][w[:, 3]] == m["er"][w[:, 0]]).all()
        assert (m["kface"][w[:, 1]] == w[:, 0]).all() and (np.diff(w[:, 0]) > 0).all() and (np.diff(ref["bnode"]) > 0).all()
        fb = m["batch"][m["es"][w[:, 0]]]
        for q, (b0, b1) in enumerate(zip(ref["wchunk_beg"], ref["wchunk_end"])):
            assert 0 < b1 - b0 <= 64 and len(set(fb[b0:b1])) == 1
            g = int(fb[b0])
            assert ref["gwchunk_ptr"][g] <= q < ref["gwchunk_ptr"][g + 1]
    assert ref["faces"].tolist() == box_faces
    # the bodies inside the box are closed surfaces, to fp32 rounding
    S = m["kS"][w[:, 1]].astype(f64)
    for g in range(m["B"]):
        if box_faces[g]:
            assert np.abs(S[fb == g].sum(0)).max() < 1e-8, (which, g)
    if which == "cyl_b3":
        two = np.nonzero((m["face_type"] == R.WALL_BOUNDARY) & (inc == 2))[0]
        assert int((m["face_type"] == R.WALL_BOUNDARY).sum()) == 205 and len(two) >= 1
        assert not set(two.tolist()) & set(R.select_faces(m).tolist())                             # never selected by default
        with pytest.raises(ValueError, match="incidences"):
            WF.select_faces(graphs, torch.tensor([int(two[0])]), None)                             # refused when named


def test_faces_masks_indices_and_boxes_per_graph():
    from gfv import wallforce as WF
    graphs, plan, m = setup("cyl_b3")
    inbox = R.select_faces(m, None, BOX)
    mask = torch.zeros(m["E"], dtype=torch.bool)
    mask[torch.from_numpy(inbox[::2])] = True
    for faces in (mask, torch.from_numpy(inbox[::2]), torch.from_numpy(inbox[::2]).to(torch.int32), inbox[::2].tolist()):
        assert WF.select_faces(graphs, faces, None).tolist() == inbox[::2].tolist()
    # both given: both must hold; a list of boxes: one per graph
    far = (10.0, 11.0, 10.0, 11.0)
    got = WF.select_faces(graphs, torch.from_numpy(inbox), [BOX, far, BOX])
    want = R.select_faces(m, inbox, [BOX, far, BOX])
    assert got.tolist() == want.tolist()
    t = WF.build_tables(plan, got)
    assert t.faces.tolist() == [5, 0, 5] and t.gwchunk_ptr.tolist() == [0, 1, 1, 2]                # a graph with no face
    _tables_equal(t, R.build_tables(m, want))
    # more than one chunk per graph: the default selection (65, 78 and 61 faces)
    t = WF.build_tables(plan, WF.select_faces(graphs))
    assert t.faces.tolist() == [65, 78, 61] and t.gwchunk_ptr.tolist() == [0, 2, 4, 5]
    assert (t.wchunk_end - t.wchunk_beg).tolist() == [64, 1, 64, 14, 61]


# ---- 2. refusals and window arguments ----------------------------------------------------------------------------------------------
def test_refusals_and_window_arguments():
    from gfv import wallforce as WF
    from gfv.wallforce import WallForces
    graphs, plan, m = setup("cyl_b3")
    # the window: FieldStats' checks, word for word
    for kw, what in ((dict(start=0), "start"), (dict(start=1.5), "start"), (dict(start=True), "start"), (dict(stride=0), "stride"),
                     (dict(stop=-1), "stop"), (dict(start=2 ** 31), "start"), (dict(stride="2"), "stride")):
        with pytest.raises(ValueError, match=what):
            WallForces(**kw)
    wf = WallForces(start=3, stride=2, stop=9, keep=7)
    assert (wf.start, wf.stride, wf.stop, wf.enabled, wf.keep) == (3, 2, 9, True, 7)
    wf.set_window(stride=4)
    assert (wf.start, wf.stride, wf.stop) == (3, 4, 9)
    wf.set_window(stop=None, enabled=False)
    assert wf.stop is None and not wf.enabled
    with pytest.raises(ValueError, match="stride"):
        wf.set_window(stride=0)
    assert wf.stride == 4                                                                          # checked before anything changes
    for keep in (0, -1, 2.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="keep"):
            WallForces(keep=keep)
    for box in ((0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), "abcd", 5, [(0, 1, 0, 1), (0, 1)], (0, 1, 0, float("nan")), []):
        with pytest.raises(ValueError, match="box"):
            WallForces(box=box)
    for origin in ((0,), (0, 1, 2), (0, float("inf")), 3, [(0, 0), (1,)], "ab"):
        with pytest.raises(ValueError, match="origin"):
            WallForces(origin=origin)
    with pytest.raises(ValueError, match="faces"):
        WallForces(faces=torch.zeros(4))                                                           # a float tensor
    # the selection
    with pytest.raises(ValueError, match="no face"):
        WF.select_faces(graphs, None, (10.0, 11.0, 10.0, 11.0))
    with pytest.raises(ValueError, match="no face"):
        WF.select_faces(graphs, torch.zeros(m["E"], dtype=torch.bool), None)
    not_wall = int(np.nonzero(m["face_type"] != R.WALL_BOUNDARY)[0][0])
    with pytest.raises(ValueError, match="not a wall face"):
        WF.select_faces(graphs, torch.tensor([not_wall]), None)
    with pytest.raises(ValueError, match="outside"):
        WF.select_faces(graphs, torch.tensor([m["E"]]), None)
    with pytest.raises(ValueError, match="one entry per face"):
        WF.select_faces(graphs, torch.zeros(3, dtype=torch.bool), None)
    with pytest.raises(ValueError, match="one box per graph"):
        WF.select_faces(graphs, None, [BOX, BOX])
    sel = WF.select_faces(graphs, None, BOX)
    with pytest.raises(ValueError, match="ascending"):
        WF.build_tables(plan, sel.flip(0))
    with pytest.raises(ValueError, match="one .* incidence"):
        WF.build_tables(plan, torch.arange(m["E"]))
    with pytest.raises(ValueError, match="no face"):
        WF.build_tables(plan, torch.zeros(0, dtype=torch.int64))
    # the owners' checks
    WF.check_owner("Rollout", None, graphs, 2)
    with pytest.raises(ValueError, match="WallForces"):
        WF.check_owner("Rollout", dict(box=BOX), graphs)
    with pytest.raises(ValueError, match="anderson"):
        WF.check_owner("Rollout", WallForces(), graphs, 2)

    class Pooled:
        _gfv_pool_plan = object()
    with pytest.raises(ValueError, match="DevicePool"):
        WF.check_owner("MarchStep", WallForces(), (Pooled(),) + tuple(graphs[1:]))
    # an object that is not attached; an attach that fails leaves it free
    wf = WallForces(box=BOX)
    for call in (wf.read, wf.count, wf.raw, wf.reset, lambda: wf.coefficients(0.1)):
        with pytest.raises(RuntimeError, match="not attached"):
            call()
    with pytest.raises(ValueError, match="GPU"):
        wf.attach(object(), graphs, plan, torch.zeros(plan.N, 12), torch.zeros(1, dtype=torch.int32))     # a CPU tensor
    wf.check_free()
    assert wf.rec is None and wf.tables is None
    for kw in (dict(ref_length=0.0), dict(ref_length=0.1, ref_speed=-1.0), dict(ref_length="1")):
        with pytest.raises(ValueError, match="ref_"):
            WF.coefficients({}, **kw)
    with pytest.raises(ValueError, match="field"):
        WF.evaluate(graphs, torch.zeros(plan.N, 4))
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        WF.evaluate(graphs, torch.zeros(plan.N, 3))


def test_coefficients_and_the_order_of_the_ring():
    from gfv import wallforce as WF
    rng = np.random.default_rng(5)
    keep, B = 4, 2
    hist = torch.from_numpy(rng.standard_normal((keep, B, 6)))
    hclock = torch.tensor([9, 10, 7, 8], dtype=torch.int32)                                        # n = 10: rows 6 .. 9 -> slots 2, 3, 0, 1
    clock, rows = WF.split_history(10, keep, hist, hclock)
    assert clock.tolist() == [7, 8, 9, 10] and torch.equal(rows, hist[[2, 3, 0, 1]])
    clock, rows = WF.split_history(3, keep, hist, hclock)
    assert clock.tolist() == [9, 10, 7] and torch.equal(rows, hist[0:3])
    assert WF.split_history(0, keep, hist, hclock)[1].shape == (0, B, 6)
    h = {"clock": clock, "pressure": rows[:, :, 0:2], "viscous": rows[:, :, 2:4], "moment": rows[:, :, 4:6]}
    c = WF.coefficients(h, ref_length=0.1, ref_speed=2.0)
    q = 0.5 * 2.0 * 2.0 * 0.1
    assert torch.equal(c["cd"], (rows[:, :, 0] + rows[:, :, 2]) / q) and torch.equal(c["cl"], (rows[:, :, 1] + rows[:, :, 3]) / q)
    assert torch.equal(c["cm"], (rows[:, :, 4] + rows[:, :, 5]) / (q * 0.1)) and c["cd"].shape == (3, B)


# ---- 3. two known answers ----------------------------------------------------------------------------------------------------------
# Linear fields phi_c(x) = C[c, 0] + C[c, 1] x + C[c, 2] y per graph; the node state holds fl32(dim_c * phi_c): what the launches
# divide again.
COEF = np.array([[[0.3, -0.7, 0.45], [-0.2, 0.6, 0.9], [1.1, 2.5, 0.0]],
                 [[-0.4, 0.8, -0.35], [0.5, -1.2, 0.3], [-0.6, -1.75, 0.0]],
                 [[0.1, 0.25, 1.3], [0.7, 0.55, -0.8], [0.9, 3.0, 0.0]]])


def linear_case(which, box):
    """-> dict: the mesh arrays, the tables of the selection, the field [N, 12] fp32, and per graph the exact answers with their
    tolerances.

    The answers.  WLSQ of 2nd order reproduces a linear field, so g = C[c, 1:3] at every node and the face values are phi_c at the
    face centre.  Viscous, any selection: Fv[c] = -theta4 * (C[c, 1:3] . sum_f S_f), with the sum over the fp32 vectors the launch
    reads (no geometry enters).  Pressure, phi_p = a + b x on a CLOSED body whose S point into it: sum_f phi_p(x_f) S_f =
    -integral of grad p over the body = -(b V, 0), so Fp = (-theta3 b V, 0) with V the shoelace area of the body's polygon.

    The tolerances, from the precision of the data alone (u = 2^-24):
      * the node value the launches see is fl32(fl32(dim * phi) / dim) = phi (1 + d), |d| <= 2.01 u, so every difference of the
        right-hand side is off by at most 2 eps, eps = 2.01 u max|phi_c|;
      * A / rn has rows of unit norm, so || (A / rn)^-1 ||_2 <= cond_2(A / rn) = kappa_i, and the gradient at node i is off by at most
        e_i = kappa_i * || sum_s |B_s| / rn ||_2 * 2 eps; e = the largest over the body nodes;
      * viscous: |dFv[c]| <= theta4 * e * sum_f (|S_x| + |S_y|);
      * pressure: the face value is off by at most eps + rho_f e, rho_f the larger 1-norm of the two offsets, so |dFp| <= theta3 *
        sum_f (eps + rho_f e) |S|; and the discrete surface is the polygon only to the rounding of its fp32 data: the face centres
        (1 u relative) and the vectors S (a normal times a length, each rounded: 4 u relative is generous for a product of two
        fp32 numbers formed from float64 geometry), which moves sum_f x_f S_f by at most 5 u |b| sum_f |x_f| |S_f|, and the open
        remainder |a| |sum_f S_f| of a surface closed only to rounding.
    """
    graphs, plan, m = setup(which)
    sel = R.select_faces(m, None, box)
    t = R.build_tables(m, sel)
    B = m["B"]
    pos = m["pos"].astype(f64)
    C = COEF[:B]
    b = m["batch"]
    phi = C[b, :, 0] + C[b, :, 1] * pos[:, 0:1] + C[b, :, 2] * pos[:, 1:2]                          # [N, 3] float64
    field = np.zeros((m["N"], 12), dtype=f32)
    field[:, 0:3] = (m["uvp_dim"][b].astype(f64) * phi).astype(f32)
    q, cond = R.gradient_bounds(m, t["bnode"], field)                                              # (cond only)
    w = t["wface"].astype(np.int64)
    fb = b[m["es"][w[:, 0]]]
    S = m["kS"][w[:, 1]].astype(f64)
    out = {"m": m, "t": t, "sel": sel, "field": field, "graphs": graphs, "exact": np.zeros((B, 4)), "tol": np.zeros((B, 4)),
           "closed": [bool((fb == g).any()) and box == BOX for g in range(B)]}
    for g in range(B):
        rows = fb == g
        if not rows.any():
            continue
        th3, th4 = float(m["theta"][g, 3]), float(m["theta"][g, 4])
        nodes = t["bnode"][np.unique(w[rows][:, 2:4])].astype(np.int64)
        e = np.zeros(3)
        eps = 2.01 * U32 * np.abs(phi[b == g]).max(0)                                              # [3]
        for i in nodes:
            s0, s1 = m["x_rowptr"][i], m["x_rowptr"][i + 1]
            a = np.linalg.norm(np.abs(m["x_B"][s0:s1].astype(f64)).sum(0) / m["rn"][i].astype(f64))
            kappa = np.linalg.cond(m["An"][i].astype(f64) / m["rn"][i].astype(f64)[:, None])
            e = np.maximum(e, kappa * a * 2.0 * eps)
        Sg = S[rows]
        S1 = np.abs(Sg).sum()
        out["exact"][g, 2:4] = -th4 * (C[g, 0:2, 1:3] @ Sg.sum(0))
        out["tol"][g, 2:4] = th4 * e[0:2] * S1
        if out["closed"][g]:
            V = R.shoelace_area(m, sel[rows])
            f = w[rows][:, 0]
            rho = np.maximum(np.abs(m["fpos"][f].astype(f64) - pos[m["es"][f]]).sum(1),
                             np.abs(m["fpos"][f].astype(f64) - pos[m["er"][f]]).sum(1))
            xf = np.abs(m["fpos"][f].astype(f64)[:, 0:1])
            geo = 5 * U32 * abs(C[g, 2, 1]) * (xf * np.abs(Sg)).sum(0) + abs(C[g, 2, 0]) * np.abs(Sg.sum(0))
            out["exact"][g, 0:2] = (-th3 * C[g, 2, 1] * V, 0.0)
            out["tol"][g, 0:2] = th3 * (((eps[2] + rho * e[2])[:, None] * np.abs(Sg)).sum(0) + geo)
    return out


@pytest.mark.parametrize("which", ["cyl_b3", "cyl_cavity_b2"])
def test_known_answers_of_the_restatement(which):
    for box in (BOX, HALF):
        k = linear_case(which, box)
        m, t = k["m"], k["t"]
        gb = R.gradients(m, t["bnode"], k["field"])
        sums, _ = R.graph_sums(m, t["wface"], np.zeros((m["B"], 2), dtype=f32), k["field"], gb)
        for g in range(m["B"]):
            if not t["faces"][g]:
                assert (sums[g] == 0).all()
                continue
            err = np.abs(sums[g, 0:4] - k["exact"][g])
            print(f"{which} box={box} graph {g}: exact {k['exact'][g]}, err {err}, tol {k['tol'][g]}")
            assert (err[2:4] <= k["tol"][g, 2:4]).all(), (which, g, "viscous")
            if k["closed"][g]:
                assert (err[0:2] <= k["tol"][g, 0:2]).all(), (which, g, "pressure")
                assert abs(k["exact"][g, 0]) > 100 * k["tol"][g, 0]                                # the tolerance decides something
            else:
                assert (np.abs(k["exact"][g, 2:4]) > 10 * k["tol"][g, 2:4]).all()                  # (an open arc: sum S != 0)


# ---- 4. the ring -------------------------------------------------------------------------------------------------------------------
def test_the_ring_at_keep_4_over_11_samples():
    from gfv import wallforce as WF
    graphs, plan, m = setup("cyl_cavity_b2")
    t = R.build_tables(m, R.select_faces(m, None, BOX))
    rng = np.random.default_rng(11)
    ref = R.WallForcesRef(m, t, (0.2, 0.2), keep=4)
    fields = [rng.standard_normal((m["N"], 3)).astype(f32) for _ in range(11)]
    single = []
    for c, fld in enumerate(fields, start=1):
        assert ref.launch(fld, c)
        assert not ref.launch(fld, c)                                                              # an unchanged clock adds nothing
        single.append(R.graph_sums(m, t["wface"], ref.origin, fld, R.gradients(m, t["bnode"], fld))[0])
    assert ref.rec.tolist() == [1, 1, -1, 11, 11, 0, 1, 0]
    assert ref.hist_clock.tolist() == [9, 10, 11, 8]                                               # slot = sample % 4
    clock, rows, _ = ref.rows()
    assert clock.tolist() == [8, 9, 10, 11]
    for k, c in enumerate(clock):
        assert rows[k].tobytes() == single[c - 1].tobytes()
    assert (rows[:, 1] == 0).all() and np.abs(rows[:, 0]).min() > 0                                # graph 1 has no face in the box
    # the module's reader puts the device's ring in the same order
    got_clock, got = WF.split_history(int(ref.rec[R.N]), 4, torch.from_numpy(ref.hist), torch.from_numpy(ref.hist_clock))
    assert got_clock.tolist() == clock.tolist() and got.numpy().tobytes() == rows.tobytes()
    ref.reset()
    assert ref.rec[R.N] == 0 and ref.rec[R.LAST] == -1 and ref.rows()[1].shape == (0, 2, 6)
