"""Probes, the part that needs no GPU (gfv/probes.py; tests/probes_ref.py is the float64 restatement).

1. location against a brute-force restatement on `cyl_cavity_b2`, `cavity_mixed_b1` and `cyl_b3`: 400 seeded random points per graph
   in its bounding box land in identical cells; the points inside a cylinder are refused, the first one named; every centroid
   locates to its own cell; the stored centre of an interior face goes to the lower-indexed of its two cells; `graph=None` with
   more than one graph is refused; `line()` ends exactly on its end points;
2. the weight tables at all four orders on `cyl_b3`: ascending and unique nodes, the same bytes from two builds, the weights' sums,
   and `weights @ phi` against the restatement that solves with the right-hand side (the bound: `probes_ref.combined_bound`);
3. two known answers at 2nd order, a linear and a quadratic field (the tolerances are derived in `known_case`);
4. the record and the ring over the clock script of the window tests, past a wrap of a ring of 4;
5. every refusal that needs no GPU, in `check_handed`'s order, and `check_followers` with five followers.
"""
import functools
import types

import numpy as np
import pytest
import torch

import cases
import probes_ref as R
import wallforce_ref as W
import window_ref
from test_wallforce_cpu import COEF

f32, f64 = np.float32, np.float64
U32 = R.U32
CASES3 = ("cyl_cavity_b2", "cavity_mixed_b1", "cyl_b3")


@functools.lru_cache(maxsize=None)
def setup(which, order="2nd"):
    """-> (graphs, plan, the restatement's arrays) of a case, on the CPU.  Once."""
    from gfv.plan import build_plan
    graphs = cases.make_graphs(which, order=order)
    plan = build_plan(*graphs)
    return graphs, plan, R.mesh_arrays(graphs, plan)


def box_points(m, b, n, seed):
    """n seeded random points in the bounding box of graph b's nodes."""
    nodes = m["pos"][m["batch"] == b].astype(f64)
    lo, hi = nodes.min(0), nodes.max(0)
    return lo + np.random.default_rng(seed).random((n, 2)) * (hi - lo)


@functools.lru_cache(maxsize=None)
def accepted_points(which, per_graph, seed):
    """The first `per_graph` of a graph's random box points that lie in the mesh, for every graph: (points [P, 2], graph [P])."""
    _, _, m = setup(which)
    pts, gr = [], []
    for b in range(m["B"]):
        cand = box_points(m, b, 4 * per_graph, seed + b)
        ok = [x for x in cand if R.locate(m, x, b)[1] <= 1e-6][:per_graph]
        assert len(ok) == per_graph
        pts += ok
        gr += [b] * per_graph
    return np.array(pts), gr


# ---- 1. location -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES3)
def test_location_is_the_brute_force_restatement(which):
    from gfv import probes as PR
    graphs, plan, m = setup(which)
    for C in range(m["C"]):                                                    # the premise of the equal weights: distinct vertices
        V = R.vertices(m, C)
        assert len(set(V.tolist())) == len(V) >= 3
    inside_total = 0
    for b in range(m["B"]):
        pts = box_points(m, b, 400, 100 + b)
        ref = [R.locate(m, x, b) for x in pts]
        outside = np.array([r[1] for r in ref])
        bad = outside > 1e-6
        # a point in the mesh lies in exactly one cell; a point inside the cylinder in none, and far from every cell
        assert all(r[2] == 1 for r, o in zip(ref, bad) if not o) and all(r[2] == 0 for r, o in zip(ref, bad) if o)
        assert (outside[bad] >= 0.01).all() and int(bad.sum()) <= 8
        inside_total += int(bad.sum())
        cell, out, gr = PR.locate(plan, pts[~bad], b if m["B"] > 1 else None)
        assert cell.dtype == torch.int64 and out.dtype == torch.float64 and gr.tolist() == [b] * int((~bad).sum())
        assert cell.tolist() == [r[0] for r, o in zip(ref, bad) if not o]
        assert np.abs(out.numpy() - outside[~bad]).max() <= 4 * 2.0 ** -53 * np.abs(outside).max()
        assert (out.numpy() <= 0).all()
        if bad.any():
            first = int(np.nonzero(bad)[0][0])
            with pytest.raises(ValueError, match=rf"{int(bad.sum())} of 400 points lie outside the mesh; point {first} \("):
                PR.locate(plan, pts, b)
            cell, out, _ = PR.locate(plan, pts, b, tolerance=1.0)              # a tolerance of a whole cell accepts them, unmoved
            assert cell.tolist() == [r[0] for r in ref]
    assert inside_total >= (1 if which.startswith("cyl") else 0)
    # every centroid locates to its own cell
    cell, out, _ = PR.locate(plan, plan.centroid.to(torch.float64), plan.cbatch.tolist())
    assert cell.tolist() == list(range(m["C"])) and float(out.max()) < -0.05
    # the stored centre of an interior face: d = 0 exactly in both neighbours, the lower index wins
    kcell = np.repeat(np.arange(m["C"]), np.diff(m["crow"]))
    faces = np.nonzero(W.incidences(m) == 2)[0]
    assert len(faces) > m["C"]
    two = np.array([np.sort(kcell[m["kface"] == f]) for f in faces])           # [F, 2]
    assert (two[:, 0] < two[:, 1]).all()
    fb = m["batch"][m["es"][faces]]
    cell, out, _ = PR.locate(plan, m["fpos"][faces].astype(f64), fb.tolist())
    assert cell.tolist() == two[:, 0].tolist() and (out.numpy() == 0).all()
    for f, (lo, hi) in list(zip(faces, two))[::37]:
        x = m["fpos"][f].astype(f64)
        assert R.cell_distance(m, lo, x) == 0 and R.cell_distance(m, hi, x) == 0 and R.locate(m, x, fb[faces == f][0])[0] == lo


def test_centroids_of_the_polygon_mesh_locate_to_their_own_cells():
    """Cells of 3 to 9 vertices, not all of them convex.  Over all 17436 centroids (a run of a quarter of a minute, made once): 17436
    locate to their own cell, the largest `outside` is -0.133; here every 16th."""
    from gfv import probes as PR
    from gfv.plan import build_plan
    graphs, _, _ = cases.poly_cylinder()
    plan = build_plan(*graphs)
    assert plan.C == 17436 and plan.B == 1
    own = torch.arange(plan.C)[::16]
    cell, outside, gr = PR.locate(plan, plan.centroid.to(torch.float64)[::16])
    assert cell.tolist() == own.tolist() and float(outside.max()) < -0.1 and gr.tolist() == [0] * len(own)


def test_graph_arguments_and_line():
    from gfv import probes as PR
    _, plan3, m3 = setup("cyl_b3")
    _, plan1, _ = setup("cavity_mixed_b1")
    x = [[0.5, 0.3]]
    with pytest.raises(ValueError, match="graph=None needs a batch of one graph; this batch has 3"):
        PR.locate(plan3, x)
    assert PR.locate(plan1, x)[2].tolist() == [0]                              # B == 1: None is graph 0
    for graph, what in ((3, "outside 0 .. 2"), (-1, "outside 0"), ([0, 1], "one int per point"), (1.0, "graph must be"),
                        (True, "graph must be"), ([0.5], "graph must be"), (torch.tensor([0.0]), "graph must be")):
        with pytest.raises(ValueError, match=what):
            PR.locate(plan3, x, graph)
    # the graphs of a batch overlap in space: one point, three graphs, three cells
    cells = [int(PR.locate(plan3, [[1.0, 0.2]], b)[0][0]) for b in range(3)]
    assert all(m3["gcell_ptr"][b] <= c < m3["gcell_ptr"][b + 1] for b, c in enumerate(cells))
    cell, _, gr = PR.locate(plan3, [[1.0, 0.2]] * 3, torch.tensor([0, 1, 2], dtype=torch.int32))
    assert cell.tolist() == cells and gr.tolist() == [0, 1, 2]
    # line(): both end points included, and exactly
    p0, p1 = (0.1, 0.7), (0.3, 0.123456789)
    ln = PR.line(p0, p1, 7)
    assert ln.dtype == torch.float64 and tuple(ln.shape) == (7, 2)
    assert ln[0].tolist() == list(p0) and ln[-1].tolist() == list(p1)
    step = ln[1:] - ln[:-1]
    assert float((step - step[0]).abs().max()) <= 4 * 2.0 ** -53
    assert PR.line(p0, p1, 2).tolist() == [list(p0), list(p1)]
    for n in (1, 0, 2.0, True):
        with pytest.raises(ValueError, match="line"):
            PR.line(p0, p1, n)
    with pytest.raises(ValueError, match="points"):
        PR.line(p0, (0.0, float("nan")), 3)


# ---- 2. the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order, terms", [("1st", 2), ("2nd", 5), ("3rd", 9), ("4th", 14)])
def test_tables_are_the_restatement_with_the_right_hand_side(order, terms):
    from gfv import probes as PR
    graphs, plan, m = setup("cyl_b3", order)
    assert plan.M == terms
    pts, gr = accepted_points("cyl_b3", 8, 300)
    node = int(np.nonzero(m["batch"] == 1)[0][40])                             # a probe AT a node, and one at a face centre
    face = int(np.nonzero((W.incidences(m) == 2) & (m["batch"][m["es"]] == 2))[0][10])
    pts = np.concatenate((pts, m["pos"][[node]].astype(f64), m["fpos"][[face]].astype(f64)))
    gr = gr + [1, 2]
    P = len(gr)
    cell, outside, _ = PR.locate(plan, pts, gr)
    t = PR.build_tables(plan, pts, cell)
    again = PR.build_tables(plan, torch.from_numpy(pts), cell.clone())
    for k in ("pw_ptr", "pw_node", "pw_w"):
        a, b = getattr(t, k), getattr(again, k)
        assert a.dtype == b.dtype and a.is_contiguous() and a.numpy().tobytes() == b.numpy().tobytes(), k      # the same bytes
    assert t.pw_ptr.dtype == torch.int32 and t.pw_node.dtype == torch.int32 and t.pw_w.dtype == torch.float64
    ptr, nodes, w = t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy()
    assert tuple(ptr.shape) == (P + 1,) and ptr[0] == 0 and ptr[-1] == len(nodes) == t.nnz and tuple(w.shape) == (t.nnz, 3)
    rng = np.random.default_rng(50 + terms)
    field = (rng.standard_normal((m["N"], 12)) * 10.0 ** rng.uniform(-1.0, 1.0, (m["N"], 12))).astype(f32)
    rows, mag = R.dot_rows(ptr, nodes, w, W.node_values(m, field))
    worst, decides = 0.0, []
    for p in range(P):
        seg, wp = nodes[ptr[p]:ptr[p + 1]], w[ptr[p]:ptr[p + 1]]
        nnz = len(seg)
        assert nnz >= 3 and (np.diff(seg) > 0).all()                          # ascending and unique
        assert (m["batch"][seg] == gr[p]).all() and set(R.vertices(m, int(cell[p])).tolist()) <= set(seg.tolist())
        sums, room = wp.sum(0), (nnz + 16) * R.U * np.abs(wp).sum(0)
        assert abs(sums[0] - 1.0) <= room[0] and abs(sums[1]) <= room[1] and abs(sums[2]) <= room[2], (p, sums, room)
        val, g = R.value_gradient(m, int(cell[p]), pts[p], field)
        want = np.concatenate((val[:, None], g), 1).reshape(-1)                # q = 3 c + j
        bound = R.combined_bound(m, int(cell[p]), pts[p], field, nnz, mag[p])
        err = np.abs(rows[p] - want)
        assert (err <= bound).all(), (order, p, err, bound)
        decides.append(bool((np.abs(want) > 1e4 * bound).any()))
        worst = max(worst, float((err / bound).max()))
    # the bound decides something: at 2nd order at every probe; the 9- and 14-term systems of some boundary vertices are close to
    # singular (kappa above 1e12), and the bound says so
    assert all(decides) if order in ("1st", "2nd") else sum(decides) > P // 2, (order, decides)
    print(f"{order}: {t.nnz / P:.1f} entries per probe, weights @ phi against the restatement: largest error / bound {worst:.3g}")


# ---- 3. two known answers ----------------------------------------------------------------------------------------------------------
# phi_c(x) = C[c, 0] + C[c, 1:3] . x (+ 1/2 x^T H_c x) per graph, C = test_wallforce_cpu's COEF; the node state holds
# fl32(dim_c * phi_c): what the launch divides again.  H: a curvature across the channel that dominates, as in a Poiseuille profile.
HESS = np.array([[[0.2, 0.3], [0.3, -3.0]], [[-0.3, 0.25], [0.25, 2.4]], [[0.15, -0.2], [-0.2, 2.0]]])


@functools.lru_cache(maxsize=None)
def known_case(which, quadratic):
    """-> dict: the mesh arrays, graphs, the probes (12 random points and the centroids of the 4 largest cells per graph), the field
    [N, 12] fp32, and per probe the exact value [P, 3] and gradient [P, 3, 2] of the header's formulas with their tolerances, and the
    correction term.

    The answers.  WLSQ of 2nd order (5 terms) reproduces a quadratic field, so g_v = b + H pos[v] at every vertex.  Linear field:
    value = phi(x), gradient = b.  Quadratic: phi(v) + g_v . (x - pos[v]) = phi(x) - 1/2 (x - pos[v])^T H (x - pos[v]) (the Taylor
    expansion of a quadratic about v, exact), so value = phi(x) - (1 / k) sum_v 1/2 (x - pos[v])^T H (x - pos[v]) - the `correction`,
    which pins the EQUAL weights - and gradient = the mean of b + H pos[v].

    The tolerances, from the precision of the data alone (u = 2^-24), in the way of test_wallforce_cpu.linear_case:
      * the node value the launch sees is fl32(fl32(dim * phi) / dim) = phi (1 + d), |d| <= 2.01 u: every node value is off by at
        most eps = 2.01 u max|phi_c| (over the graph), every difference of the right-hand side by 2 eps;
      * the stencil is fp32 data: x_B and An are each the rounding of the numbers for which the reproduction is exact, off by at
        most u relative, entry by entry.  With A = An / rn and the exact solution s (the Taylor coefficients), (A + dA) g = rhs +
        drhs gives, to first order, |A (g - s)| <= |drhs| + |dA| |s| <= sum_s |B_s| (2 eps + u |dphi_s|) / rn + u |A| |s|;
      * A has rows of unit norm, so || A^-1 ||_2 <= cond_2(A) = kappa_v, and the gradient at vertex v is off by at most
        e_v = kappa_v * ( || sum_s |B_s| / rn ||_2 * 2 eps + u * ( || sum_s |B_s| |dphi_s| / rn ||_2 + || |A| |s| ||_2 ) ),
        with |s| taken from the float64 solution of the restatement's system (it differs from s by e_v itself: second order);
      * gradient: (1 / k) sum_v e_v;  value: eps + (1 / k) sum_v e_v |x - pos[v]|_1.
    The positions are the fp32 numbers the plan holds, taken as exact: the fields are DEFINED on them.
    """
    graphs, plan, m = setup(which)
    B, b = m["B"], m["batch"]
    pos = m["pos"].astype(f64)
    C = COEF[:B]
    H = HESS if quadratic else np.zeros_like(HESS)
    phi = C[b, :, 0] + C[b, :, 1] * pos[:, 0:1] + C[b, :, 2] * pos[:, 1:2] + 0.5 * np.einsum("na,cab,nb->nc", pos, H, pos)
    field = np.zeros((m["N"], 12), dtype=f32)
    field[:, 0:3] = (m["uvp_dim"][b].astype(f64) * phi).astype(f32)
    pts, gr = accepted_points(which, 12, 700)
    pts, gr = list(pts), list(gr)
    for g in range(B):
        c0, c1 = int(m["gcell_ptr"][g]), int(m["gcell_ptr"][g + 1])
        for cell in c0 + np.argsort(-m["area"][c0:c1], kind="stable")[:4]:
            pts.append(pos[R.vertices(m, cell)].mean(0))
            gr.append(g)
    pts = np.array(pts)
    P = len(gr)
    out = {"m": m, "graphs": graphs, "plan": plan, "points": pts, "graph": gr, "field": field, "cell": [],
           "value": np.zeros((P, 3)), "gradient": np.zeros((P, 3, 2)), "tol_value": np.zeros((P, 3)),
           "tol_gradient": np.zeros((P, 3)), "correction": np.zeros((P, 3)), "kappa": 0.0}
    eps_g = np.stack([2.01 * U32 * np.abs(phi[b == g]).max(0) for g in range(B)])                   # [B, 3]
    e_of = {}

    def e_vertex(v, eps):
        if v not in e_of:
            s0, s1 = m["x_rowptr"][v], m["x_rowptr"][v + 1]
            rn = m["rn"][v].astype(f64)
            Bs = m["x_B"][s0:s1].astype(f64)
            A = m["An"][v].astype(f64) / rn[:, None]
            d = phi[m["x_out"][s0:s1]] - phi[v]                                                     # [S, 3]
            sol = np.linalg.solve(A, (Bs.T @ d) / rn[:, None])                                      # [M, 3]
            kappa = np.linalg.cond(A)
            a = np.linalg.norm(np.abs(Bs).sum(0) / rn)
            q = np.linalg.norm((np.abs(Bs).T @ np.abs(d)) / rn[:, None], axis=0)                    # [3]
            r = np.linalg.norm(np.abs(A) @ np.abs(sol), axis=0)                                     # [3]
            e_of[v] = kappa * (a * 2.0 * eps + U32 * (q + r))
            out["kappa"] = max(out["kappa"], float(kappa))
        return e_of[v]

    for p in range(P):
        g, x = gr[p], pts[p]
        cell = R.locate(m, x, g)[0]
        V = R.vertices(m, cell)
        off = x - pos[V]                                                                            # [k, 2]
        out["cell"].append(cell)
        corr = 0.5 * np.einsum("va,cab,vb->c", off, H, off) / len(V)
        at_x = C[g, :, 0] + C[g, :, 1:3] @ x + 0.5 * np.einsum("a,cab,b->c", x, H, x)
        out["correction"][p] = corr
        out["value"][p] = at_x - corr
        out["gradient"][p] = (C[g, :, 1:3][None] + np.einsum("cab,vb->vca", H, pos[V])).mean(0)
        e = np.stack([e_vertex(int(v), eps_g[g]) for v in V])                                       # [k, 3]
        out["tol_gradient"][p] = e.mean(0)
        out["tol_value"][p] = eps_g[g] + (e * np.abs(off).sum(1)[:, None]).mean(0)
    return out


def check_known(k, value, gradient, extra_value=0.0, extra_gradient=0.0, what=""):
    """value [P, 3], gradient [P, 3, 2] against the exact answers of a known_case within its tolerances (+ `extra`, the caller's own
    rounding).  Prints the figures, then asserts."""
    ev = np.abs(value - k["value"])
    eg = np.abs(gradient - k["gradient"]).max(2)
    tv, tg = k["tol_value"] + extra_value, k["tol_gradient"] + extra_gradient
    print(f"{what}: kappa <= {k['kappa']:.3g}; value: largest error {ev.max():.3g}, error / tolerance {(ev / tv).max():.3g}; "
          f"gradient: largest error {eg.max():.3g}, error / tolerance {(eg / tg).max():.3g}; "
          f"largest correction / tolerance {(np.abs(k['correction']) / tv).max():.3g}")
    assert (ev <= tv).all(), (what, "value", ev, tv)
    assert (eg <= tg).all(), (what, "gradient", eg, tg)


@pytest.mark.parametrize("which", CASES3)
@pytest.mark.parametrize("quadratic", [False, True], ids=["linear", "quadratic"])
def test_known_answers(which, quadratic):
    from gfv import probes as PR
    k = known_case(which, quadratic)
    m, pts, gr = k["m"], k["points"], k["graph"]
    cell, _, _ = PR.locate(k["plan"], pts, gr)
    assert cell.tolist() == k["cell"]
    t = PR.build_tables(k["plan"], pts, cell)
    rows, mag = R.dot_rows(t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy(), W.node_values(m, k["field"]))
    nnz = np.diff(t.pw_ptr.numpy())
    r = rows.reshape(-1, 3, 3)
    room = ((nnz[:, None] + 16.0) * R.U * mag).reshape(-1, 3, 3)               # the double arithmetic of tables and sum
    check_known(k, r[:, :, 0], r[:, :, 1:3], room[:, :, 0], room[:, :, 1:3].max(2), f"{which} tables")
    # ... and the restatement that solves with the right-hand side
    vg = [R.value_gradient(m, c, x, k["field"]) for c, x in zip(k["cell"], pts)]
    check_known(k, np.stack([v for v, _ in vg]), np.stack([g for _, g in vg]), room[:, :, 0], room[:, :, 1:3].max(2),
                f"{which} restatement")
    if quadratic:
        # the tolerance decides something: the equal-weight correction stands 100 tolerances tall at some probe, and an answer
        # without it is refused
        assert (np.abs(k["correction"]) > 100.0 * (k["tol_value"] + room[:, :, 0])).any()
        with pytest.raises(AssertionError):
            check_known(dict(k, value=k["value"] + k["correction"]), r[:, :, 0], r[:, :, 1:3], room[:, :, 0], room[:, :, 1:3].max(2))
    else:
        assert (k["correction"] == 0).all() and (np.abs(k["value"]) > 1e3 * k["tol_value"]).any()


# ---- 4. the record and the ring ----------------------------------------------------------------------------------------------------
def test_record_and_ring_over_the_clock_script_past_a_wrap():
    from gfv import probes as PR
    from test_wallforce_gpu import SCRIPT                                      # the window tests' script, then past a ring of 4
    _, plan, m = setup("cyl_cavity_b2")
    pts, gr = accepted_points("cyl_cavity_b2", 3, 900)
    cell, _, _ = PR.locate(plan, pts, gr)
    t = PR.build_tables(plan, pts, cell)
    KEEP, P = 4, len(gr)
    ref = R.ProbesRef(t.pw_ptr.numpy(), t.pw_node.numpy(), t.pw_w.numpy(), m["uvp_dim"], m["batch"], KEEP, start=2, stride=2)
    rec = ref.rec.copy()                                                       # window_ref alone, beside it
    rng = np.random.default_rng(3)
    taken = []
    for words, c, expect in SCRIPT:
        for name, v in (words or {}).items():
            ref.rec[getattr(R, name)] = rec[getattr(window_ref, name)] = v
        field = rng.standard_normal((m["N"], 12)).astype(f32)
        before = (ref.hist.copy(), ref.hist_clock.copy())
        want = window_ref.take(rec, c)
        assert ref.launch(field, c) is want is expect, (c, expect)
        window_ref.commit(rec, c, want)
        assert ref.rec.tolist() == rec.tolist()
        if want:
            slot = len(taken) % KEEP
            taken.append((c, R.dot_rows(ref.ptr, ref.node, ref.w, ref.phi(field))[0]))
            assert ref.hist_clock[slot] == c and ref.hist[slot].tobytes() == taken[-1][1].tobytes()
        else:
            assert ref.hist.tobytes() == before[0].tobytes() and ref.hist_clock.tolist() == before[1].tolist()
    assert [c for c, _ in taken] == [2, 4, 8, 12, 14, 16] and rec[window_ref.N] == 6
    clock, rows, _ = ref.rows()
    assert clock.tolist() == [8, 12, 14, 16] and ref.hist_clock.tolist() == [14, 16, 8, 12]
    assert all(rows[i].tobytes() == taken[2 + i][1].tobytes() for i in range(4))
    # the module's readers put the device's ring in the same order, and split a row as read() documents
    got_clock, got = PR.split_history(int(ref.rec[R.N]), KEEP, torch.from_numpy(ref.hist), torch.from_numpy(ref.hist_clock))
    assert got_clock.tolist() == clock.tolist() and got.numpy().tobytes() == rows.tobytes()
    value, gradient = PR.split_rows(got)
    assert tuple(value.shape) == (4, P, 3) and tuple(gradient.shape) == (4, P, 3, 2)
    r = rows.reshape(4, P, 3, 3)
    assert np.array_equal(value.numpy(), r[..., 0]) and np.array_equal(gradient.numpy(), r[..., 1:3])
    h = {"gradient": gradient}
    assert np.array_equal(PR.vorticity(h).numpy(), r[:, :, 1, 1] - r[:, :, 0, 2])                  # v_x - u_y
    assert np.array_equal(PR.divergence(h).numpy(), r[:, :, 0, 1] + r[:, :, 1, 2])                 # u_x + v_y
    ref.reset()
    assert ref.rec[R.N] == 0 and ref.rec[R.LAST] == -1 and ref.rows()[1].shape == (0, P, 9)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    from gfv import lib as L
    from gfv import probes as PR
    from gfv.follow import Follower
    from gfv.probes import Probes
    graphs, plan, m = setup("cyl_cavity_b2")
    X = [[1.0, 0.2]]
    assert issubclass(Probes, Follower) and Probes.KEYWORD == "probes" and "sample()" in Probes.NO_ANDERSON
    assert L.PROBE_RECORD == L.WINDOW_RECORD == R.RECORD == 8 and L.PROBE_SUMS == R.SUMS == 9
    assert "gfv_probe_sample" in L.declared_symbols()
    pooled = (types.SimpleNamespace(_gfv_pool_plan=object()),) + tuple(graphs[1:])
    # check_handed's order: the type, a follower that is taken, anderson, the graphs
    with pytest.raises(ValueError, match="Rollout: probes must be a gfv.probes.Probes or None"):
        Probes.check_handed("Rollout", dict(points=X), pooled, 2)
    taken = Probes(X, graph=5)
    taken._owner = "Rollout"
    with pytest.raises(ValueError, match="this Probes is already attached to a Rollout"):
        Probes.check_handed("MarchStep", taken, pooled, 2)
    with pytest.raises(ValueError, match=r"Rollout: anderson > 0 together with probes.*sample\(\)"):
        Probes.check_handed("Rollout", Probes(X, graph=5), pooled, 2)
    with pytest.raises(ValueError, match="DevicePool"):
        Probes.check_handed("Rollout", Probes(X, graph=5), pooled, 0)
    with pytest.raises(ValueError, match="outside 0 .. 1"):
        Probes.check_handed("Rollout", Probes(X, graph=5), graphs, 0)
    with pytest.raises(ValueError, match="graph=None needs a batch of one graph"):
        Probes.check_handed("Rollout", Probes(X), graphs, 0)
    Probes.check_handed("Rollout", None, pooled, 2)
    Probes.check_handed("MarchStep", Probes(X, graph=1), graphs, 0)
    # the constructor's arguments
    for points in ([], [[0.0, 1.0, 2.0]], [0.0, 1.0], [[0.0, float("nan")]], [[float("inf"), 0.0]], "ab", None, [["a", "b"]]):
        with pytest.raises(ValueError, match="points"):
            Probes(points)
    for graph in (-1, 1.5, True, [0, 1], "0", [[0]], torch.tensor([0.0])):
        with pytest.raises(ValueError, match="graph"):
            Probes(X, graph=graph)
    for keep in (0, -1, 2.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="keep"):
            Probes(X, keep=keep)
    for tolerance in (-1e-9, float("nan"), float("inf"), "1e-6", True, None):
        with pytest.raises(ValueError, match="tolerance"):
            Probes(X, tolerance=tolerance)
    for kw, what in ((dict(start=0), "start"), (dict(stride=0), "stride"), (dict(stop=-1), "stop"), (dict(start=1.5), "start")):
        with pytest.raises(ValueError, match=what):
            Probes(X, **kw)
    pr = Probes(torch.tensor(X, dtype=torch.float32), graph=0, start=3, stride=2, stop=9, keep=7, tolerance=0)
    assert (pr.start, pr.stride, pr.stop, pr.enabled, pr.keep, pr.tolerance, pr.P) == (3, 2, 9, True, 7, 0.0, 1)
    assert pr.points.dtype == torch.float64
    pr.set_window(stride=4, stop=None, enabled=False)
    assert (pr.start, pr.stride, pr.stop, pr.enabled) == (3, 4, None, False)
    with pytest.raises(ValueError, match="stride"):
        pr.set_window(stride=0)
    # an object that is not attached; an attach that raised leaves it free
    for call in (pr.read, pr.count, pr.raw, pr.reset):
        with pytest.raises(RuntimeError, match=r"this Probes is not attached yet: hand it to Rollout\(..., probes=\)"):
            call()
    xb, clock, owner = torch.zeros(plan.N, 12), torch.zeros(2, dtype=torch.int32), types.SimpleNamespace()
    with pytest.raises(ValueError, match="GPU"):
        pr.attach(owner, graphs, plan, xb, clock, 0)                           # a CPU node state: there is no CPU path
    with pytest.raises(ValueError, match="DevicePool"):
        pr.attach(owner, pooled, plan, xb, clock, 0)
    with pytest.raises(ValueError, match="outside 0 .. 1"):
        Probes(X, graph=2).attach(owner, graphs, plan, xb, clock, 0)
    pr.check_free()
    assert pr.rec is None and pr.tables is None and pr.hist is None and pr._owner is None
    with pytest.raises(ValueError, match="field"):
        PR.sample(graphs, torch.zeros(plan.N, 4), X, 0)
    with pytest.raises(ValueError, match="points"):
        PR.sample(graphs, torch.zeros(plan.N, 3), [[0.0]], 0)
    with pytest.raises((RuntimeError, ValueError), match="GPU"):
        PR.sample(graphs, torch.zeros(plan.N, 3), X, 0)


def test_check_followers_with_five_followers_refuses_in_launch_order():
    import inspect
    from gfv import follow
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.probes import Probes
    from gfv.timescheme import TimeScheme
    from gfv.wallforce import WallForces
    graphs, _, _ = setup("cyl_cavity_b2")
    X = [[1.0, 0.2]]
    assert list(inspect.signature(follow.check_followers).parameters)[-1] == "probes"              # last: every existing call holds
    follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=WallForces(), probes=Probes(X, graph=0),
                           time_bc=T.TimeBC(velocity=T.Const()), time_scheme=TimeScheme())
    follow.check_followers("Rollout", graphs, 2)
    # among several, the launch order decides: field_stats, wall_forces, probes, time_bc, time_scheme
    with pytest.raises(ValueError, match="wall_forces must be"):
        follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=1, probes=2, time_bc=3, time_scheme=4)
    with pytest.raises(ValueError, match="MarchStep: probes must be"):
        follow.check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=WallForces(), probes=2, time_bc=3,
                               time_scheme=4)
    with pytest.raises(ValueError, match="time_bc must be"):
        follow.check_followers("MarchStep", graphs, 0, probes=Probes(X, graph=0), time_bc=3, time_scheme=4)
    with pytest.raises(ValueError, match="anderson > 0 together with probes"):
        follow.check_followers("Rollout", graphs, 1, probes=Probes(X, graph=0), time_bc=3)
    with pytest.raises(ValueError, match="anderson > 0 together with wall_forces"):
        follow.check_followers("Rollout", graphs, 1, wall_forces=WallForces(), probes=Probes(X, graph=0))
    assert "five followers" in follow.__doc__ and "probes, time_bc, time_scheme" in follow.__doc__
