"""CPU: the float64 restatement of the finite-volume section (tests/fvm_float64.py) is itself checked before the GPU tests lean
on it - against the float32 oracle and the reference's committed golden outputs at the fixtures' own coefficients, for its power
to tell a mis-wired coefficient from a right one at `distinct_coefficients`, and for the mesh features the GPU tests count on."""
import os

import numpy as np
import pytest
import torch

import cases
import fvm_float64 as F
from oracle import fvgn_oracle as O

TOL, TOL_GRAD = 1e-5, 1e-4      # the suite's bars for the float32 oracle (tests/test_oracle_golden.py), here per column
MESHES = ("cyl_b3", "cyl_cavity_b2")


def _worst(err):
    return max(float(v.max()) for v in err.values())


@pytest.mark.parametrize("order", ["1st", "2nd"])
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
@pytest.mark.parametrize("mesh", MESHES)
def test_float64_reference_agrees_with_the_float32_oracle(mesh, conserved, order):
    """At the fixtures' own coefficients: every column of every stage and every one-hot gradient, float32 against float64 of the
    same statements, within the float32 oracle's rounding; the losses consistent with the sums they are the roots of."""
    graphs = cases.make_graphs(mesh, order=order)
    dec, uvo = F.draw_dec(graphs[0].x.shape[0], 11), F.uv_old_of(graphs)
    G64, G32 = F.graph_tensors(graphs), F.graph_tensors(graphs, torch.float32)
    ref = F.detached(F.stages(dec.double(), uvo.double(), G64, conserved, "imex", order))
    err = F.column_errors(F.detached(F.stages(dec, uvo, G32, conserved, "imex", order)), ref, G64)
    assert set(err) == set(ref)
    gref = F.one_hot_gradients(dec.double(), uvo.double(), G64, conserved, "imex", order)
    gerr = F.gradient_errors(F.one_hot_gradients(dec, uvo, G32, conserved, "imex", order), gref, G64)
    print(f"{mesh} {order} conserved={conserved}: stages {_worst(err):.1e}, one-hot gradients {_worst(gerr):.1e}")
    assert _worst(err) < TOL, F.family_max(err)
    assert _worst(gerr) < TOL_GRAD, F.family_max(gerr)
    sums, losses = F.graph_norms(ref["cres"].float(), torch.cat((torch.zeros(1, dtype=torch.long),
                                                                  torch.bincount(G64["cell_batch"]).cumsum(0))),
                                 G64["theta_PDE"], G64["sigma"])
    assert float((sums - ref["sums"]).abs().max()) <= 1e-6 * float(ref["sums"].abs().max())      # (cres rounded to float32 here)
    assert float((losses - ref["losses"]).abs().max()) <= 1e-6 * float(ref["losses"].abs().max())


@pytest.mark.parametrize("name,mesh,conserved", [("cyl_b3", "cyl_b3", True), ("cyl_cavity_b2", "cyl_cavity_b2", True),
                                                 ("nc_cyl_cavity_b2", "cyl_cavity_b2", False)])
def test_float64_reference_reproduces_the_golden_outputs(name, mesh, conserved, golden_dir):
    """From the decoder output the reference itself produced to its four losses and two fields (tests/golden/make_golden.py), per
    column and per graph."""
    fx = np.load(os.path.join(golden_dir, f"{name}.npz"))
    if "dec" not in fx.files:
        # (the fixture of the non-conserved form keeps no decoder output: the oracle's, pinned to it by test_oracle_golden.py)
        out, inter = O.model_forward(O.init_parameters(cases.WEIGHT_SEED), O.new_normalizer_buffers(), cases.make_graphs(mesh),
                                     hyper={"conserved_form": conserved}, return_intermediates=True)
        dec = inter["dec"].detach()
    else:
        dec = torch.from_numpy(fx["dec"])
    graphs = cases.make_graphs(mesh)
    G64 = F.graph_tensors(graphs)
    ref = F.detached(F.stages(dec.double(), F.uv_old_of(graphs).double(), G64, conserved, "imex", "2nd"))
    gold = dict(losses=torch.from_numpy(np.concatenate([fx[k].reshape(-1, 1) for k in ("loss_cont", "loss_mom_x", "loss_mom_y",
                                                                                       "loss_press")], axis=1)),
                uvp_node=torch.from_numpy(fx["uvp_node"]), uvp_cell=torch.from_numpy(fx["uvp_cell"]))
    err = F.column_errors(gold, ref, G64)
    assert set(err) == {"losses", "uvp_node", "uvp_cell"}
    print(name, F.family_max(err))
    assert _worst(err) < TOL, F.family_max(err)


@pytest.mark.parametrize("order", ["1st", "2nd"])
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
@pytest.mark.parametrize("mesh", MESHES)
def test_distinct_coefficients_expose_every_wiring_mistake(mesh, conserved, order):
    """The GPU tests' cases: each mis-wired variant of the reference moves at least one compared column by more than 100 x that
    column's tolerance there (4 x the float32 oracle's error, floor 2^-22)."""
    base = cases.make_graphs(mesh, order=order)
    graphs = F.distinct_coefficients(base, 7)
    gi = graphs[4]
    B = gi.theta_PDE.shape[0]
    for t in (gi.theta_PDE[:, 0:6], gi.sigma, gi.uvp_dim, gi.dt_graph):
        assert t.unique().numel() == t.numel() and bool((t != 0).all())
    fac = gi.theta_PDE[:, 0:5] / base[4].theta_PDE[:, 0:5]
    assert float(fac.min()) >= 0.5 and float(fac.max()) <= 2.0
    assert torch.equal(base[4].theta_PDE[:, 0:4], torch.ones(B, 4))                    # (what made the mistakes invisible)
    dec, uvo = F.draw_dec(graphs[0].x.shape[0], 11), F.uv_old_of(graphs)
    G64, G32 = F.graph_tensors(graphs), F.graph_tensors(graphs, torch.float32)
    ref = F.detached(F.stages(dec.double(), uvo.double(), G64, conserved, "imex", order))
    tol = F.tolerance(F.column_errors(F.detached(F.stages(dec, uvo, G32, conserved, "imex", order)), ref, G64))
    # the source is of the size of the momentum residual per unit area
    per_area = float((ref["cres"][:, 1:3].abs() / G64["cells_area"].view(-1, 1)).median())
    assert 20.0 <= per_area <= 70.0 and 10.0 <= float(gi.theta_PDE[:, 5].abs().min()) and float(gi.theta_PDE[:, 5].abs().max()) <= 40.0
    for name, miswire in F.MISWIRED.items():
        wrong = F.detached(F.stages(dec.double(), uvo.double(), miswire(G64), conserved, "imex", order))
        err = F.column_errors(wrong, ref, G64)
        moved = max(float((err[k] / tol[k]).max()) for k in err)
        assert moved > 100.0, (name, moved)
    # dt: every graph but the one whose dt was handed out sees it
    err = F.column_errors(F.detached(F.stages(dec.double(), uvo.double(), F.MISWIRED["dt of graph 0 for all"](G64), conserved,
                                              "imex", order)), ref, G64)
    assert bool(((err["cres"][1:, 1:3] / tol["cres"][1:, 1:3]) > 100.0).all())


@pytest.mark.parametrize("integrator", F.MODES)
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
@pytest.mark.parametrize("mesh", MESHES)
def test_one_hot_gradients_reach_every_channel(mesh, conserved, integrator):
    """Each loss of each graph on its own has a non-zero gradient in every dec channel the mathematics allows: the continuity
    loss does not see the pressure, with the explicit integrator a momentum loss does not see the other velocity component, the
    outlet loss of a graph without an outlet sees nothing (and is left out)."""
    graphs = F.distinct_coefficients(cases.make_graphs(mesh), 7)
    G64 = F.graph_tensors(graphs)
    dec, uvo = F.draw_dec(graphs[0].x.shape[0], 11), F.uv_old_of(graphs)
    grads = F.one_hot_gradients(dec.double(), uvo.double(), G64, conserved, integrator, "2nd")
    outflow = F.has_outflow(G64)
    B = G64["num_graphs"]
    assert set(grads) == {(b, l) for b in range(B) for l in range(4) if l < 3 or bool(outflow[b])}
    assert bool(outflow[0]) and (mesh != "cyl_cavity_b2" or not bool(outflow[1]))
    for (b, l), g in grads.items():
        mine = G64["node_batch"] == b
        assert bool((g[~mine] == 0).all())
        top = g[mine].abs().amax(0)
        allowed = [True, True, l != 0]                 # continuity: no pressure
        if integrator == "explicit" and l in (1, 2):   # uv_hat = uv_old: the x-momentum sees u (unsteady term) and p only
            allowed[2 - l] = False
        assert [float(t) > 0.0 for t in top] == allowed, (b, l, top)


def test_fixtures_cover_what_the_gpu_tests_count_on():
    """Asserted, so that a later change of a fixture cannot silently take it away."""
    g3, g2 = cases.make_graphs("cyl_b3"), cases.make_graphs("cyl_cavity_b2")
    N = g3[0].x.shape[0]
    assert (N, g3[3].pos.shape[0], g3[4].theta_PDE.shape[0]) == (708, 1108, 3)
    assert (g2[0].x.shape[0], torch.bincount(g2[3].batch).tolist()) == (453, [624, 36])
    # stencil row lengths: all four residues mod 4 in both CSR directions (the 4-way unrolled loops of wlsq_fwd_kernel,
    # wlsq_bwd_gather_kernel and wlsq_gather_phi_bwd_kernel)
    out_idx, in_idx = O.wlsq_stencil(g3[1].face_node_x, g3[1].support_edge)
    for idx in (in_idx, out_idx):
        residues = torch.bincount(torch.bincount(idx, minlength=N) % 4, minlength=4)
        print("stencil rows by length mod 4:", residues.tolist())
        assert bool((residues > 0).all()), residues
    assert set(g3[0].node_type.reshape(-1).tolist()) == {0, 1, 2, 3, 5}
    assert 4 in set(g2[0].node_type.reshape(-1).tolist())
    for g in (g3, g2):
        assert set(g[2].face_type.reshape(-1).tolist()) == {0, 1, 2, 3}
    for g in (g3, g2):
        assert {3, 4} <= set(torch.bincount(g[3].face).tolist())       # 3-node and 4-node cells
