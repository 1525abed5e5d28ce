"""GPU: the forward-only engine path (`Engine.forward(keep=False)`) and `gfv.rollout.Rollout` on top of it.

1. the forward-only forward has the BITS of the training forward (every case, hidden 128 and 64, and once at full size);
2. five rollout steps against five steps of the CPU oracle + write-back, 1e-5 relative (test_model_gpu.TOL);
3. five `Rollout.step()` calls, list mode and eager mode, are bit-equal to five rounds of `with torch.no_grad(): model(*graphs)`
   + the reference's write-back in Python - also after an unrelated training forward + backward of a larger batch went through the
   same engine (who owns the buffers a recorded list points at);
4. the history kernel: losses bit for bit, update norms against float64 to 1e-6, run-to-run bit identity, `run(tol=...)`;
5. nothing is saved: no saved state, and the peak memory of a full-size forward-only step is below the training forward's by at
   least z1 and z2 of every 128-wide MLP;
6. the forward-only instantiation of the Transolver block's row-local chain against its saving form, both tile forms;
7. a narrow model (hidden 64: padded parameters, the library's hidden size set around the launches) as a recorded list.
"""
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5          # tests/test_model_gpu.py
NORM_TOL = 1e-6     # fp32 result of a fixed-order double sum over the graph's nodes against float64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _hip_model(P, dataset_size=100, **kw):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    m = NNmodel(default_params(dataset_size=dataset_size, **kw))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


def _to_gpu(graphs):
    hg = tuple(g.clone().to("cuda") for g in graphs)
    hg[0].norm_uvp, hg[0].norm_global = True, True
    return hg


def _bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.detach().cpu(), b.detach().cpu()))


def _forward_only(model, hg):
    """Engine.forward(keep=False) from the inputs NNmodel.forward would hand it -> (losses, uvp_node, uvp_cell, ea15, saved)."""
    from FVMmodel.padding import pad_parameters
    from gfv.plan import get_plan
    eng = model.engine()
    names, tensors = model.param_names_tensors()
    with torch.no_grad():
        P = dict(zip(names, (t.detach() for t in pad_parameters(names, tensors, model.hidden_size))))
    plan = get_plan(hg)
    acc = model.node_norm.should_accumulate()
    with eng.model_width():
        out = eng.forward(P, model.node_norm.buffers_dict(), hg[0].x, plan, norm_global=True, accumulate=acc, keep=False)
    torch.cuda.synchronize()
    return out


def _check_bit_identity(graphs, P, **kw):
    train, fwd = _hip_model(P, **kw), _hip_model(P, **kw)
    hg_t, hg_f = _to_gpu(graphs), _to_gpu(graphs)
    out = train(*hg_t)                                   # grad-enabled: the saving forward
    assert out[0].requires_grad
    losses, uvp_node, uvp_cell, ea15, saved = _forward_only(fwd, hg_f)
    assert saved is None
    for i in range(4):
        assert _bits(out[i], losses[:, i:i + 1]), f"loss {i}"
    assert _bits(out[4], uvp_node), "uvp_node"
    assert _bits(out[5], uvp_cell), "uvp_cell"
    assert _bits(hg_t[0].x, hg_f[0].x), "graph_node.x"
    assert _bits(hg_t[0].edge_attr, ea15), "edge_attr"
    bt, bf = train.node_norm.buffers_dict(), fwd.node_norm.buffers_dict()
    for k in bt:
        assert _bits(bt[k], bf[k]), f"Normalizer buffer {k}"


@pytest.mark.parametrize("hidden", [128, 64])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_forward_only_has_the_bits_of_the_training_forward(name, hidden):
    hyper = {"hidden_size": hidden}
    P = O.init_parameters(cases.WEIGHT_SEED, hyper)
    _check_bit_identity(cases.make_graphs(name), P, hidden_size=hidden)


@pytest.fixture(scope="module")
def bench_mesh():
    """The 50 020-cell cylinder mesh of the full-size tests (tests/test_fullsize_gpu.py): the persistent / column-owner families."""
    from gfv import meshgen
    from gfv.graph import build_batch
    nx, ny = meshgen.cylinder_grid_for_cells(50000)
    m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234))
    return build_batch([m], [meshgen.random_fields(m, seed=1234 + 7)])


def test_forward_only_has_the_bits_of_the_training_forward_full_size(bench_mesh):
    _check_bit_identity(bench_mesh, O.init_parameters(cases.WEIGHT_SEED))


def test_forward_only_saves_nothing_full_size(bench_mesh):
    """Peak memory of a forward-only step against a grad-enabled forward: lower by at least z1 and z2 ([M,128] fp32 each = 2 x 512 B
    per row) of every 128-wide MLP of simulator_fwd - the two encoders, an EdgeBlock and a NodeBlock MLP per GnBlock, the decoder."""
    P = O.init_parameters(cases.WEIGHT_SEED)
    model = _hip_model(P, dataset_size=1)
    eng = model.engine()
    from gfv.plan import get_plan

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        keep = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del keep
        return p

    hg = _to_gpu(bench_mesh)
    plan = get_plan(hg)
    _forward_only(model, hg)            # (settles the weight-image set and the engine's workspaces: not part of either peak)
    hg = _to_gpu(bench_mesh)
    p_fwd = peak(lambda: _forward_only(model, hg))
    hg = _to_gpu(bench_mesh)
    p_train = peak(lambda: model(*hg))
    n_blocks = eng.n_proc * eng.mp
    n_edge_mlps, n_node_mlps = 1 + n_blocks, 2 + n_blocks
    need = 2 * 512 * (plan.E * n_edge_mlps + plan.N * n_node_mlps)
    print(f"peak forward-only {p_fwd / 2**20:.1f} MiB, training forward {p_train / 2**20:.1f} MiB, required gap {need / 2**20:.1f} MiB")
    assert p_train - p_fwd >= need, (p_train, p_fwd, need)


def _oracle_rollout(graphs, P, steps):
    """`steps` rounds of the oracle's forward + the write-back of solve_without_grad_GPU.py:168-173 on the CPU."""
    buffers = O.new_normalizer_buffers()
    og = tuple(g.clone() for g in graphs)
    backup = og[0].x.clone()
    out = []
    with torch.no_grad():
        for _ in range(steps):
            og[0].x = backup.clone()
            o = O.model_forward(P, buffers, og)
            out.append([t.detach().clone() for t in o[:6]])
            backup = torch.cat((o[4].detach(), backup[:, 3:]), dim=1)
    return out


@pytest.mark.parametrize("name", list(cases.CASES))
def test_five_step_rollout_matches_oracle(name):
    from gfv.rollout import Rollout
    graphs = cases.make_graphs(name)
    P = O.init_parameters(cases.WEIGHT_SEED)
    ref = _oracle_rollout(graphs, P, 5)
    r = Rollout(_hip_model(P), _to_gpu(graphs), max_steps=8)
    got = []
    for _ in range(5):
        losses, uvp_node, uvp_cell = r.step()
        got.append((losses.clone(), uvp_node.clone(), uvp_cell.clone()))
    hist = r.history[:5].cpu()
    worst = 0.0
    for k in range(5):
        for i, key in enumerate(("loss_cont", "loss_mom_x", "loss_mom_y", "loss_press")):
            e = rel(got[k][0][:, i:i + 1], ref[k][i])
            worst = max(worst, e)
            print(f"{name} step {k + 1} {key}: rel {e:.2e}")
            assert e < TOL, (name, k + 1, key, e)
            assert rel(hist[k, :, i:i + 1], ref[k][i]) < TOL
        for j, key in ((1, "uvp_node"), (2, "uvp_cell")):
            e = rel(got[k][j], ref[k][3 + j])
            worst = max(worst, e)
            print(f"{name} step {k + 1} {key}: rel {e:.2e}")
            assert e < TOL, (name, k + 1, key, e)
    print(f"{name}: worst relative error over five steps {worst:.2e}")
    # run() from the same state writes the same history (a fresh model: this one's Normalizer has accumulated five steps)
    again = Rollout(_hip_model(P), _to_gpu(graphs), max_steps=5).run(steps=5)
    assert again.shape == (5, r.plan.B, 6) and torch.equal(again, hist)


def _python_route(model, hg, steps):
    """`with torch.no_grad(): model(*graphs)` + the reference's write-back, in Python."""
    backup = hg[0].x.clone()
    out = []
    for _ in range(steps):
        hg[0].norm_uvp, hg[0].norm_global = True, True
        with torch.no_grad():
            o = model(*hg)
        out.append((torch.cat(o[:4], dim=1).clone(), o[4].clone(), o[5].clone()))
        backup = torch.cat((o[4].detach(), backup[:, 3:]), dim=1)
        hg[0].x = backup.clone()
    return out


def _larger_batch():
    """Four cylinder meshes of ~1 500 cells: more graphs, nodes and edges than any of cases.CASES."""
    from gfv import meshgen
    from gfv.graph import build_batch
    meshes, fields = [], []
    for s in range(4):
        nx, ny = meshgen.cylinder_grid_for_cells(1500 + 100 * s)
        m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=40 + s))
        meshes.append(m)
        fields.append(meshgen.random_fields(m, seed=50 + s))
    return build_batch(meshes, fields)


@pytest.mark.parametrize("name", ["cavity_mixed_b1", "cyl_b3"])
def test_rollout_equals_the_no_grad_route_and_owns_its_buffers(name):
    from gfv.rollout import Rollout
    graphs = cases.make_graphs(name)
    P = O.init_parameters(cases.WEIGHT_SEED)
    model = _hip_model(P, dataset_size=1)     # a trained model: the Normalizer no longer accumulates, nothing below changes it
    ref = _python_route(model, _to_gpu(graphs), 5)
    big = _to_gpu(_larger_batch())
    assert big[0].x.shape[0] > graphs[0].x.shape[0] and int(big[0].batch.max()) + 1 > len(cases.CASES[name])
    for mode in ("cmd_list", "eager"):
        r = Rollout(model, _to_gpu(graphs), max_steps=5, launch_mode=mode)
        for k in range(5):
            if k == 3:
                # an unrelated training forward + backward of another, larger batch through the same model's engine: it rebuilds
                # the engine's per-step weight images, grows its workspaces and allocates ~everything a step can allocate
                assert mode == "eager" or r._lists, "the list should have been recorded by now"
                big[0].norm_uvp, big[0].norm_global = True, True
                x_keep = big[0].x.clone()
                o = model(*big)
                (o[0].sum() + o[1].sum() + o[2].sum() + o[3].sum()).backward()
                model.zero_grad(set_to_none=True)
                big[0].x = x_keep
                torch.cuda.synchronize()
            losses, uvp_node, uvp_cell = r.step()
            assert _bits(losses, ref[k][0]), (mode, k, "losses")
            assert _bits(uvp_node, ref[k][1]), (mode, k, "uvp_node")
            assert _bits(uvp_cell, ref[k][2]), (mode, k, "uvp_cell")
        assert r.steps_done == 5
        with pytest.raises(IndexError):
            r.step()


def _ref_norms(r, prev, new):
    """float64 per-graph ||new - prev||_2 and ||new||_2 from the fp32 fields."""
    b = r.plan.batch.long().cpu()
    B = r.plan.B
    d = (new.double().cpu() - prev.double().cpu()).pow(2).sum(1)
    n = new.double().cpu().pow(2).sum(1)
    dn = torch.zeros(B, dtype=torch.float64).index_add_(0, b, d).sqrt()
    nn = torch.zeros(B, dtype=torch.float64).index_add_(0, b, n).sqrt()
    return dn, nn


@pytest.mark.parametrize("name", ["cyl_cavity_b2", "cyl_b3"])
def test_history_kernel_and_early_stop(name):
    from gfv.rollout import Rollout
    graphs = cases.make_graphs(name)
    P = O.init_parameters(cases.WEIGHT_SEED)
    K = 6
    r = Rollout(_hip_model(P, dataset_size=1), _to_gpu(graphs), max_steps=K)
    for k in range(K):
        prev = r.x_backup[:, 0:3].clone()
        losses, uvp_node, _ = r.step()
        row = r.history[k].cpu()
        assert torch.equal(row[:, 0:4], losses.cpu()), k
        assert torch.equal(r.x_backup[:, 0:3], uvp_node) and torch.equal(r.x, r.x_backup), k
        dn, nn = _ref_norms(r, prev, uvp_node)
        e_d = float(((row[:, 4].double() - dn).abs() / dn).max())
        e_n = float(((row[:, 5].double() - nn).abs() / nn).max())
        print(f"{name} step {k + 1}: update norm rel {e_d:.2e}, field norm rel {e_n:.2e}")
        assert e_d < NORM_TOL and e_n < NORM_TOL, (k, e_d, e_n)
    hist = r.history.cpu().clone()
    assert int(r._state[0]) == K and int(r._state[1]) == 0
    # run to run
    r.reset()
    assert torch.equal(r.run(steps=K), hist)
    # early stop: a tolerance between two recorded values of this very history
    m = (hist[:, :, 4] / hist[:, :, 5]).max(dim=1).values.double()     # worst graph per step
    k_star = 0
    for k in range(1, K):
        if m[k] < m[:k].min():
            k_star = k          # the last step that is a strict record low
    tol = float((m[k_star] + m[:k_star].min()) / 2) if k_star > 0 else float(2 * m[0])
    below = [bool(m[k] < tol) for k in range(K)]
    assert below.index(True) == k_star
    r.reset()
    out = r.run(steps=K, tol=tol, check_every=1)
    assert out.shape[0] == k_star + 1 == r.steps_done, (out.shape, k_star, m.tolist(), tol)
    assert torch.equal(out, hist[:k_star + 1])
    # checks every second step only: the first CHECKED step below the tolerance ends the run
    checked = [k for k in range(K) if (k + 1) % 2 == 0 or k + 1 == K]
    expect = next((k for k in checked if below[k]), K - 1)
    r.reset()
    out = r.run(steps=K, tol=tol, check_every=2)
    assert out.shape[0] == expect + 1, (out.shape, expect, m.tolist(), tol)
    # without a tolerance nothing stops it
    r.reset()
    assert r.run(steps=K, tol=None).shape[0] == K


def test_refresh_weights_is_required_after_a_parameter_change():
    from gfv.rollout import Rollout
    graphs = cases.make_graphs("cavity_mixed_b1")
    P = O.init_parameters(cases.WEIGHT_SEED)
    model = _hip_model(P, dataset_size=1)
    r = Rollout(model, _to_gpu(graphs), max_steps=8)
    for _ in range(3):
        first = [t.clone() for t in r.step()]
    P2 = O.init_parameters(cases.WEIGHT_SEED + 1)
    sd = model.state_dict()
    for k, v in P2.items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        r.step()
    r.refresh_weights()
    r.reset()
    other = Rollout(_hip_model(P2, dataset_size=1), _to_gpu(graphs), max_steps=2, launch_mode="eager")
    a, b = r.step(), other.step()
    for u, v in zip(a, b):
        assert _bits(u, v)
    assert not _bits(a[1], first[1])


@pytest.mark.parametrize("M,small", [(129, 0), (3000, 0), (25479, 0), (33, 1), (3000, 1)])
def test_trans_mlp_forward_only_form_has_the_bits_of_the_saving_form(M, small, gfv_limits):
    """gfv_trans_mlp_fwd with fx1 == z == NULL (csrc/transmlp.hip / csrc/ctrans.hip, SAVE = false) against the saving launch on the
    same rows: `out` bit for bit.  small = 1: the small-tile form, 0: the 128-row-block kernel at every size."""
    from gfv import ops
    gfv_limits(GFV_CTRANS=small)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(M)
    s = lambda *sh: torch.randn(*sh, generator=g)
    P = {"Wout": s(128, 128) * 0.09, "bout": s(128) * 0.1, "gamma": 1 + 0.1 * s(128), "beta": 0.1 * s(128),
         "Wpre": s(256, 128) * 0.09, "bpre": s(256) * 0.1, "Wpost": s(128, 256) * 0.06, "bpost": s(128) * 0.1}
    x = (s(M, 128) * torch.logspace(-2, 1, M)[:, None]).to(dev).contiguous()      # rows over three decades
    res = s(M, 128).to(dev).contiguous()
    wmax = torch.stack([v.abs().max() for k, v in P.items() if k.startswith("W")]).max().reshape(1).to(dev)
    Pd = {k: v.to(dev).contiguous() for k, v in P.items()}
    wi = ops.WeightImages(dev, wmax)
    wi.static = [(0, 1 << 62)]
    prev = ops.set_weight_images(wi)
    try:
        new = lambda *sh: torch.full(sh, float("nan"), device=dev)
        args = (x, res, Pd["Wout"], Pd["bout"], Pd["gamma"], Pd["beta"], Pd["Wpre"], Pd["bpre"], Pd["Wpost"], Pd["bpost"])
        f1, zz, saving = new(M, 128), new(M, 256), new(M, 128)
        assert ops.trans_mlp_fwd(*args, f1, zz, saving)
        only = new(M, 128)
        assert ops.trans_mlp_fwd(*args, None, None, only)
        torch.cuda.synchronize()
    finally:
        ops.set_weight_images(prev)
    assert not bool(torch.isnan(saving).any()) and torch.equal(saving, only)


def test_narrow_model_rollout_list_equals_eager():
    from gfv import lib as L
    from gfv.rollout import Rollout
    graphs = cases.make_graphs("cyl_cavity_b2")
    P = O.init_parameters(cases.WEIGHT_SEED, {"hidden_size": 64})
    ref = _python_route(_hip_model(P, hidden_size=64), _to_gpu(graphs), 5)
    runs = {}
    for mode in ("cmd_list", "eager"):
        r = Rollout(_hip_model(P, hidden_size=64), _to_gpu(graphs), max_steps=5, launch_mode=mode)
        outs = []
        for _ in range(5):
            outs.append([t.clone() for t in r.step()])
        runs[mode] = (outs, r.history.cpu().clone())
        assert L.load().gfv_hidden_size() == 128
    for k in range(5):
        for a, b, c in zip(runs["cmd_list"][0][k], runs["eager"][0][k], ref[k]):
            assert _bits(a, b) and _bits(a, c), k
    assert torch.equal(runs["cmd_list"][1], runs["eager"][1])
