"""GPU: the observation term (gfv/observe.py, csrc/obs.hip; include/gfv.h "Observation term").

1. gfv_obs_fwd alone against tests/obs_ref.py: the chunk workspace and float(W_b) bit for bit, obs_b within one fp32 spacing (the
   bound of tests/test_evaluate_gpu.py: a double quotient rounded once), loss / gloss / gobs / tot within 4 fp32 spacings of the
   float64 reference rounded to fp32 (logf and the fp32 products, as tests/test_balance_gpu.py), counter back at zero, a second
   launch bit-identical;
2. gfv_obs_bwd alone: untouched rows keep their bits, every other element within 2e-6 * (|g_dec0| + |increment|) of float64 - at
   most about eight fp32 roundings (5e-7); with |dec| <= 10 the factor 1 - t^2 is at least 0.42, which amplifies tanhf's last-place
   error less than three times;
3. the whole step against the oracle's autograd of mean log(batch + w_obs * obs): loss 1e-5, every gradient by the criterion of
   tests/test_model_gpu.py;
4. all weights zero = no observations, bit for bit;   5. eager, list and hipGraph agree bit for bit;
6. `.weight` and `set_values` reach recorded steps without a re-recording;   7. the pool path against a plain TrainStep;
8. it fits;   9. refusals that need a device."""
import numpy as np
import pytest
import torch

import cases
import chunk_sums_ref as CS
import obs_ref as R
from oracle import fvgn_oracle as O
from test_march_gpu import _assert_same, _bits, _cpu_graphs, _graphs, _model

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LW = (6e4, 5e4, 1.0)
SPACINGS = 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spacings_apart(got, want):
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), (got, want)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


# ---- the synthetic shape of tests 1 and 2 ------------------------------------------------------------------------------------------
# the three graphs of chunk_sums_ref.ROWS (1, 6 and 70 chunks of 1 .. 100 rows) and a fourth of 4097 rows in chunks of 64: 65 chunks,
# so that a lane of the per-graph fold takes two; 142 chunks (no multiple of the 4 waves of a workgroup); the last chunk's end past N
ROWS = CS.ROWS + [[64] * 64 + [1]]
ZERO_GRAPH = 1


@pytest.fixture(scope="module")
def case():
    """Tables, fields and the reference: computed once, shared by tests 1 and 2, left unchanged."""
    rows = np.array([r for g in ROWS for r in g], dtype=np.int64)
    end = np.cumsum(rows)
    beg = end - rows
    N = int(end[-1])
    end[-1] += CS.OVERHANG
    B = len(ROWS)
    gcp = np.concatenate(([0], np.cumsum([len(g) for g in ROWS]))).astype(np.int32)
    row_graph = np.repeat(np.arange(B), [sum(g) for g in ROWS])
    assert N % 256 != 0 and len(rows) % 4 != 0 and len(ROWS[3]) > 64 and sum(ROWS[3]) == 4097
    rng = np.random.default_rng(20261020)
    spread = lambda shape: (rng.standard_normal(shape) * 10.0 ** rng.uniform(-1.5, 1.5, shape)).astype(f32)
    phi = spread((N, 8))
    target = spread((N, 3))
    weight = (rng.uniform(0.1, 2.0, (N, 3)) * (rng.uniform(0, 1, (N, 3)) > 1.0 / 3.0)).astype(f32)
    weight[row_graph == ZERO_GRAPH] = 0.0
    target[weight == 0] = np.nan
    assert 0.25 < (weight == 0).mean() < 0.45
    c = dict(cb=beg.astype(np.int32), ce=end.astype(np.int32), gcp=gcp, N=N, B=B, nc=len(rows), row_graph=row_graph, phi=phi,
             target=target, weight=weight, uvp_dim=rng.uniform(0.5, 2.0, (B, 3)).astype(f32),
             sigma=rng.uniform(0.5, 2.0, (B, 3)).astype(f32),
             losses=(rng.uniform(1e-5, 1e-3, (B, 4)) * np.array([1.0, 1.0, 1.0, 1e3])).astype(f32),
             dec=rng.uniform(-10.0, 10.0, (N, 3)).astype(f32), node_type=rng.integers(0, 6, N).astype(np.int32),
             g_dec0=spread((N, 3)) * f32(1e-4), w_obs=f32(2.5e3))     # (the size of the increments: both terms of the bound count)
    c["node_type"][40:46] = np.arange(6)
    hyper = np.zeros(8, dtype=f32)
    hyper[5:8] = LW
    c["hyper"] = hyper
    e, _ = R.misfit(phi[:, 0:3], target, weight, c["uvp_dim"], c["sigma"], row_graph)
    c["e"] = e
    c["partial"], c["SW"] = R.sums(R.row_terms(e, weight), c["cb"], c["ce"], gcp, N)
    c["rec"] = R.record(c["SW"], c["losses"], LW, c["w_obs"])
    return c


def _fwd(c):
    from gfv import lib as L
    t = {k: _dev(c[k]) for k in ("phi", "target", "weight", "cb", "ce", "gcp", "uvp_dim", "sigma", "losses", "hyper")}
    w = torch.full((4,), float(c["w_obs"]), dtype=torch.float32, device="cuda")
    partial = torch.full((c["nc"], 2), -1.0, dtype=torch.float64, device="cuda")
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    rec = torch.full((c["B"], 4), -3.0, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), -3.0, dtype=torch.float32, device="cuda")
    gloss = torch.full((c["B"], 4), -3.0, dtype=torch.float32, device="cuda")
    L.check(L.load().gfv_obs_fwd(t["phi"].data_ptr(), t["target"].data_ptr(), t["weight"].data_ptr(), c["N"], t["cb"].data_ptr(),
                                 t["ce"].data_ptr(), t["gcp"].data_ptr(), c["nc"], c["B"], t["uvp_dim"].data_ptr(),
                                 t["sigma"].data_ptr(), t["losses"].data_ptr(), t["hyper"].data_ptr(), w.data_ptr(),
                                 partial.data_ptr(), counter.data_ptr(), rec.data_ptr(), loss.data_ptr(), gloss.data_ptr(),
                                 L.stream_ptr()), "gfv_obs_fwd")
    torch.cuda.synchronize()
    return dict(partial=partial.cpu().numpy(), counter=counter.tolist(), rec=rec.cpu().numpy(), loss=loss.cpu().numpy(),
                gloss=gloss.cpu().numpy(), rec_dev=rec, t=t)


def test_forward_kernel_alone(case):
    c, ref = case, case["rec"]
    o = _fwd(c)
    assert o["counter"] == [0, 0, 0, 0]
    assert o["partial"].tobytes() == c["partial"].tobytes()                      # the chunk workspace, bit for bit
    rec = o["rec"]
    assert rec[:, 1].tobytes() == c["SW"][:, 1].astype(f32).tobytes()            # float(W_b): the fold's order, bit for bit
    assert ref["W"][ZERO_GRAPH] == 0 and rec[ZERO_GRAPH, 0] == 0.0 and (ref["obs"][np.arange(c["B"]) != ZERO_GRAPH] > 0).all()
    d_obs = _spacings_apart(rec[:, 0], ref["obs"])
    d_tot, d_gobs = _spacings_apart(rec[:, 3], ref["tot"]), _spacings_apart(rec[:, 2], ref["gobs"])
    d_gloss, d_loss = _spacings_apart(o["gloss"], ref["gloss"]), _spacings_apart(o["loss"], [ref["loss"]])
    print(f"obs_fwd: fp32 spacings from the reference - obs {d_obs.max()}, tot {d_tot.max()}, gobs {d_gobs.max()}, "
          f"gloss {d_gloss.max()}, loss {d_loss.max()}")
    assert d_obs.max() <= 1
    assert max(d_tot.max(), d_gobs.max(), d_gloss.max(), d_loss.max()) <= SPACINGS
    assert np.isfinite(rec).all() and np.isfinite(o["gloss"]).all() and np.isfinite(o["loss"]).all()
    again = _fwd(c)
    for k in ("partial", "rec", "loss", "gloss"):
        assert o[k].tobytes() == again[k].tobytes(), k
    assert again["counter"] == o["counter"]


def test_backward_kernel_alone(case):
    from gfv import lib as L
    c = case
    o = _fwd(c)
    t = o["t"]
    dec, batch, nt = _dev(c["dec"]), _dev(c["row_graph"].astype(np.int32)), _dev(c["node_type"])
    g = _dev(c["g_dec0"])
    L.check(L.load().gfv_obs_bwd(o["rec_dev"].data_ptr(), dec.data_ptr(), t["phi"].data_ptr(), t["target"].data_ptr(),
                                 t["weight"].data_ptr(), batch.data_ptr(), nt.data_ptr(), t["uvp_dim"].data_ptr(),
                                 t["sigma"].data_ptr(), c["N"], c["B"], g.data_ptr(), L.stream_ptr()), "gfv_obs_bwd")
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    inc, contributes = R.gdec_increment(c["rec"], c["e"], c["weight"], c["dec"], c["uvp_dim"], c["sigma"], c["row_graph"],
                                        c["node_type"])
    assert set(c["node_type"].tolist()) == set(range(6))
    rows_off = ~contributes.any(axis=1)
    assert rows_off.sum() > c["N"] // 10 and contributes.sum() > c["N"] // 2 and (~contributes[~rows_off]).any()
    assert got[rows_off].tobytes() == c["g_dec0"][rows_off].tobytes()            # not written at all
    assert got[~contributes].tobytes() == c["g_dec0"][~contributes].tobytes()
    want = c["g_dec0"].astype(f64) + inc
    bound = 2e-6 * (np.abs(c["g_dec0"].astype(f64)) + np.abs(inc))
    err = np.abs(got.astype(f64) - want)
    ratio = float((err[contributes] / bound[contributes]).max())
    print(f"obs_bwd: worst error / bound = {ratio:.3f} (bound 2e-6 * (|g_dec0| + |increment|)) over {int(contributes.sum())} elements")
    assert (err[contributes] <= bound[contributes]).all(), ratio
    assert np.abs(inc[contributes]).min() > 0 and not np.array_equal(got[contributes], c["g_dec0"][contributes])


# ---- 3. the whole step against the oracle ----------------------------------------------------------------------------------------------
def _oracle_with_term(graphs, P, target, weight, w_obs, hyper):
    """loss = mean log(batch + w_obs * obs) on the CPU, obs from the oracle's own uvp_new -> loss, obs [B], gradients by name."""
    Pg = {k: v.detach().requires_grad_(True) for k, v in P.items()}
    og = tuple(g.clone() for g in graphs)
    out, inter = O.model_forward(Pg, O.new_normalizer_buffers(), og, hyper, return_intermediates=True)
    obs, batch, pred = _oracle_obs(out, inter, og, target, weight)
    loss = torch.mean(torch.log(batch + w_obs * obs))
    names = list(Pg)
    grads = dict(zip(names, torch.autograd.grad(loss, [Pg[k] for k in names], allow_unused=True)))
    return float(loss.detach()), obs.detach(), grads


def _oracle_obs(out, inter, og, target, weight):
    G = O.graph_tensors(*og)
    nb, B = G["node_batch"], G["num_graphs"]
    pred = inter["uvp_new"] * G["uvp_dim"][nb] * G["sigma"][nb]
    hp = O.DEFAULT_HYPER
    batch = (hp["loss_press"] * out[3] + hp["loss_cont"] * out[0] + hp["loss_mom"] * out[1] + hp["loss_mom"] * out[2]).reshape(-1)
    if target is None:
        return None, batch, pred
    sq = torch.where(weight != 0, weight * (pred - torch.nan_to_num(target)) ** 2, torch.zeros(()))
    S = torch.zeros(B).index_add(0, nb, sq.sum(1))
    W = torch.zeros(B).index_add(0, nb, weight.sum(1))
    return torch.where(W > 0, S / torch.where(W > 0, W, torch.ones(())), torch.zeros(())), batch, pred


@pytest.mark.parametrize("name", ["cyl_cavity_b2", "cyl_b3", "poly"])
def test_whole_step_against_the_oracle(name):
    from gfv.observe import Observations
    from gfv.trainer import TrainStep
    graphs = _cpu_graphs(name)
    hyper = {"dataset_size": 1}
    P = O.init_parameters(cases.WEIGHT_SEED)
    with torch.no_grad():
        og = tuple(g.clone() for g in graphs)
        out, inter = O.model_forward(P, O.new_normalizer_buffers(), og, hyper, return_intermediates=True)
        _, batch, pred = _oracle_obs(out, inter, og, None, None)
    nb = graphs[0].batch
    B, N = int(batch.numel()), pred.shape[0]
    gen = torch.Generator().manual_seed(5)
    # targets: the oracle's own dimensional prediction plus 5 % noise; about half of the nodes observed, one graph not at all
    scale = pred.abs().amax(0, keepdim=True)
    target = (pred + 0.05 * scale * torch.randn(pred.shape, generator=gen)).float()
    seen = (torch.rand(N, generator=gen) < 0.5)
    if B > 1:
        seen &= nb != 0
    weight = (seen[:, None] * torch.empty(N, 3).uniform_(0.5, 1.5, generator=gen)).float()
    target[weight == 0] = float("nan")
    obs0 = _oracle_obs(out, inter, og, target, weight)[0]
    w_obs = float(f32(float(batch.mean() / obs0[obs0 > 0].mean())))      # the data term weighs about what the residual does
    oloss, oobs, ograds = _oracle_with_term(graphs, P, target, weight, w_obs, hyper)
    obs = Observations(target.cuda(), weight.cuda(), weight=w_obs)
    ts = TrainStep(_model(), _graphs(name), lr=5e-5, observations=obs)
    ts.step()
    torch.cuda.synchronize()
    rec = obs.read()
    assert rec.shape == (B, 4) and (B == 1 or float(rec[0, 0]) == 0.0)
    # (obs itself: the fields agree to 1e-5 of their maximum, the misfit is 5 % of it - up to 2e-4 per element, less in the mean)
    d_obs = float((rec[:, 0].double() - oobs.double()).abs().max()) / float(oobs.abs().max())
    assert d_obs < 2e-4, d_obs
    err = abs(float(ts.loss) - oloss) / abs(oloss)
    plain = float(torch.mean(torch.log(batch)))
    assert abs(plain - oloss) > 1e-3 * abs(oloss), "the data term does not show in the loss: nothing is tested"
    assert err < 1e-5, (float(ts.loss), oloss)
    assert ts.losses.shape == (B, 4)                                      # (still the four residuals)
    gscale = max(float(g.abs().max()) for g in ograds.values() if g is not None)
    worst = 0.0
    for k, g in ograds.items():
        if g is None:
            continue
        mine = ts.G.view(k)
        e = float((mine.cpu().double() - g.double()).abs().max())
        bound = 1e-4 * float(g.abs().max()) + 1e-6 * gscale
        worst = max(worst, e / bound)
        assert e < bound, (k, e, bound)
    print(f"{name}: loss rel err {err:.2e}, worst gradient error / bound {worst:.3f}, w_obs {w_obs:.4g}")


# ---- 4 - 6. the step object ---------------------------------------------------------------------------------------------------------------
def _state(ts):
    torch.cuda.synchronize()
    out = {"named": torch.cat([t.reshape(-1) for pmv in ts.named_state().values() for t in pmv]).cpu(),
           "adam_t": ts.adam_state[0:1].cpu().clone(), "loss": ts.loss.cpu().clone()}
    if ts.observations is not None:
        out["rec"] = ts.observations.rec.cpu().clone()
    return out


def _field(graphs, seed, frac=0.5):
    """Observed values near the initial state and weights with about `frac` of the nodes observed, on the device."""
    x = graphs[0].x
    gen = torch.Generator().manual_seed(seed)
    n = x.shape[0]
    values = (x[:, 0:3].cpu() * (1.0 + 0.1 * torch.randn(n, 3, generator=gen))).float()
    weights = ((torch.rand(n, 1, generator=gen) < frac) * torch.empty(n, 3).uniform_(0.5, 1.5, generator=gen)).float()
    return values.cuda(), weights.cuda()


def test_zero_weights_equal_no_observations():
    from gfv.observe import Observations
    from gfv.trainer import TrainStep
    graphs = _graphs("cyl_cavity_b2")
    values, weights = _field(graphs, 1)
    a = TrainStep(_model(), graphs, lr=5e-5, observations=Observations(values, torch.zeros_like(weights), weight=1e4))
    b = TrainStep(_model(), _graphs("cyl_cavity_b2"), lr=5e-5)
    for k in range(3):
        a.step()
        b.step()
        sa, sb = _state(a), _state(b)
        rec = sa.pop("rec")
        _assert_same(sa, sb, f"step {k}")
        assert (rec[:, 0:2] == 0).all()


W_OBS = 1e6


def _run_modes(mode, changes=False):
    from gfv.observe import Observations
    from gfv.trainer import TrainStep
    graphs = _graphs("poly")
    values, weights = _field(graphs, 2)
    obs = Observations(values, weights, weight=W_OBS)
    ts = TrainStep(_model(), graphs, lr=5e-5, use_graph=mode, observations=obs)
    # (dataset_size 1: the first step accumulates the Normalizer and has a key of its own; of the steady key, steps 1 and 2 warm
    # up, step 3 records the list - the hipGraph mode captures on a key's first step - steps 4 and 5 replay)
    for _ in range(4):
        ts.step()
    kept = ts._lists if mode == "list" else ts._captures       # (command lists; hipGraph captures)
    recorded = None if not mode else dict(kept)
    if changes:
        obs.weight = 3e5
        obs.set_values(values * 1.05)
    ts.step()
    if changes:
        obs.set_weights(weights * 0.5)
    ts.step()
    if recorded is not None:
        assert len(recorded) >= 1 and kept.keys() == recorded.keys()
        assert all(kept[k] is recorded[k] for k in recorded)      # replayed, never re-recorded
        if mode == "list":
            assert all(kept[k].cl is recorded[k].cl and len(kept[k].cl) == len(recorded[k].cl) for k in recorded)
            assert ts.stats()["recorded"] == len(recorded)
    return _state(ts)


def test_launch_modes_are_bit_identical():
    eager = _run_modes(False)
    assert float(eager["rec"][0, 0]) > 0
    _assert_same(_run_modes("list"), eager, "list against eager")
    _assert_same(_run_modes(True), eager, "hipGraph against eager")


def test_device_resident_controls_reach_recorded_steps():
    eager = _run_modes(False, changes=True)
    assert not torch.equal(_bits(eager["named"]), _bits(_run_modes(False)["named"]))   # the changes do change the run
    _assert_same(_run_modes("list", changes=True), eager, "list against eager")
    _assert_same(_run_modes(True, changes=True), eager, "hipGraph against eager")


def test_the_list_of_a_step_without_observations_is_two_launches_shorter():
    """With observations=None the launch sequence is what it was: the recorded list of a step with observations has exactly the
    two launches of the term more."""
    from gfv.observe import Observations
    from gfv.trainer import TrainStep
    counts = []
    for with_obs in (False, True):
        graphs = _graphs("poly")
        obs = Observations(*_field(graphs, 2), weight=W_OBS) if with_obs else None
        ts = TrainStep(_model(), graphs, lr=5e-5, use_graph="list", observations=obs)
        for _ in range(4):                     # (one accumulating step, two warm-ups, the recording)
            ts.step()
        (entry,) = ts._lists.values()
        counts.append(len(entry.cl))
    print("recorded commands per step without / with observations:", counts)
    assert counts[1] == counts[0] + 2


# ---- 7. the pool path ---------------------------------------------------------------------------------------------------------------------
def test_pool_steps_equal_a_plain_trainstep_over_the_same_batch():
    """Entries 0 (a cylinder channel, observed) and 2 (a cavity, not observed) as [0, 2], [2, 0], [0, 2], repeated until both
    ordered signatures replay their list; after clear(0) the next step is a step without observations."""
    from gfv.observe import Observations, PoolObservations
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    from test_pool_train_gpu import _model as pool_model
    from test_pool_train_gpu import _three_size_pool
    seq = [[0, 2], [2, 0], [0, 2]] * 4
    pool = _three_size_pool()
    assert pool.sizes[0]["n"] != pool.sizes[2]["n"]
    n0 = int(pool.sizes[0]["n"])
    gen = torch.Generator().manual_seed(3)
    v0 = torch.randn(n0, 3, generator=gen).cuda()
    w0 = ((torch.rand(n0, 1, generator=gen) < 0.5) * torch.empty(n0, 3).uniform_(0.5, 1.5, generator=gen)).float().cuda()
    pobs = PoolObservations(pool, weight=1e5)
    pobs.set(0, v0, w0)
    ts = PoolTrainStep(pool_model(), pool, max_graphs=2, lr=1e-3, use_graph="list", observations=pobs)
    got = []
    for idx in seq:
        ts.step(idx)
        got.append(dict(_state(ts), rec=pobs.read()))
    assert ts.stats()["lists"] == 2 and ts.stats()["replayed"] >= 5, ts.stats()
    pobs.clear(0)
    ts.step([0, 2])
    last = _state(ts)
    assert (last.pop("rec")[:, 0:2] == 0).all()
    assert pobs.read().shape == (2, 4)
    ts.step([2])                                                         # (a batch of one graph: the record read back follows)
    assert pobs.read().shape == (1, 4) and ts.gloss.shape == (1, 4)

    # the reference: ONE eager TrainStep; per step the batch assembled by pool.batch and Observations over exactly its nodes (the
    # attachment is renewed by hand: set_batch refuses while observations are attached)
    ref_pool = _three_size_pool()
    ref = None
    for k, idx in enumerate(seq + [[0, 2]]):
        g, _ = ref_pool.batch(idx)
        if ref is None:
            ref = TrainStep(pool_model(), g, lr=1e-3, use_graph=False)
        else:
            ref.observations = None
            ref.set_batch(g)
        if k < len(seq):
            vals = torch.cat([v0 if i == 0 else torch.zeros(int(ref_pool.sizes[i]["n"]), 3, device="cuda") for i in idx])
            wts = torch.cat([w0 if i == 0 else torch.zeros(int(ref_pool.sizes[i]["n"]), 3, device="cuda") for i in idx])
            obs = Observations(vals, wts, weight=1e5)
            obs._attach(ref)
            ref.observations = obs
        ref.step()
        want = _state(ref)
        if k < len(seq):
            want["rec"] = obs.read()
            assert float(want["rec"][idx.index(0), 0]) > 0 and float(want["rec"][idx.index(2), 0]) == 0.0
            _assert_same(got[k], want, f"step {k} {idx}")
        else:
            _assert_same(last, want, "the step after clear(0)")


# ---- 8. it fits -------------------------------------------------------------------------------------------------------------------------------
FIT_STEPS, FIT_LR = 6, 1e-4


def test_it_fits():
    """Small polygon mesh, every node and channel observed with weight 1, targets = the initial state's (u, v, p), w_obs = 1e6 (the
    data term is then about 0.6 of the residual part, 1.1e4 against 1.7e4), Adam at lr 1e-4, dataset_size 1.  The ORACLE's loop (its
    train_step extended by the term, on the CPU) gives obs = 1.0964e-2, 1.0224e-2, 9.4979e-3, 8.7882e-3, 8.0842e-3, 7.3609e-3 over six
    steps: every step below the one before, the sixth 0.671 of the first - the HIP path is 1e-5 from the oracle."""
    from gfv.observe import Observations
    from gfv.trainer import TrainStep
    graphs = _graphs("poly")
    target = graphs[0].x[:, 0:3].clone()
    obs = Observations(target, torch.ones_like(target), weight=W_OBS)
    ts = TrainStep(_model(), graphs, lr=FIT_LR, use_graph="list", observations=obs)
    hist = []
    for _ in range(FIT_STEPS):
        ts.step()
        hist.append(obs.read()[:, 0].clone())
    hist = torch.stack(hist)
    print("obs per step:", [f"{float(v):.4e}" for v in hist[:, 0]], "ratio", float(hist[-1, 0] / hist[0, 0]))
    assert bool((hist[-1] < hist[0]).all())
    assert abs(float(hist[0, 0]) - 1.096354e-2) < 1e-4 * 1.096354e-2     # (the first value is the oracle's)


# ---- 9. refusals that need a device ----------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from gfv.balance import Inverse
    from gfv.march import MarchStep
    from gfv.observe import Observations, PoolObservations
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    from test_pool_train_gpu import _three_size_pool
    graphs = _graphs("poly")
    n = graphs[0].x.shape[0]
    values, weights = _field(graphs, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        Observations(values.cpu(), weights.cpu())
    model = _model()
    obs = Observations(values, weights)
    ts = TrainStep(model, graphs, lr=5e-5, observations=obs)
    with pytest.raises(ValueError, match="set_batch"):
        ts.set_batch(_graphs("poly"))
    assert "gfv_observations" not in ts.state_dict() and not any("obs" in k for k in ts.state_dict())
    with pytest.raises(ValueError, match="already attached"):
        TrainStep(model, graphs, lr=5e-5, observations=obs)
    with pytest.raises(ValueError, match="rows"):
        TrainStep(model, graphs, lr=5e-5, observations=Observations(values[:-1], weights[:-1]))
    with pytest.raises(ValueError, match="balance= together"):
        TrainStep(model, graphs, lr=5e-5, balance=Inverse(), observations=Observations(values, weights))
    with pytest.raises(ValueError, match="observations= is not supported"):
        MarchStep(model, graphs, lr=5e-5, observations=Observations(values, weights))
    with pytest.raises(ValueError, match="rows"):
        obs.set_values(values[:-1])
    with pytest.raises(ValueError, match="finite and >= 0"):
        obs.set_weights(-weights - 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        obs.set_values(values.cpu())
    pool, other = _three_size_pool(), _three_size_pool()
    pobs = PoolObservations(pool)
    n0 = int(pool.sizes[0]["n"])
    with pytest.raises(ValueError, match="rows"):
        pobs.set(0, torch.zeros(n0 + 1, 3, device="cuda"), torch.ones(n0 + 1, 3, device="cuda"))
    with pytest.raises(ValueError, match="does not exist"):
        pobs.set(pool.n, torch.zeros(n0, 3, device="cuda"), torch.ones(n0, 3, device="cuda"))
    with pytest.raises(ValueError, match="another pool"):
        PoolTrainStep(model, other, max_graphs=2, observations=pobs)
    with pytest.raises(TypeError):
        PoolTrainStep(model, pool, max_graphs=2, observations=Observations(values, weights))
    with pytest.raises(TypeError):
        TrainStep(model, graphs, lr=5e-5, observations=pobs)
    assert n == values.shape[0]
