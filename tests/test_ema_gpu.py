"""Averaged weights on the GPU (include/gfv.h gfv_ema_init / gfv_adam_step_ema_dev, gfv/ema.py).  The kernel alone
on random vectors - the average against a float64 recurrence fed the kernel's own parameters and weights, the Adam arithmetic
bit for bit that of the three existing entry points, steps that are not applied leaving no trace - and through `TrainStep` and
`PoolTrainStep`: the three launch modes, accumulation and the guard, the swap for evaluation, the checkpoint."""
import struct

import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CLIP, SKIP_NONFINITE = 1, 2


# ---- the C ABI on flat buffers ---------------------------------------------------------------------------------------------
def _lib():
    from gfv import lib as L
    return L, L.load()


def _hyper(lr=1e-2):
    return torch.tensor([lr, 0.9, 0.999, 1e-8, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _int_record(words):
    rec = torch.zeros(8, dtype=torch.int32)
    for k, w in words.items():
        rec[k] = w
    return rec.cuda().view(torch.float32)


def _guard_record(coef, decision):
    return _int_record({3: struct.unpack("i", struct.pack("f", coef))[0], 4: decision})


def _accum_record(apply):
    return _int_record({0: 2, 3: apply})


def _ema_record(decay, warmup, updates=0):
    L, lib = _lib()
    rec = torch.full((8,), float("nan"), device="cuda")       # (the launch writes all eight words)
    L.check(lib.gfv_ema_init(rec.data_ptr(), decay, int(warmup), updates, L.stream_ptr()), "ema_init")
    return rec


def _read_ema(rec):
    torch.cuda.synchronize()
    f = rec.detach().cpu().clone()
    i = f.view(torch.int32)
    return dict(decay=float(f[0]), warmup=int(i[1]), updates=int(i[2]), w=float(f[3]), rest=[int(x) for x in i[4:]])


class _Flat:
    """p, m, v, state and average of one Adam run over n slots; `twin()` is a bit copy."""

    def __init__(self, n, seed=3):
        L, lib = _lib()
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, generator=gen).cuda()
        self.e = (self.p.cpu() + 0.25 * torch.randn(n, generator=gen)).cuda()
        self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.state = torch.zeros(16, device="cuda")
        L.check(lib.gfv_adam_state_init(self.state.data_ptr(), 0.9, 0.999, 0.0, L.stream_ptr()), "state_init")

    def twin(self):
        t = object.__new__(_Flat)
        t.n = self.n
        for name in ("p", "e", "m", "v", "state"):
            setattr(t, name, getattr(self, name).clone())
        return t

    def bits(self):
        torch.cuda.synchronize()
        return [t.detach().cpu().view(torch.int32).clone() for t in (self.p, self.m, self.v, self.state)]

    def ema_step(self, g, hyper, rec, guard=None, accum=None):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_ema_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.e.data_ptr(),
                                          self.n, self.state.data_ptr(), hyper.data_ptr(), None if guard is None else guard.data_ptr(),
                                          None if accum is None else accum.data_ptr(), rec.data_ptr(), L.stream_ptr()), "adam_ema")

    def plain(self, g, hyper):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                      self.state.data_ptr(), hyper.data_ptr(), L.stream_ptr()), "adam")

    def guarded(self, g, hyper, guard):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_guarded_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                              self.state.data_ptr(), hyper.data_ptr(), guard.data_ptr(), L.stream_ptr()), "adam_guarded")

    def accumulating(self, g, hyper, guard, accum):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_accum_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                            self.state.data_ptr(), hyper.data_ptr(), None if guard is None else guard.data_ptr(),
                                            accum.data_ptr(), L.stream_ptr()), "adam_accum")


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _grads(n, k, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * (0.5 + j)).cuda() for j in range(k)]


STEPS = 12


@pytest.mark.parametrize("n", [1, 5, 511, 513, 262151])      # the last: above 512 x 512, the grid-stride loop's second trip
def test_the_average_against_a_float64_recurrence(n):
    """E_k = E_{k-1} + w_k (P_k - E_{k-1}) in float64, fed the kernel's own p after step k and the w the record held before it.
    Bound 5 2^-24 M / (1 - decay), M = max(|p|, |e|) over the run: an update commits at most five roundings of at most 2^-24 M
    each (fmaf(w, p - e, e) commits two), the recurrence damps what was there by 1 - w <= 1, and the error never exceeds the
    geometric sum.  The weight: within 2^-22 of ema_weight(float32(decay), warmup, updates); updates == k after step k."""
    from gfv.ema import ema_weight
    hyper = _hyper()
    gs = _grads(n, STEPS)
    for decay in (0.9, 0.5):
        for warmup in (True, False):
            a = _Flat(n)
            rec = _ema_record(decay, warmup)
            d32 = float(np.float32(decay))
            E = a.e.cpu().double()
            M, worst = float(max(a.p.abs().max(), a.e.abs().max())), 0.0
            for k in range(1, STEPS + 1):
                r = _read_ema(rec)
                assert r["updates"] == k - 1 and r["decay"] == d32 and r["warmup"] == int(warmup) and r["rest"] == [0, 0, 0, 0]
                assert abs(r["w"] - ema_weight(d32, warmup, k - 1)) <= 2.0 ** -22, (k, r)
                a.ema_step(gs[k - 1], hyper, rec)
                torch.cuda.synchronize()
                P, e = a.p.cpu().double(), a.e.cpu().double()
                E = E + r["w"] * (P - E)
                M = max(M, float(P.abs().max()), float(e.abs().max()))
                err = float((e - E).abs().max())
                bound = 5 * EPS * M / (1.0 - decay)
                worst = max(worst, err / bound)
                assert err <= bound, (decay, warmup, k, err, bound)
            r = _read_ema(rec)
            assert r["updates"] == STEPS and abs(r["w"] - ema_weight(d32, warmup, STEPS)) <= 2.0 ** -22
            assert float(a.state[0]) == STEPS and int(a.state.view(torch.int32)[4]) == 0
            print(f"n={n} decay={decay} warmup={warmup}: worst error / bound {worst:.3f}")


N_ADAM = 70001     # 137 workgroups


@pytest.mark.parametrize("form", ["plain", "guarded", "accum", "guarded_accum"])
def test_adam_is_untouched(form):
    """p, m, v and the sixteen state words after 5 steps: those of the entry point without the average, bit for bit."""
    hyper = _hyper(1e-3)
    gs = _grads(N_ADAM, 5, seed=11)
    a = _Flat(N_ADAM)
    b = a.twin()
    rec = _ema_record(0.9, True)
    guard = _guard_record(0.5, CLIP) if "guarded" in form else None        # hand-written: a clipped, applied step
    accum = _accum_record(1) if "accum" in form else None                  # ... and a closing micro-step
    e0 = a.e.clone()
    for g in gs:
        a.ema_step(g, hyper, rec, guard=guard, accum=accum)
        if accum is not None:
            b.accumulating(g, hyper, guard, accum)
        elif guard is not None:
            b.guarded(g, hyper, guard)
        else:
            b.plain(g, hyper)
    assert _same(a.bits(), b.bits())
    assert float(a.state[0]) == 5.0 and _read_ema(rec)["updates"] == 5
    assert not torch.equal(a.e, e0) and torch.equal(b.e, e0)
    if form == "guarded":                                                   # (the coefficient is obeyed: not the plain step)
        c = _Flat(N_ADAM)
        c.plain(gs[0], hyper)
        d = _Flat(N_ADAM)
        d.ema_step(gs[0], hyper, _ema_record(0.9, True), guard=guard)
        assert not torch.equal(c.p, d.p)


@pytest.mark.parametrize("form", ["guard_skip", "accum_hold", "both"])
def test_no_trace_of_a_step_that_was_not_applied(form):
    hyper = _hyper(1e-3)
    g0, g1 = _grads(N_ADAM, 2, seed=13)
    a = _Flat(N_ADAM)
    rec = _ema_record(0.9, True)
    a.ema_step(g0, hyper, rec)                    # one applied step first: t = 1, updates = 1, something to lose
    guard = _guard_record(1.0, SKIP_NONFINITE) if form in ("guard_skip", "both") else None
    accum = _accum_record(0) if form in ("accum_hold", "both") else None
    if form == "both":
        guard = _guard_record(0.5, CLIP)          # (the guard would apply; the hold alone leaves the step out)
    before, e_before = a.bits(), a.e.cpu().view(torch.int32).clone()
    rec_before = rec.cpu().view(torch.int32).clone()
    assert int(rec_before[2]) == 1
    a.ema_step(g1, hyper, rec, guard=guard, accum=accum)
    torch.cuda.synchronize()
    assert _same(before, a.bits())                # p, m, v, all 16 words of the state - the arrival counter back at zero
    assert int(a.state.view(torch.int32)[4]) == 0
    assert torch.equal(a.e.cpu().view(torch.int32), e_before)
    assert torch.equal(rec.cpu().view(torch.int32), rec_before)
    a.ema_step(g1, hyper, rec)                    # ... and the next applied one counts on from where it was
    assert _read_ema(rec)["updates"] == 2 and float(a.state[0]) == 2.0


# ---- through the step objects ----------------------------------------------------------------------------------------------
LR = 1e-3
MESH = "cavity_mixed_b1"


def _graphs(name=MESH):
    return tuple(g.clone().to("cuda") for g in cases.make_graphs(name))


def _fresh_model(dataset_size):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    P = O.init_parameters(cases.WEIGHT_SEED)
    m = NNmodel(default_params(dataset_size=dataset_size))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def frozen_sd():
    """Model state after the Normalizer's accumulation has ended (dataset_size = 3: two accumulating steps), computed once."""
    from gfv.trainer import TrainStep
    model = _fresh_model(3).cuda()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False)
    for _ in range(3):
        ts.step()
    torch.cuda.synchronize()
    assert not model.node_norm.should_accumulate()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _model(sd):
    m = _fresh_model(3)
    m.load_state_dict(sd)
    m = m.cuda()
    assert not m.node_norm.should_accumulate()
    return m


def _named_bits(ts):
    """Parameters and moments of the named tensors (the alignment padding of the flat buffers is not state) + the Adam state."""
    torch.cuda.synchronize()
    ns = ts.named_state()
    return [torch.cat([v[j].reshape(-1) for v in ns.values()]).detach().cpu().view(torch.int32) for j in range(3)] + \
        [ts.adam_state.detach().cpu().view(torch.int32).clone()]


def _ema_bits(ts):
    """The average of the named tensors and the eight words of its record."""
    torch.cuda.synchronize()
    e = ts._ema.e
    return [torch.cat([e[ts.G.off[n]:ts.G.off[n] + ts.G.numel(n)] for n in ts.G.off]).detach().cpu().view(torch.int32),
            ts._ema.rec.detach().cpu().view(torch.int32).clone()]


def _run(sd, mode, steps=6, **kw):
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(sd), _graphs(), lr=LR, use_graph=mode, **kw)
    for _ in range(steps):
        ts.step()
    return ts


@pytest.fixture(scope="module")
def eager_ema(frozen_sd):
    ts = _run(frozen_sd, False, ema_decay=0.9)
    return _named_bits(ts), _ema_bits(ts)


@pytest.mark.parametrize("mode", [False, "list", True], ids=["eager", "list", "hipgraph"])
def test_trainstep_modes_agree_and_adam_is_the_plain_step(frozen_sd, eager_ema, mode):
    from gfv.ema import ema_weight
    ts = _run(frozen_sd, mode, ema_decay=0.9)
    assert ts.ema_decay == 0.9 and ts.ema_warmup is True
    assert _same(_ema_bits(ts), eager_ema[1])                  # e and the record: the bits of the eager run
    assert _same(_named_bits(ts), eager_ema[0])
    plain = _run(frozen_sd, mode)
    assert plain.ema_decay is None and plain._ema is None
    assert _same(_named_bits(ts), _named_bits(plain))          # flat_p, flat_m, flat_v, the Adam state: EMA on or off
    st = ts.ema_stats()
    assert set(st) == {"decay", "warmup", "updates", "w"}
    assert st["updates"] == 6 and st["warmup"] is True and st["decay"] == float(np.float32(0.9))   # (a hipGraph warm-up counts nothing)
    assert abs(st["w"] - ema_weight(float(np.float32(0.9)), True, 6)) <= 2.0 ** -22
    assert plain.ema_stats()["updates"] == 0 and plain.ema_stats()["decay"] is None
    if mode == "list":
        assert len(ts._lists) >= 1
    # the average is one: not the iterate, and between the start and the iterate where the parameters moved one way
    e, p = _ema_bits(ts)[0], _named_bits(ts)[0]
    assert not torch.equal(e, p)


def test_trainstep_counts_optimiser_steps_not_micro_steps(frozen_sd):
    ts = _run(frozen_sd, "list", ema_decay=0.9, accum_steps=2)
    assert ts.ema_stats()["updates"] == 3 and float(ts.adam_state[0]) == 3.0
    plain = _run(frozen_sd, "list", accum_steps=2)
    assert _same(_named_bits(ts), _named_bits(plain))


def test_trainstep_a_skipped_step_is_not_averaged(frozen_sd):
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(frozen_sd), _graphs(), lr=LR, use_graph=False, ema_decay=0.9, skip_nonfinite=True)
    twin = TrainStep(_model(frozen_sd), _graphs(), lr=LR, use_graph=False, ema_decay=0.9, skip_nonfinite=True)
    for t in (ts, twin):
        t.step()
        t.step()
    assert ts.ema_stats()["updates"] == 2
    before = _ema_bits(ts)
    name = next(n for n in ts.G.off if n not in ts.G.skip and ts.G.numel(n) > 0)
    adam = ts._adam

    def poisoned():                               # one gradient of a named tensor, between the backward and the guard's norm
        ts.flat_g[ts.G.off[name]] = float("nan")
        adam()
    ts._adam = poisoned
    ts.step()
    del ts._adam
    st = ts.guard_stats()
    assert st["skipped_nonfinite"] == 1 and st["decision"] == SKIP_NONFINITE
    assert ts.ema_stats()["updates"] == 2 and _same(before, _ema_bits(ts)) and float(ts.adam_state[0]) == 2.0
    for t in (ts, twin):                          # the next step: as if the bad one had never been issued
        t.step()
    assert ts.ema_stats()["updates"] == 3
    assert _same(_ema_bits(ts), _ema_bits(twin)) and _same(_named_bits(ts), _named_bits(twin))
    assert bool(torch.isfinite(ts._ema.e).all())


def test_attributes_follow_without_a_new_launch_sequence(frozen_sd):
    from gfv.ema import ema_weight
    ts = _run(frozen_sd, "list", ema_decay=0.9)
    lists = dict(ts._lists)
    assert lists
    ts.ema_decay = 0.5                            # a value: through gfv_ema_init, the count stays, the lists stay
    st = ts.ema_stats()
    assert st["decay"] == 0.5 and st["updates"] == 6 and st["w"] == pytest.approx(ema_weight(0.5, True, 6), abs=2.0 ** -22)
    ts.ema_warmup = False
    st = ts.ema_stats()
    assert st["warmup"] is False and st["updates"] == 6 and st["w"] == 0.5 and dict(ts._lists) == lists
    ts.step()
    assert ts.ema_stats()["updates"] == 7
    with pytest.raises(ValueError, match="ema_decay"):
        ts.ema_decay = 1.0
    ts.ema_decay = None                           # off: the launch sequence changes, the lists go
    assert ts._ema is None and not ts._lists and not ts._captures
    with pytest.raises(RuntimeError, match="ema_decay"):
        ts.ema_parameters()
    ts.ema_decay = 0.9                            # ... and on again: from the current parameters, counted from zero
    assert ts.ema_stats()["updates"] == 0 and ts.ema_warmup is False
    assert torch.equal(_ema_bits(ts)[0], _named_bits(ts)[0])
    ts.ema_reset()
    assert ts.ema_stats()["updates"] == 0


def _to_rollout(graphs):
    hg = tuple(g.clone().to("cuda") for g in graphs)
    hg[0].norm_uvp, hg[0].norm_global = True, True
    return hg


def test_the_swap_hands_the_average_to_the_model_and_takes_it_back(frozen_sd):
    from gfv.rollout import Rollout
    model = _model(frozen_sd)
    from gfv.trainer import TrainStep
    ts = TrainStep(model, _graphs(), lr=LR, use_graph="list", ema_decay=0.9)
    for _ in range(4):
        ts.step()
    torch.cuda.synchronize()
    avg = ts.ema_parameters()
    names, tensors = model.param_names_tensors()
    assert list(avg) == list(names) and all(avg[n].shape == t.shape and not avg[n].is_cuda for n, t in zip(names, tensors))
    p_before, e_before = ts.flat_p.detach().cpu().clone(), ts._ema.e.detach().cpu().clone()
    iterate = {n: t.detach().cpu().clone() for n, t in zip(names, tensors)}
    assert any(not torch.equal(avg[n], iterate[n]) for n in names)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    graphs = cases.make_graphs(MESH)
    with ts.ema_weights() as inside:
        assert inside is ts
        for n, t in zip(names, tensors):
            assert torch.equal(t.detach().cpu(), avg[n]), n
        assert all(torch.equal(v, avg[n]) for n, v in ts.ema_parameters().items())     # (the same answer inside the block)
        with pytest.raises(RuntimeError, match="ema_weights"):
            ts.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with ts.ema_weights():
                pass
        hist = Rollout(model, _to_rollout(graphs), max_steps=3).run(3)
    torch.cuda.synchronize()
    assert torch.equal(ts.flat_p.detach().cpu(), p_before) and torch.equal(ts._ema.e.detach().cpu(), e_before)
    for n, t in zip(names, tensors):
        assert torch.equal(t.detach().cpu(), iterate[n]), n
    # an independent model loaded with those parameters gives the rollout's bits
    for n in names:
        assert n in sd
        sd[n] = avg[n]
    other = Rollout(_model(sd), _to_rollout(graphs), max_steps=3).run(3)
    assert torch.equal(hist, other) and bool(torch.isfinite(hist).all())
    ts.step()                                     # training goes on
    assert ts.ema_stats()["updates"] == 5


def test_a_rollout_built_before_the_swap_is_told_to_refresh(frozen_sd):
    from gfv.rollout import Rollout
    from gfv.trainer import TrainStep
    model = _model(frozen_sd)
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False, ema_decay=0.9)
    ts.step()
    ro = Rollout(model, _to_rollout(cases.make_graphs(MESH)), max_steps=4)
    ro.step()
    with ts.ema_weights():
        with pytest.raises(RuntimeError, match="refresh_weights"):
            ro.step()
        ro.refresh_weights()
        ro.step()
    with pytest.raises(RuntimeError, match="refresh_weights"):
        ro.step()


def test_checkpoint(frozen_sd):
    from gfv.trainer import TrainStep
    plain = _run(frozen_sd, False, steps=1)
    assert set(plain.state_dict()) == {"state", "param_groups", "gfv_param_names", "gfv_loss_weights"}     # today's keys
    model = _model(frozen_sd)
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False, ema_decay=0.9)
    for _ in range(3):
        ts.step()
    sd = ts.state_dict()
    assert set(sd) == set(plain.state_dict()) | {"gfv_ema"}
    avg = sd["gfv_ema"]
    assert set(avg) == {"decay", "warmup", "updates", "params"} and avg["updates"] == 3 and avg["decay"] == 0.9
    assert len(avg["params"]) == len(sd["gfv_param_names"])
    # torch.optim.Adam takes the dict as it takes today's
    names, tensors = model.param_names_tensors()
    opt = torch.optim.Adam([torch.nn.Parameter(t.detach().clone()) for t in tensors], lr=LR)
    opt.load_state_dict(sd)
    torch.cuda.synchronize()
    msd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    second = TrainStep(_model(msd), _graphs(), lr=LR, use_graph=False, ema_decay=0.5, ema_warmup=False)
    second.load_state_dict(sd)
    assert _same(_ema_bits(ts), _ema_bits(second)) and second.ema_decay == 0.9 and second.ema_warmup is True
    assert _same(_named_bits(ts)[:3], _named_bits(second)[:3])
    ts.load_state_dict(sd)                        # (both twins form the bias corrections from the step count the same way)
    assert _same(_ema_bits(ts), _ema_bits(second)) and _same(_named_bits(ts), _named_bits(second))
    for t in (ts, second):
        t.step()
        t.step()
    assert _same(_ema_bits(ts), _ema_bits(second)) and _same(_named_bits(ts), _named_bits(second))
    assert ts.ema_stats()["updates"] == 5
    # a dict without the key: the average restarts from the (loaded) parameters
    old = {k: v for k, v in sd.items() if k != "gfv_ema"}
    second.load_state_dict(old)
    assert second.ema_stats()["updates"] == 0
    assert torch.equal(_ema_bits(second)[0], _named_bits(second)[0])
    assert torch.equal(second._ema.e, second.flat_p[:second.n_params])


def _two_size_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = [meshgen.raw_quad_cavity(n=7, jitter=0.1, tri_fraction=0.3, seed=13), meshgen.raw_poisson_cavity(n=6, seed=14)]
    ms = [meshgen.finish_mesh(r, U=U) for r, U in zip(raws, (1.0, None))]
    return DevicePool(ms, [meshgen.random_fields(m, seed=30 + i) for i, m in enumerate(ms)])


def test_pool_lists_replay_the_average(frozen_sd):
    from gfv.pool_trainer import PoolTrainStep
    seq = [[k % 2] for k in range(8)]             # per signature: two eager steps, the recording, one replay
    eager = PoolTrainStep(_model(frozen_sd), _two_size_pool(), max_graphs=1, lr=LR, use_graph=False, ema_decay=0.9)
    ts = PoolTrainStep(_model(frozen_sd), _two_size_pool(), max_graphs=1, lr=LR, use_graph="list", ema_decay=0.9)
    for idx in seq:
        eager.step(idx)
        ts.step(idx)
    st = ts.stats()
    assert st["lists"] == 2 and st["replayed"] > 0, st
    assert _same(_ema_bits(eager), _ema_bits(ts)) and _same(_named_bits(eager), _named_bits(ts))
    assert ts.ema_stats()["updates"] == 8
    with ts.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            ts.step([0])
