"""Parameter groups on the GPU (include/gfv.h gfv_adam_step_groups_dev, gfv/groups.py): the grouped Adam launch at
the C ABI against the launches without groups, `gfv.optim.Adam` / `AdamW` with groups against the torch.optim class of the same
name, frozen groups and gradient-less parameters that keep their bits, the guard's norm over the live parameters, and end to
end through `TrainStep`: the driver sequence with torch.optim.AdamW, values that move under a recorded list, unfreezing, the
combination with guard + accumulation + averaged weights, a narrow model, and the checkpoint.

The accuracy bound of the kernel-level comparisons is not a fixed number.  The torch optimiser runs twice on the same gradients,
in fp32 and in float64; D is the largest absolute difference between those two runs (per quantity: p, exp_avg, exp_avg_sq, over
all tensors), and the fused result must lie within 2 D of the float64 run: the kernel is a second fp32 evaluation of the same
recurrence, whose roundings differ in place (where the decay term is added, a product formed in another order), not in number."""
import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 17, 511, 512, 513, 4101, 300001]   # one element; one short of, on, one past the 512-thread block; a tail; more
#                                                    than one grid sweep of 512 x 512 elements (the stride wraps inside a run)
GROUPS = [(1e-3, 0.1), (3e-3, 0.0), (5e-4, 0.5)]  # (lr, weight_decay) of the groups [0::3], [1::3], [2::3]
LR_MOVES_AT, LR_MOVED_TO = 17, 1e-3               # group 1's lr at step 17
BETAS, EPS = (0.9, 0.999), 1e-8


def _lib():
    from gfv import lib as L
    return L, L.load()


def _start(seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(k, generator=gen) for k in SIZES]


_GRADS = {}


def _grads(steps, seed=11):
    """randn * (1 + step) per tensor and step, fp32 on the host; computed once per length."""
    if steps not in _GRADS:
        gen = torch.Generator().manual_seed(seed)
        _GRADS[steps] = [[torch.randn(k, generator=gen) * (1 + s) for k in SIZES] for s in range(steps)]
    return _GRADS[steps]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. one group is the kernel without groups ---------------------------------------------------------------------------------
class _Flat:
    def __init__(self):
        from gfv.engine import GradStore
        self.store = GradStore([str(i) for i in range(len(SIZES))], [(k,) for k in SIZES], "cuda")
        n = self.n = self.store.total
        gen = torch.Generator().manual_seed(3)
        self.p = torch.randn(n, generator=gen).cuda()
        self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.e = self.p.clone()
        self.state = torch.zeros(16, device="cuda")
        self.ema = torch.zeros(8, device="cuda")
        L, lib = _lib()
        L.check(lib.gfv_adam_state_init(self.state.data_ptr(), *BETAS, 0.0, L.stream_ptr()), "state_init")
        L.check(lib.gfv_ema_init(self.ema.data_ptr(), 0.9, 1, 0, L.stream_ptr()), "ema_init")

    def bits(self):
        torch.cuda.synchronize()
        return [t.detach().cpu().view(torch.int32).clone() for t in (self.p, self.m, self.v, self.state, self.e, self.ema)]


@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
@pytest.mark.parametrize("form", ["plain", "guard_accum_ema"])
def test_one_live_group_without_decay_is_the_launch_without_groups(form, decoupled):
    from gfv.groups import ParamGroups
    L, lib = _lib()
    a, b = _Flat(), _Flat()
    pg = ParamGroups(b.store, "cuda", {str(i): 0 for i in range(len(SIZES))}, [(1e-3, 0.0, False)], decoupled)
    assert pg.n_runs == len(SIZES)
    hyper = torch.tensor([1e-3, *BETAS, EPS, 1.0, 0.0, 0.0, 0.0], device="cuda")
    guard = torch.zeros(8, device="cuda")
    guard[3] = 0.5                                   # a clip coefficient, decision 0: applied
    accum = torch.zeros(8, dtype=torch.int32, device="cuda")
    accum[3] = 1                                     # apply
    accum = accum.view(torch.float32)
    full = form != "plain"
    gen = torch.Generator().manual_seed(11)
    for step in range(10):
        g = (torch.randn(a.n, generator=gen) * (1 + step)).cuda()
        if step == 5:
            hyper[0] = 2.5e-4                        # an lr change on the way: hyper[0] there, the group's row here
            pg.sync([(2.5e-4, 0.0, False)], decoupled)
        st = L.stream_ptr()
        if full:
            L.check(lib.gfv_adam_step_ema_dev(a.p.data_ptr(), g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.e.data_ptr(), a.n,
                                              a.state.data_ptr(), hyper.data_ptr(), guard.data_ptr(), accum.data_ptr(),
                                              a.ema.data_ptr(), st), "adam_ema")
        else:
            L.check(lib.gfv_adam_step_dev(a.p.data_ptr(), g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.n, a.state.data_ptr(),
                                          hyper.data_ptr(), st), "adam")
        L.check(lib.gfv_adam_step_groups_dev(b.p.data_ptr(), g.data_ptr(), b.m.data_ptr(), b.v.data_ptr(),
                                             b.e.data_ptr() if full else None, b.n, b.state.data_ptr(), hyper.data_ptr(),
                                             guard.data_ptr() if full else None, accum.data_ptr() if full else None,
                                             b.ema.data_ptr() if full else None, pg.run_start.data_ptr(), pg.run_group.data_ptr(),
                                             pg.n_runs, pg.table.data_ptr(), st), "adam_groups")
    assert float(a.state[0]) == 10.0
    assert _same(a.bits(), b.bits())


# ---- 2. groups against torch ---------------------------------------------------------------------------------------------------
def _torch_run(decoupled, dtype, steps, clip=None, frozen=(), no_grad=(), lr_move=True):
    """torch.optim.Adam / AdamW on the host over the shared gradients -> (p, exp_avg, exp_avg_sq per tensor (None without state),
    norms).  frozen: group indices left alone; no_grad: tensor indices whose .grad is None every step."""
    ps = [torch.nn.Parameter(t.clone().to(dtype)) for t in _start()]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": ps[k::3], "lr": lr, "weight_decay": wd} for k, (lr, wd) in enumerate(GROUPS)], betas=BETAS, eps=EPS)
    dead = set(no_grad) | {i for i in range(len(ps)) if i % 3 in frozen}
    norms = []
    for step, grads in enumerate(_grads(steps)):
        if lr_move and step == LR_MOVES_AT:
            opt.param_groups[1]["lr"] = LR_MOVED_TO
        for i, p in enumerate(ps):
            p.grad = None if i in dead else grads[i].clone().to(dtype)
        if clip is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, clip)))
        opt.step()
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        out.append((p.detach().clone(), st.get("exp_avg"), st.get("exp_avg_sq")))
    return out, norms


_REF = {}


def _reference(decoupled, steps, **kw):
    """(float64 run, D per quantity, norms of the fp32 run); computed once per configuration."""
    key = (decoupled, steps, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        r32, norms = _torch_run(decoupled, torch.float32, steps, **kw)
        r64, _ = _torch_run(decoupled, torch.float64, steps, **kw)
        D = [max(float((a[j].double() - b[j]).abs().max()) for a, b in zip(r32, r64) if a[j] is not None) for j in range(3)]
        _REF[key] = (r64, D, norms)
    return _REF[key]


def _fused(decoupled, steps, frozen=(), no_grad=(), lr_move=True, only=None, **kw):
    """gfv.optim.Adam / AdamW over the shared gradients.  only: the tensor indices handed to the optimiser (default: all)."""
    from gfv.optim import Adam, AdamW
    idx = list(range(len(SIZES))) if only is None else list(only)
    start = _start()
    ps = {i: torch.nn.Parameter(start[i].clone().cuda()) for i in idx}
    groups = []
    for k, (lr, wd) in enumerate(GROUPS):
        members = [ps[i] for i in idx if i % 3 == k]
        if members:
            groups.append(dict({"params": members, "lr": lr, "weight_decay": wd, "tag": k}, **({"frozen": True} if k in frozen else {})))
    opt = (AdamW if decoupled else Adam)(groups, betas=BETAS, eps=EPS, **kw)
    norms = []
    for step, grads in enumerate(_grads(steps)):
        if lr_move and step == LR_MOVES_AT:
            next(g for g in opt.param_groups if g["tag"] == 1)["lr"] = LR_MOVED_TO
        for i, p in ps.items():
            p.grad = None if i in no_grad else grads[i].cuda()
        opt.step()
        if kw.get("max_grad_norm") is not None:
            norms.append(opt.guard_stats()["norm"])
    torch.cuda.synchronize()
    return opt, ps, norms


def _moments(opt, ps):
    """{tensor index: (exp_avg, exp_avg_sq)} views of the optimiser's flat moment buffers."""
    out = {}
    index = {id(p): i for i, p in ps.items()}        # (the optimiser holds the parameters group by group)
    for p, off in zip(opt._params, opt._offs):
        k = p.numel()
        out[index[id(p)]] = (opt.flat_m[off:off + k].detach().cpu(), opt.flat_v[off:off + k].detach().cpu())
    return out


def _within_2D(ref64, D, ps, mom, what):
    err = [0.0, 0.0, 0.0]
    for i, p in ps.items():
        r = ref64[i]
        if r[1] is None:
            continue
        err[0] = max(err[0], float((p.detach().cpu().double() - r[0]).abs().max()))
        err[1] = max(err[1], float((mom[i][0].double() - r[1]).abs().max()))
        err[2] = max(err[2], float((mom[i][1].double() - r[2]).abs().max()))
    print(f"{what}: D (p, m, v) = {D}; err = {err}; err / D = {[e / d for e, d in zip(err, D)]}")
    for e, d, q in zip(err, D, "pmv"):
        assert d > 0 and e <= 2.0 * d, (what, q, e, d)


@pytest.mark.parametrize("decoupled", [False, True], ids=["Adam", "AdamW"])
def test_three_groups_follow_torch(decoupled):
    """40 steps, three groups (lr 1e-3 / 3e-3 / 5e-4, weight_decay 0.1 / 0 / 0.5), one group's lr changed at step 17.
    Measured on the MI355X (err / D for p, exp_avg, exp_avg_sq): see DESIGN.md 5i."""
    ref64, D, _ = _reference(decoupled, 40)
    opt, ps, _ = _fused(decoupled, 40)
    assert float(opt.adam_state[0]) == 40.0 and opt._pg is not None
    _within_2D(ref64, D, ps, _moments(opt, ps), "AdamW" if decoupled else "Adam")
    # the checkpoint nesting is torch's: the class of the same name loads it, group values included
    sd = opt.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [1e-3, LR_MOVED_TO, 5e-4]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.1, 0.0, 0.5]
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5], [6, 7]]
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps.values()]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    t = cls([{"params": twin[k::3]} for k in range(3)])
    t.load_state_dict(sd)
    assert [g["weight_decay"] for g in t.param_groups] == [0.1, 0.0, 0.5]
    assert t.param_groups[0]["decoupled_weight_decay"] is decoupled


def _abi_run(decoupled, steps, table_of=lambda i: i % 3):
    """gfv_adam_step_groups_dev itself over SIZES laid out in index order, run i in group table_of(i): with i % 3 every pair of
    neighbouring runs differs in rate and decay, and the 300 001-element run that wraps the grid carries a decay."""
    from gfv.engine import GradStore
    from gfv.groups import ParamGroups
    L, lib = _lib()
    store = GradStore([str(i) for i in range(len(SIZES))], [(k,) for k in SIZES], "cuda")
    n = store.total
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    for i, t in enumerate(_start()):
        p[store.off[str(i)]:store.off[str(i)] + t.numel()] = t.cuda()
    state = torch.zeros(16, device="cuda")
    L.check(lib.gfv_adam_state_init(state.data_ptr(), *BETAS, 0.0, L.stream_ptr()), "state_init")
    hyper = torch.tensor([float("nan"), *BETAS, EPS, 1.0, 0.0, 0.0, 0.0], device="cuda")   # (hyper[0] is not read)
    vals = [(lr, wd, False) for lr, wd in GROUPS]
    pg = ParamGroups(store, "cuda", {str(i): table_of(i) for i in range(len(SIZES))}, vals, decoupled)
    assert pg._rows == [table_of(i) for i in range(len(SIZES))]
    g = torch.zeros(n, device="cuda")
    for step, grads in enumerate(_grads(steps)):
        if step == LR_MOVES_AT:
            vals[1] = (LR_MOVED_TO, vals[1][1], False)
            pg.sync(vals, decoupled)
        for i, t in enumerate(grads):
            g[store.off[str(i)]:store.off[str(i)] + t.numel()] = t.cuda()
        L.check(lib.gfv_adam_step_groups_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, state.data_ptr(),
                                             hyper.data_ptr(), None, None, None, pg.run_start.data_ptr(), pg.run_group.data_ptr(),
                                             pg.n_runs, pg.table.data_ptr(), L.stream_ptr()), "adam_groups")
    torch.cuda.synchronize()
    cut = lambda buf, i: buf[store.off[str(i)]:store.off[str(i)] + SIZES[i]].detach().cpu()
    ps = {i: cut(p, i) for i in range(len(SIZES))}
    return ps, {i: (cut(m, i), cut(v, i)) for i in range(len(SIZES))}, state


@pytest.mark.parametrize("decoupled", [False, True], ids=["Adam", "AdamW"])
def test_alternating_groups_at_the_c_abi_follow_torch(decoupled):
    """The launch itself with the groups dealt round-robin over neighbouring RUNS (gfv.optim lays its buffer out group by group,
    so there only two run boundaries change group): 40 steps against the same torch reference, the same 2 D rule."""
    ref64, D, _ = _reference(decoupled, 40)
    ps, mom, state = _abi_run(decoupled, 40)
    assert float(state[0]) == 40.0
    _within_2D(ref64, D, ps, mom, "C ABI, alternating runs, " + ("AdamW" if decoupled else "Adam"))


# ---- 3. frozen is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["Adam", "AdamW"])
def test_frozen_group_and_gradient_less_parameter_keep_their_bits(decoupled):
    NO_GRAD = 5                                      # (513 elements, in the group with weight_decay 0.5)
    start = _start()
    opt, ps, _ = _fused(decoupled, 10, frozen=(1,), no_grad=(NO_GRAD,), lr_move=False)
    mom = _moments(opt, ps)
    still = [i for i in ps if i % 3 == 1] + [NO_GRAD]
    for i in still:
        assert torch.equal(ps[i].detach().cpu().view(torch.int32), start[i].view(torch.int32)), i
        assert not mom[i][0].any() and not mom[i][1].any(), i
    sd = opt.state_dict()
    order = list(ps)                                 # position in the optimiser = order of the groups' members
    pos = {i: k for k, i in enumerate([i for g in range(3) for i in order if i % 3 == g])}
    assert set(sd["state"]) == {pos[i] for i in ps if i not in still}
    assert float(opt.adam_state[0]) == 10.0
    # the live parameters: the same run with the others taken out of the optimiser, bit for bit
    live = [i for i in ps if i not in still]
    opt2, ps2, _ = _fused(decoupled, 10, lr_move=False, only=live)
    mom2 = _moments(opt2, ps2)
    for i in live:
        assert torch.equal(ps[i].detach().cpu().view(torch.int32), ps2[i].detach().cpu().view(torch.int32)), i
        assert torch.equal(mom[i][0], mom2[i][0]) and torch.equal(mom[i][1], mom2[i][1]), i
        assert not torch.equal(ps[i].detach().cpu(), start[i])


# ---- 4. the guard sees the live parameters ------------------------------------------------------------------------------------
def test_guard_norm_covers_the_live_parameters_and_the_clipped_step_follows_torch():
    NO_GRAD, CLIP_AT, STEPS = 5, 1.0, 10
    kw = dict(frozen=(1,), no_grad=(NO_GRAD,), lr_move=False)
    ref64, D, norms = _reference(True, STEPS, clip=CLIP_AT, **kw)
    assert all(n > CLIP_AT for n in norms)           # clipping acts on every step
    # the frozen group's gradients are real numbers in the flat buffer: a norm over everything would be larger
    with_frozen = [float(torch.sqrt(sum((g.double() ** 2).sum() for i, g in enumerate(gs) if i != NO_GRAD))) for gs in _grads(STEPS)]
    assert all(w > 1.0001 * n for w, n in zip(with_frozen, norms))
    opt, ps, got = _fused(True, STEPS, max_grad_norm=CLIP_AT, **kw)
    for a, b in zip(norms, got):
        assert abs(a - b) < 1e-4 * abs(a), (a, b)
    assert opt.guard_stats()["clipped"] == STEPS
    _within_2D(ref64, D, ps, _moments(opt, ps), "AdamW, clipped")
    start = _start()
    for i in [i for i in ps if i % 3 == 1] + [NO_GRAD]:
        assert torch.equal(ps[i].detach().cpu().view(torch.int32), start[i].view(torch.int32)), i


# ---- through TrainStep ---------------------------------------------------------------------------------------------------------
LR, WD, CASE, STEPS = 1e-3, 0.05, "cyl_cavity_b2", 6
ENC, DEC = "simulator.encoder", "simulator.decoder"


def _model(seed=cases.WEIGHT_SEED, **kw):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    params = default_params(dataset_size=1, **kw)
    hyper = {"hidden_size": kw["hidden_size"], "net": "TransFVGN_v2"} if "hidden_size" in kw else None
    P0 = O.init_parameters(seed, hyper) if hyper else O.init_parameters(seed)
    model = NNmodel(params)
    sd = model.state_dict()
    for k, v in P0.items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    return model.to("cuda"), params


def _graphs(name=CASE):
    return tuple(g.clone().to("cuda") for g in cases.make_graphs(name))


def _named_bits(ts):
    torch.cuda.synchronize()
    ns = ts.named_state()
    return [torch.cat([v[j].reshape(-1) for v in ns.values()]).detach().cpu().view(torch.int32) for j in range(3)] + \
        [ts.adam_state.detach().cpu().view(torch.int32).clone()]


def _param_groups(model):
    """The recipe of the issue with this model's names: no decay on biases and vectors (those of the processor blocks - encoder and
    decoder have groups of their own, and a parameter belongs to one group), the encoders frozen, the decoder at a tenth of the rate."""
    from gfv.groups import no_decay_names
    nd = [n for n in no_decay_names(model) if not n.startswith(ENC + ".") and not n.startswith(DEC + ".")]
    return [{"params": nd, "weight_decay": 0.0}, {"params": [ENC], "frozen": True}, {"params": [DEC], "lr_scale": 0.1}]


def _start_values(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


_DRIVER = {}


def _driver_reference():
    """loss.backward(); torch.optim.AdamW(same groups).step() on the drop-in model, computed once.  The frozen encoders are not
    handed to the optimiser (torch has no frozen key)."""
    if not _DRIVER:
        model, params = _model()
        graphs = _graphs()
        named = dict(model.named_parameters())
        spec = _param_groups(model)
        nd, dec = set(spec[0]["params"]), {n for n in named if n.startswith(DEC + ".")}
        enc = {n for n in named if n.startswith(ENC + ".")}
        rest = [n for n in named if n not in nd | dec | enc]
        opt = torch.optim.AdamW([{"params": [named[n] for n in named if n in nd], "weight_decay": 0.0},
                                 {"params": [named[n] for n in named if n in dec], "lr": LR * 0.1},
                                 {"params": [named[n] for n in rest]}], lr=LR, weight_decay=WD)
        gn = graphs[0]
        backup = gn.x.clone()
        losses = []
        for _ in range(STEPS):
            gn.x.copy_(backup)
            gn.norm_uvp, gn.norm_global = params.norm_uvp, params.norm_global
            opt.zero_grad()
            lc, lx, ly, lp, un, uc = model(*graphs)
            loss = torch.mean(torch.log(params.loss_press * lp + params.loss_cont * lc + params.loss_mom * lx + params.loss_mom * ly))
            loss.backward()
            opt.step()
            losses.append(float(loss))
        _DRIVER["ref"] = ({n: p.detach().cpu().clone() for n, p in named.items()}, losses,
                          {n: (LR * 0.1 if n in dec else LR) for n in named})
    return _DRIVER["ref"]


@pytest.mark.parametrize("mode", [False, "list"])
def test_trainstep_follows_backward_then_adamw_with_the_same_groups(mode):
    from gfv.functions import unused_param_names
    from gfv.trainer import TrainStep
    want, want_losses, lr_of = _driver_reference()
    model, params = _model()
    start = _start_values(model)
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=mode, weight_decay=WD, param_groups=_param_groups(model))
    assert [g["frozen"] for g in ts.param_groups] == [False, True, False, False] and ts.weight_decay == WD
    assert [g["weight_decay"] for g in ts.param_groups] == [0.0, WD, WD, WD] and ts.param_groups[2]["lr"] == LR * 0.1
    losses = [float(ts.step()) for _ in range(STEPS)]
    torch.cuda.synchronize()
    if mode == "list":
        assert len(ts._lists) >= 1
    for a, b in zip(want_losses, losses):
        assert abs(a - b) < 1e-5 * abs(a), (a, b)
    got = _start_values(model)
    unused = unused_param_names(list(got))
    assert unused
    moved = 0
    for n, a in want.items():
        assert float((a - got[n]).abs().max()) < 0.02 * lr_of[n], n
        if n.startswith(ENC + ".") or n in unused:
            # frozen, or without a gradient: the bits of the start - also where a decay of 0.05 would have moved them
            assert torch.equal(got[n].view(torch.int32), start[n].view(torch.int32)), n
        else:
            moved += int(not torch.equal(got[n], start[n]))
    assert moved > 100


# ---- 6. values move without re-recording --------------------------------------------------------------------------------------
def test_new_group_values_reach_a_recorded_list():
    """The same sequence - three steps, then a new lr_scale and weight_decay for the decoder's group and a new lr, then two steps -
    in list mode and in eager mode: the recorded list stays the object it was and the results are the eager ones bit for bit.
    An eager object is the yardstick because it reads every value at every launch."""
    from gfv.trainer import TrainStep
    out = {}
    for mode in (False, "list"):
        model, _ = _model()
        ts = TrainStep(model, _graphs(), lr=LR, use_graph=mode, weight_decay=WD, param_groups=_param_groups(model))
        for _ in range(3):
            ts.step()
        recorded = {k: e.cl for k, e in ts._lists.items()}
        assert bool(recorded) == (mode == "list") and ts.stats()["recorded"] == len(recorded)
        before = _named_bits(ts)
        ts.set_group(2, lr_scale=0.5, weight_decay=0.2)
        ts.lr = 2.5e-4
        assert ts.param_groups[2]["lr"] == 2.5e-4 * 0.5 and ts.param_groups[2]["weight_decay"] == 0.2
        losses = [ts.step().clone() for _ in range(2)]
        assert ts._lists.keys() == recorded.keys() and ts.stats()["recorded"] == len(recorded)
        assert all(ts._lists[k].cl is v for k, v in recorded.items())      # nothing was recorded again
        out[mode] = (_named_bits(ts), [l.cpu() for l in losses], before)
    assert _same(out[False][2], out["list"][2])
    assert _same(out[False][0], out["list"][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out["list"][1]))
    assert not torch.equal(out[False][0][0], out[False][2][0])


def test_pool_training_replays_new_group_values():
    from gfv import meshgen
    from gfv.pool import DevicePool
    from gfv.pool_trainer import PoolTrainStep
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    seq = [[0], [1], [2], [3], [0], [1]]
    res = {}
    for mode in (False, "list"):
        pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
        for j in range(3):
            pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
        model, _ = _model()
        ts = PoolTrainStep(model, pool, lr=LR, use_graph=mode, weight_decay=WD, param_groups=_param_groups(model))
        recorded = []
        for k, idx in enumerate(seq):
            if k == 4:
                ts.set_group(0, weight_decay=0.3)
                ts.set_group(2, lr_scale=1.0)
                ts.lr = 5e-4
            ts.step(idx)
            recorded.append(ts.stats()["recorded"])
        res[mode] = (_named_bits(ts), recorded, ts.stats())
    assert res["list"][1] == [0, 0, 1, 1, 1, 1] and res["list"][2]["replayed"] == 3
    assert _same(res[False][0], res["list"][0])


# ---- 7. unfreeze ---------------------------------------------------------------------------------------------------------------
def _restated(p, m, v, g, t, lr, wd, decoupled, b1=BETAS[0], b2=BETAS[1], eps=EPS):
    """One step of the update as include/gfv.h states it, in the dtype of its arguments; t: the count this step carries."""
    if wd != 0 and not decoupled:
        g = g + wd * p
    if wd != 0 and decoupled:
        p = p * (1.0 - lr * wd)
    m = m * b1 + (1.0 - b1) * g
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps
    return p - (lr / (1.0 - b1 ** t)) * (m / denom), m, v


def test_an_unfrozen_group_continues_with_the_shared_step_count():
    """The documented deviation: the decoder, frozen for three steps and then unfrozen by set_group, takes its first step with
    zero moments and the SHARED count 4 (torch, counting per parameter, would use 1).  Checked against the float64 restatement
    of the update, with D = the distance between the restatement evaluated in fp32 and in float64 and the bound 2 D."""
    from gfv.trainer import TrainStep
    model, _ = _model()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False, weight_decay=WD, param_groups=[{"params": [DEC], "frozen": True}])
    dec = list(ts.param_groups[0]["params"])
    start = _start_values(model)
    for _ in range(3):
        ts.step()
    ns = ts.named_state()
    for n in dec:
        assert torch.equal(ns[n][0].cpu(), start[n]) and not ns[n][1].any() and not ns[n][2].any()
    assert set(ts.state_dict()["state"]).isdisjoint({list(ts.G.off).index(n) for n in dec})
    ts.set_group(0, frozen=False)
    assert ts.param_groups[0]["frozen"] is False
    ts.step()
    torch.cuda.synchronize()
    assert float(ts.adam_state[0]) == 4.0
    assert {list(ts.G.off).index(n) for n in dec} <= set(ts.state_dict()["state"])
    err, D = [0.0] * 3, [0.0] * 3
    for n in dec:
        g = ts.G.view(n).detach().cpu()              # the gradient of step 4, still in the flat buffer
        p0 = start[n]
        z = torch.zeros_like(p0)
        w64 = _restated(p0.double(), z.double(), z.double(), g.double(), 4, LR, WD, True)
        w32 = _restated(p0, z, z, g, 4, LR, WD, True)
        with_one = _restated(p0.double(), z.double(), z.double(), g.double(), 1, LR, WD, True)
        got = [t.detach().cpu() for t in ts.named_state()[n]]
        for j in range(3):
            err[j] = max(err[j], float((got[j].double() - w64[j]).abs().max()))
            D[j] = max(D[j], float((w32[j].double() - w64[j]).abs().max()))
        # (a bias correction started at 1 gives a step 1.7 times as long: the two readings are far apart)
        assert float((got[0].double() - with_one[0]).abs().max()) > 100 * float((got[0].double() - w64[0]).abs().max())
    print(f"unfreeze: D (p, m, v) = {D}; err = {err}; err / D = {[e / d for e, d in zip(err, D)]}")
    for e, d in zip(err, D):
        assert d > 0 and e <= 2.0 * d, (e, d)


def test_groups_beside_a_group_that_is_unfrozen_later_do_not_notice():
    """The other groups are bit-identical to a run where nothing was ever frozen - where the gradients are inputs (in a model the
    other groups' gradients depend on the frozen group's weights, so there the two runs differ from the first step on)."""
    start = _start()
    out = {}
    for freeze in (True, False):
        from gfv.optim import AdamW
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in start]
        opt = AdamW([dict({"params": ps[k::3], "lr": lr, "weight_decay": wd}, **({"frozen": True} if freeze and k == 1 else {}))
                     for k, (lr, wd) in enumerate(GROUPS)], betas=BETAS, eps=EPS)
        for step, grads in enumerate(_grads(10)[:5]):
            if step == 3:
                opt.param_groups[1]["frozen"] = False
            for p, g in zip(ps, grads):
                p.grad = g.cuda()
            opt.step()
        torch.cuda.synchronize()
        out[freeze] = [p.detach().cpu() for p in ps]
    for i in range(len(SIZES)):
        assert torch.equal(out[True][i], out[False][i]) == (i % 3 != 1), i
        assert not torch.equal(out[True][i], start[i])


# ---- 8. combinations, once -----------------------------------------------------------------------------------------------------
def test_groups_with_guard_accumulation_and_averaged_weights():
    from gfv.trainer import TrainStep
    model, _ = _model()
    start = _start_values(model)
    ts = TrainStep(model, _graphs(), lr=LR, use_graph="list", weight_decay=WD, param_groups=_param_groups(model), accum_steps=2,
                   ema_decay=0.9, max_grad_norm=1e-3, skip_nonfinite=True)

    def bits():
        torch.cuda.synchronize()
        return _named_bits(ts) + [ts._ema.e.detach().cpu().view(torch.int32).clone(), ts._ema.rec.detach().cpu().view(torch.int32).clone()]
    for k in range(8):                               # warm-up, recording, replays: micro-steps 0, 2, 4, 6 hold
        before = bits()
        ts.step()
        assert _same(before, bits()) == (k % 2 == 0), k
    assert float(ts.adam_state[0]) == 4.0 and ts.ema_stats()["updates"] == 4
    assert len(ts._lists) >= 1
    st = ts.guard_stats()
    assert st["clipped"] == 4 and st["decision"] == 1 and st["norm"] > 1e-3
    avg = ts.ema_parameters()
    got = _start_values(model)
    for n in start:
        if n.startswith(ENC + "."):
            assert torch.equal(avg[n], start[n]) and torch.equal(got[n], start[n]), n
    assert sum(int(not torch.equal(avg[n], start[n])) for n in start) > 100


def test_narrow_model_with_two_groups_matches_its_eager_mode():
    from gfv.trainer import TrainStep
    out = {}
    for mode in (False, "list"):
        model, _ = _model(hidden_size=64)
        ts = TrainStep(model, _graphs(), lr=LR, use_graph=mode, weight_decay=WD, param_groups=[{"params": [DEC], "lr_scale": 0.1,
                                                                                               "weight_decay": 0.0}])
        assert ts.padded and len(ts.param_groups) == 2
        losses = [ts.step().clone() for _ in range(4)]
        out[mode] = (_named_bits(ts), [l.cpu() for l in losses])
    assert _same(out[False][0], out["list"][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out["list"][1]))


def test_grouped_step_in_hipgraph_mode_matches_eager():
    """The third launch mode: a captured graph holds the table pointers, so new group values reach its replays."""
    from gfv.trainer import TrainStep
    out = {}
    for mode in (False, True):
        model, _ = _model()
        ts = TrainStep(model, _graphs(), lr=LR, use_graph=mode, weight_decay=WD, param_groups=_param_groups(model))
        losses = []
        for k in range(4):
            if k == 2:
                ts.set_group(2, lr_scale=0.5, weight_decay=0.2)
                ts.lr = 2.5e-4
            losses.append(ts.step().clone())
        if mode:
            assert 1 <= len(ts._captures) <= 2 and not ts._lists        # a capture per (accumulate, distributed) key: nothing captured again
        out[mode] = (_named_bits(ts), [l.cpu() for l in losses])
    assert _same(out[False][0], out[True][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out[True][1]))


def test_set_group_checks_before_it_changes_anything():
    from gfv.trainer import TrainStep
    model, _ = _model()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False, param_groups=[{"params": [ENC, DEC], "frozen": True}])
    before = ts.param_groups
    table = ts._pg.table.clone()
    with pytest.raises(ValueError, match="nothing left to optimise"):
        ts.set_group(1, frozen=True)                 # the default group is the last one that moves
    with pytest.raises(ValueError, match="weight_decay"):
        ts.set_group(0, lr_scale=0.5, weight_decay=-1.0)
    assert ts.param_groups == before and torch.equal(ts._pg.table, table)
    ts.step()
    torch.cuda.synchronize()


# ---- 9. checkpoint -------------------------------------------------------------------------------------------------------------
def test_checkpoint_of_a_grouped_trainstep():
    from gfv.trainer import TrainStep
    model, _ = _model()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False, weight_decay=WD, param_groups=_param_groups(model))
    for _ in range(3):
        ts.step()
    ts.set_group(2, lr_scale=0.25)
    sd = ts.state_dict()
    torch.cuda.synchronize()
    names = sd["gfv_param_names"]
    assert set(sd) == {"state", "param_groups", "gfv_param_names", "gfv_loss_weights", "gfv_groups"}
    assert len(sd["param_groups"]) == 4 and sorted(i for g in sd["param_groups"] for i in g["params"]) == list(range(len(names)))
    assert [g["lr"] for g in sd["param_groups"]] == [LR, LR, LR * 0.25, LR]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, WD, WD, WD]
    enc = {i for i, n in enumerate(names) if n.startswith(ENC + ".")}
    assert enc and enc.isdisjoint(sd["state"]) and enc == set(sd["param_groups"][1]["params"])
    # a fresh grouped object, built with other values: the dict brings the values back, the next step is the same step
    msd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model2, _ = _model()
    model2.load_state_dict(msd)
    other = [dict(g) for g in _param_groups(model2)]
    other[2]["lr_scale"], other[0]["weight_decay"] = 1.0, 0.3
    second = TrainStep(model2, _graphs(), lr=7e-4, use_graph=False, weight_decay=0.01, param_groups=other)
    second.load_state_dict(sd)
    assert second.lr == LR and second.weight_decay == WD and second.param_groups == ts.param_groups
    ts.load_state_dict(sd)                           # (both twins form the bias corrections from the step count the same way)
    assert _same(_named_bits(ts), _named_bits(second))
    for t in (ts, second):
        t.step()
    assert _same(_named_bits(ts), _named_bits(second)) and float(second.adam_state[0]) == 4.0
    # torch.optim.AdamW with the same grouping takes it
    tensors = [torch.nn.Parameter(t.detach().cpu().clone()) for t in model.param_names_tensors()[1]]
    opt = torch.optim.AdamW([{"params": [tensors[i] for i in g["params"]]} for g in sd["param_groups"]], lr=1.0, weight_decay=9.0)
    opt.load_state_dict({k: sd[k] for k in ("state", "param_groups")})
    assert [g["lr"] for g in opt.param_groups] == [LR, LR, LR * 0.25, LR]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, WD, WD, WD]
    assert all(g["decoupled_weight_decay"] is True for g in opt.param_groups)
    assert len(opt.state) == len(sd["state"])
    # a dict with another grouping is refused before a buffer is touched
    bits = _named_bits(second)
    wrong = dict(sd, param_groups=[dict(g) for g in sd["param_groups"][::-1]])
    with pytest.raises(ValueError, match="different parameter grouping"):
        second.load_state_dict(wrong)
    assert _same(bits, _named_bits(second)) and second.param_groups == ts.param_groups
    # a dict without groups - a pre-training checkpoint - loads into the grouped object: moments and count from the dict, the
    # groups and the rate stay the object's own; and what moves has state from then on, also where the dict had none
    pre, _ = _model()
    pre_ts = TrainStep(pre, _graphs(), lr=3e-3, use_graph=False)
    pre_ts.step()
    pre_sd = pre_ts.state_dict()
    groups_before = second.param_groups
    second.load_state_dict(pre_sd)
    assert second.param_groups == groups_before and second.lr == LR and float(second.adam_state[0]) == 1.0
    assert _same(_named_bits(second)[1:3], _named_bits(pre_ts)[1:3])
    second.load_state_dict({"state": {}, "param_groups": pre_sd["param_groups"]})
    second.step()
    live = {i for i, n in enumerate(names) if not n.startswith(ENC + ".") and i in pre_sd["state"]}
    assert set(second.state_dict()["state"]) == live and float(second.adam_state[0]) == 1.0
    # an object without groups keeps today's keys, and today's single group
    model3, _ = _model()
    plain = TrainStep(model3, _graphs(), lr=LR, use_graph=False)
    plain.step()
    psd = plain.state_dict()
    assert set(psd) == {"state", "param_groups", "gfv_param_names", "gfv_loss_weights"} and plain._pg is None
    assert len(psd["param_groups"]) == 1 and set(psd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad",
                                                                             "maximize", "params"}
