"""Training guard on the GPU (include/gfv.h gfv_grad_guard_dev / gfv_adam_step_guarded_dev, gfv/guard.py): the
global-norm launch and the guarded Adam at the C ABI - which slots the norm reads, one rounding, same bits every run, the clip
coefficient of clip_grad_norm_, bit identity with the plain Adam launch where the guard has nothing to do, a skipped step that
leaves no trace - and end to end: `TrainStep`, `PoolTrainStep` and `gfv.optim.Adam` with the guard on, in every launch mode,
against `loss.backward(); clip_grad_norm_(...); torch.optim.Adam.step()` on the drop-in model."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

TILE = 1024   # elements one workgroup of the norm launch takes per trip (csrc/misc.hip GUARD_TILE); its grid is at most 256
CLIP, SKIP_NONFINITE, SKIP_FLAG = 1, 2, 4


# ---- the C ABI on flat buffers ---------------------------------------------------------------------------------------------
def _lib():
    from gfv import lib as L
    return L, L.load()


def _hyper(lr=1e-3, grad_scale=1.0):
    return torch.tensor([lr, 0.9, 0.999, 1e-8, grad_scale, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _record(max_norm, policy):
    rec = torch.zeros(8, dtype=torch.int32)
    rec[0] = struct.unpack("i", struct.pack("f", max_norm))[0]
    rec[1] = policy
    return rec.cuda().view(torch.float32)


def _read(rec):
    f = rec.detach().cpu()
    i = f.view(torch.int32)
    return dict(norm=f[2].clone(), coef=f[3].clone(), decision=int(i[4]), clipped=int(i[5]), nonfinite=int(i[6]), flag=int(i[7]))


def _workspace():
    L, lib = _lib()
    return torch.zeros(lib.gfv_grad_guard_workspace_bytes() // 8, dtype=torch.float64, device="cuda")


def _table(segs):
    return torch.tensor(segs, dtype=torch.int64).reshape(-1).cuda()


def _guard(g, table, n_seg, n_elems, hyper, rec, ws):
    L, lib = _lib()
    L.check(lib.gfv_grad_guard_dev(g.data_ptr(), table.data_ptr(), n_seg, n_elems, hyper.data_ptr(), rec.data_ptr(), ws.data_ptr(),
                                   L.stream_ptr()), "grad_guard")


class _Flat:
    """p, m, v, state of one Adam run over n slots."""

    def __init__(self, n, seed=3):
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, generator=gen).cuda()
        self.m = torch.zeros(n, device="cuda")
        self.v = torch.zeros(n, device="cuda")
        self.state = torch.zeros(16, device="cuda")
        L, lib = _lib()
        L.check(lib.gfv_adam_state_init(self.state.data_ptr(), 0.9, 0.999, 0.0, L.stream_ptr()), "state_init")

    def plain(self, g, hyper):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                      self.state.data_ptr(), hyper.data_ptr(), L.stream_ptr()), "adam")

    def guarded(self, g, hyper, rec, table, n_seg, n_elems, ws):
        L, lib = _lib()
        _guard(g, table, n_seg, n_elems, hyper, rec, ws)
        L.check(lib.gfv_adam_step_guarded_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                              self.state.data_ptr(), hyper.data_ptr(), rec.data_ptr(), L.stream_ptr()), "adam_guarded")

    def bits(self):
        torch.cuda.synchronize()
        return [t.detach().cpu().view(torch.int32).clone() for t in (self.p, self.m, self.v, self.state)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _layout(counts, seed=0):
    """One flat buffer holding a segment of every count, at odd offsets with gaps of 1 - 7 slots; every slot outside a
    segment is NaN."""
    gen = torch.Generator().manual_seed(seed)
    segs, off = [], 3
    for j, k in enumerate(counts):
        segs.append((off, k))
        off += k + 1 + (j * 5) % 7
    flat = torch.full((off + 5,), float("nan"))
    for j, (o, k) in enumerate(segs):
        flat[o:o + k] = torch.randn(k, generator=gen) * (10.0 ** ((j % 5) - 2))
    return flat, segs


# 1, 3, 4, 5, 1025 elements; one short of a tile, a tile + 1 (= 1025), two tiles + 1; and 300 001 (293 tiles: more than the
# grid of 256 workgroups, so the workgroups come round a second time)
NORM_LAYOUTS = {"small": [1, 3, 4, 5, 1025, TILE - 1, TILE + 1, 2 * TILE + 1],
                "one_element": [1],
                "grid_stride": [5, 300001, 1, TILE - 1]}


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("layout", list(NORM_LAYOUTS))
def test_norm_reads_exactly_the_segments_and_rounds_once(layout, grad_scale):
    flat, segs = _layout(NORM_LAYOUTS[layout])
    want64 = sum(float(((flat[o:o + k].double() * grad_scale) ** 2).sum()) for o, k in segs)   # (each piece summed in float64)
    parts = torch.cat([flat[o:o + k] for o, k in segs]).double() * grad_scale
    want = np.float32(np.sqrt(float((parts * parts).sum())))
    assert abs(np.sqrt(want64) - float(want)) <= float(np.spacing(want))
    g = flat.cuda()
    table, n_elems = _table(segs), sum(k for _, k in segs)
    hyper, ws = _hyper(grad_scale=grad_scale), _workspace()
    rec = _record(0.0, SKIP_NONFINITE)       # (a NaN read from outside a segment would show as a skipped step, too)
    _guard(g, table, len(segs), n_elems, hyper, rec, ws)
    torch.cuda.synchronize()
    first = _read(rec)
    got = np.float32(first["norm"].item())
    print(f"norm {layout} scale {grad_scale}: got {got!r} want {want!r}")
    assert np.isfinite(got)
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), (got, want)
    assert first["decision"] == 0 and first["coef"].item() == 1.0
    assert first["clipped"] == first["nonfinite"] == first["flag"] == 0
    assert int(ws.view(torch.int32)[0]) == 0      # the arrival counter is back at zero
    _guard(g, table, len(segs), n_elems, hyper, rec, ws)
    torch.cuda.synchronize()
    again = _read(rec)
    assert torch.equal(again["norm"].view(torch.int32), first["norm"].view(torch.int32))


def test_clip_coefficient_is_clip_grad_norms():
    flat, segs = _layout([5, 1025, 77])
    g = flat.cuda()
    table, n_elems, hyper, ws = _table(segs), sum(k for _, k in segs), _hyper(), _workspace()
    rec = _record(1e30, CLIP)
    _guard(g, table, len(segs), n_elems, hyper, rec, ws)
    torch.cuda.synchronize()
    r = _read(rec)
    norm = r["norm"]
    assert r["coef"].item() == 1.0 and r["decision"] == 0 and r["clipped"] == 0     # below the bound: exactly one
    for frac in (0.5, 0.999, 1e-3):
        max_norm = torch.tensor(float(norm) * frac, dtype=torch.float32)
        rec = _record(float(max_norm), CLIP)
        _guard(g, table, len(segs), n_elems, hyper, rec, ws)
        torch.cuda.synchronize()
        r = _read(rec)
        assert torch.equal(r["norm"].view(torch.int32), norm.view(torch.int32))
        want = max_norm / (r["norm"] + torch.tensor(1e-6, dtype=torch.float32))     # fp32 add, fp32 divide
        assert want.dtype == torch.float32 and float(want) < 1.0
        assert torch.equal(r["coef"].view(torch.int32), want.view(torch.int32)), (float(r["coef"]), float(want))
        assert r["decision"] == CLIP and r["clipped"] == 1
    # clipping off: the coefficient is exactly one whatever max_norm holds
    rec = _record(1e-9, SKIP_NONFINITE)
    _guard(g, table, len(segs), n_elems, hyper, rec, ws)
    torch.cuda.synchronize()
    assert _read(rec)["coef"].item() == 1.0


N_ADAM = 70001     # 137 workgroups of the Adam launch, 69 of the norm launch; not a multiple of anything


def _grads(n, steps, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * (0.1 + k)).cuda() for k in range(steps)]


def test_guard_with_nothing_to_do_is_the_plain_adam_bit_for_bit():
    n = N_ADAM
    a, b = _Flat(n), _Flat(n)
    table, ws, rec = _table([(0, n)]), _workspace(), _record(1e30, CLIP | SKIP_NONFINITE | SKIP_FLAG)
    hyper = _hyper()
    for k, g in enumerate(_grads(n, 5)):
        hyper[0] = 1e-3 * (1.0 + 0.5 * k)
        a.plain(g, hyper)
        b.guarded(g, hyper, rec, table, 1, n, ws)
        assert _same(a.bits(), b.bits()), k       # p, m, v and all 16 words of state
    r = _read(rec)
    assert r["coef"].item() == 1.0 and r["decision"] == 0 and r["clipped"] == r["nonfinite"] == r["flag"] == 0
    assert float(b.state[0]) == 5.0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipped_step_is_the_plain_step_on_the_scaled_gradient(grad_scale):
    n = N_ADAM
    a, b = _Flat(n), _Flat(n)
    table, ws, hyper = _table([(0, n)]), _workspace(), _hyper(grad_scale=grad_scale)
    rec = _record(3.0, CLIP)
    for k, g in enumerate(_grads(n, 3)):
        b.guarded(g, hyper, rec, table, 1, n, ws)
        torch.cuda.synchronize()
        r = _read(rec)
        assert r["decision"] == CLIP and 0.0 < float(r["coef"]) < 1.0 and r["clipped"] == k + 1
        a.plain(g * r["coef"].cuda(), hyper)      # a torch fp32 multiply by the coefficient read back
        assert _same(a.bits(), b.bits()), k


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_step_is_left_out_without_a_trace(bad):
    n = 5000
    segs = [(0, 1000), (1004, 2996), (4000, 1000)]      # slots 1000 - 1003: padding behind the first tensor
    skipped = (1004, 2996)                              # ... and in the second table this tensor is one without a gradient
    table, n_elems = _table(segs), sum(k for _, k in segs)
    table2, n_elems2 = _table([segs[0], segs[2]]), segs[0][1] + segs[2][1]
    ws, hyper = _workspace(), _hyper()
    g0, g1, g2 = _grads(n, 3)
    gbad = g1.clone()
    gbad[1500] = bad                                    # a real slot
    a, b = _Flat(n), _Flat(n)                           # a never sees the bad step
    rec_a, rec_b = _record(1e30, CLIP | SKIP_NONFINITE), _record(1e30, CLIP | SKIP_NONFINITE)
    a.guarded(g0, hyper, rec_a, table, 3, n_elems, ws)
    b.guarded(g0, hyper, rec_b, table, 3, n_elems, ws)
    before = b.bits()
    b.guarded(gbad, hyper, rec_b, table, 3, n_elems, ws)
    assert _same(before, b.bits())                      # p, m, v, state (step count, running powers, counter): untouched
    r = _read(rec_b)
    assert r["decision"] == SKIP_NONFINITE and r["nonfinite"] == 1 and r["clipped"] == 0 and r["flag"] == 0
    assert not np.isfinite(float(r["norm"]))
    a.guarded(g2, hyper, rec_a, table, 3, n_elems, ws)
    b.guarded(g2, hyper, rec_b, table, 3, n_elems, ws)
    assert _same(a.bits(), b.bits())                    # the next finite step: as if the bad one had never been issued
    assert _read(rec_b)["decision"] == 0 and _read(rec_b)["nonfinite"] == 1 and float(b.state[0]) == 2.0
    # the same value where the norm must not look: behind a tensor, and in a tensor the table leaves out
    for slot, tab, ns, ne in ((1001, table, 3, n_elems), (1500, table2, 2, n_elems2)):
        gpad = g1.clone()
        gpad[slot] = bad
        rec = _record(1e30, CLIP | SKIP_NONFINITE)
        c = _Flat(n)
        c.guarded(gpad, hyper, rec, tab, ns, ne, ws)
        torch.cuda.synchronize()
        r = _read(rec)
        assert r["decision"] == 0 and r["nonfinite"] == 0 and np.isfinite(float(r["norm"]))
        assert float(c.state[0]) == 1.0 and bool(torch.isfinite(c.p[:1000]).all()) and bool((c.m[:1000] != 0).any())


# ---- end to end ------------------------------------------------------------------------------------------------------------
LR = 1e-3


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


def _graphs(name="cyl_cavity_b2"):
    return tuple(g.clone().to("cuda") for g in cases.make_graphs(name))


def _flat_state(ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().view(torch.int32).clone() for t in (ts.flat_p[:ts.n_params], ts.flat_m, ts.flat_v, ts.adam_state)]


def _named_bits(ts):
    """Parameters and moments of the named tensors only (the alignment padding of the flat buffers is not state)."""
    torch.cuda.synchronize()
    ns = ts.named_state()
    return [torch.cat([v[j].reshape(-1) for v in ns.values()]).detach().cpu().view(torch.int32) for j in range(3)] + \
        [ts.adam_state.detach().cpu().view(torch.int32).clone()]


@pytest.mark.parametrize("mode", [False, "list", True])
def test_trainstep_with_an_idle_guard_is_bit_identical_in_every_mode(mode):
    from gfv.trainer import TrainStep
    out = {}
    for guard in (False, True):
        model, _ = _model()
        ts = TrainStep(model, _graphs(), lr=LR, use_graph=mode, **(dict(max_grad_norm=1e30) if guard else {}))
        losses = [ts.step().clone() for _ in range(5)]
        out[guard] = (_named_bits(ts), [l.cpu() for l in losses], ts)
    assert _same(out[False][0], out[True][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out[True][1]))
    st = out[True][2].guard_stats()
    assert set(st) == {"norm", "coef", "decision", "clipped", "skipped_nonfinite", "skipped_flag"}
    assert st["norm"] > 0.0 and st["coef"] == 1.0 and st["decision"] == 0
    assert st["clipped"] == st["skipped_nonfinite"] == st["skipped_flag"] == 0      # (a hipGraph warm-up counts nothing)
    assert float(out[True][2].adam_state[0]) == 5.0
    if mode == "list":
        assert len(out[True][2]._lists) >= 1
    # the guard's counters are not optimizer state: torch.optim.Adam loads the state_dict as before
    model2, _ = _model()
    opt = torch.optim.Adam(model2.parameters(), lr=LR)
    opt.load_state_dict({k: v for k, v in out[True][2].state_dict().items() if k in ("state", "param_groups")})


def test_clipped_count_is_the_number_of_steps_above_the_bound():
    from gfv.trainer import TrainStep
    model, _ = _model()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph="list", max_grad_norm=1e30)
    ts.step()
    first = ts.guard_stats()["norm"]
    ts.max_grad_norm = 0.5 * first          # (an attribute like lr: mirrored into the device record)
    assert ts.max_grad_norm == 0.5 * first
    above = 0
    for k in range(6):                      # warm-up, recording and replays of the list: the bound reaches all of them
        ts.step()
        st = ts.guard_stats()
        hit = st["norm"] > np.float32(0.5 * first)
        above += int(hit)
        assert (st["coef"] < 1.0) == hit and st["decision"] == (CLIP if hit else 0)
    assert above >= 1 and ts.guard_stats()["clipped"] == above
    assert len(ts._lists) >= 1
    with pytest.raises(ValueError):
        ts.max_grad_norm = -1.0


def _reference_clipped(case, steps, frac, **kw):
    """loss.backward(); clip_grad_norm_(model.parameters(), c); torch.optim.Adam.step() on the drop-in model; c = frac * the
    first step's norm."""
    model, params = _model(**kw)
    graphs = _graphs(case)
    opt = torch.optim.Adam(model.parameters(), lr=params.lr)
    gn = graphs[0]
    backup = gn.x.clone()
    c, losses, norms = None, [], []
    for _ in range(steps):
        gn.x.copy_(backup)
        gn.norm_uvp, gn.norm_global = params.norm_uvp, params.norm_global
        opt.zero_grad()
        lc, lx, ly, lp, un, uc = model(*graphs)
        loss = torch.mean(torch.log(params.loss_press * lp + params.loss_cont * lc + params.loss_mom * lx + params.loss_mom * ly))
        loss.backward()
        if c is None:
            # (max_norm = inf: the coefficient is clamped to one, the gradients are multiplied by 1.0 - this call only measures)
            c = frac * float(torch.nn.utils.clip_grad_norm_(model.parameters(), float("inf")))
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), c)))
        opt.step()
        losses.append(float(loss))
    assert all(n > c for n in norms), (c, norms)        # clipping acts on every step
    return model, params, c, losses, norms


def _compare(ref, model, losses, norms, lr):
    mt, _, c, lt, nt = ref
    for a, b in zip(lt, losses):
        assert abs(a - b) < 1e-5 * abs(a), (a, b)
    for (n, a), b in zip(mt.named_parameters(), model.parameters()):
        assert float((a.detach() - b.detach()).abs().max()) < 0.02 * lr, n
    for a, b in zip(nt, norms):
        assert abs(a - b) < 1e-4 * abs(a), (a, b)


@pytest.mark.parametrize("case,steps,kw", [("cyl_cavity_b2", 6, {}), ("cavity_mixed_b1", 6, {}), ("cyl_cavity_b2", 2, {"hidden_size": 64})],
                         ids=["cyl_cavity_b2", "cavity_mixed_b1", "hidden64"])
def test_clipped_training_follows_clip_grad_norm_then_adam(case, steps, kw):
    from gfv.optim import Adam
    from gfv.trainer import TrainStep
    # c = 1 % of the first step's norm: on these cases the reference's own norm falls by up to 8.5x within six steps (1.40 ->
    # 0.165 on cyl_cavity_b2), so a bound that is to act on EVERY step has to sit well below the first norm; _reference_clipped
    # asserts that it did.  (Adam's step is invariant to the gradient's scale down to eps = 1e-8, far below 1 % of these gradients)
    ref = _reference_clipped(case, steps, 0.01, **kw)
    c, lr = ref[2], ref[1].lr
    # the fused step
    model, params = _model(**kw)
    ts = TrainStep(model, _graphs(case), lr=params.lr, use_graph="list", max_grad_norm=c)
    losses, norms = [], []
    for _ in range(steps):
        losses.append(float(ts.step()))
        st = ts.guard_stats()
        norms.append(st["norm"])
        assert st["decision"] == CLIP
    assert ts.guard_stats()["clipped"] == steps
    _compare(ref, model, losses, norms, lr)
    # the drop-in optimiser
    model, params = _model(**kw)
    graphs = _graphs(case)
    opt = Adam(model.parameters(), lr=params.lr, max_grad_norm=c)
    gn = graphs[0]
    backup = gn.x.clone()
    losses, norms = [], []
    for _ in range(steps):
        gn.x.copy_(backup)
        gn.norm_uvp, gn.norm_global = params.norm_uvp, params.norm_global
        opt.zero_grad()
        lc, lx, ly, lp, un, uc = model(*graphs)
        loss = torch.mean(torch.log(params.loss_press * lp + params.loss_cont * lc + params.loss_mom * lx + params.loss_mom * ly))
        loss.backward()
        opt.step()
        losses.append(float(loss))
        norms.append(opt.guard_stats()["norm"])
    assert opt.guard_stats()["clipped"] == steps and float(opt.adam_state[0]) == steps
    _compare(ref, model, losses, norms, lr)


@pytest.mark.parametrize("mode", [False, "list"])
def test_skip_on_flag_keeps_the_last_good_parameters(mode):
    """GFV_FLAG_CHAIN_RANGE raised as tests/test_dropin_gpu.py::test_status_word_reaches_the_training_loop raises it, with a
    learning rate that moves the parameters.  FloatingPointError arrives at the next step as ever; with skip_on_flag the flagged
    step was never applied - parameters, both moments and the step count are those of before it - without it they have moved."""
    from gfv import lib as L
    from gfv.trainer import TrainStep
    moved = {}
    for skip in (True, False):
        model, params = _model()
        ts = TrainStep(model, _graphs(), use_graph=mode, lr=LR, skip_on_flag=skip)
        for _ in range(4):
            ts.step()
        torch.cuda.synchronize()
        L.raise_on_status("test")    # a healthy run raises nothing
        assert ts.guard_stats()["skipped_flag"] == 0
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "GN_block_list.0.eb_module.net.0.2.weight" in n:
                    p.mul_(3.0e5)
        before = _flat_state(ts)      # (taken after the scaling: every word of the flat buffers)
        assert float(ts.adam_state[0]) == 4.0
        with pytest.raises(FloatingPointError, match="GFV_FLAG"):
            for _ in range(6):
                ts.step()
                torch.cuda.synchronize()
        after = _flat_state(ts)
        moved[skip] = [not torch.equal(a, b) for a, b in zip(before, after)]
        flags = C.c_int32(0)
        L.check(L.load().gfv_status_flags(C.byref(flags)), "gfv_status_flags")
        assert int(flags.value) == 0 and int(L.status_mirror()[0]) == 0
        st = ts.guard_stats() if skip else None
        if skip:
            assert st["skipped_flag"] == 1 and st["decision"] & SKIP_FLAG
            assert float(ts.adam_state[0]) == 4.0
        else:
            assert float(ts.adam_state[0]) == 5.0
    assert moved[True] == [False, False, False, False], moved
    assert moved[False] == [True, True, True, True], moved


def _variant_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
    for j in range(3):
        pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
    return pool


def test_pool_training_replays_the_guard_and_follows_its_bound():
    from gfv.pool_trainer import PoolTrainStep
    seq = [[0], [1], [2], [3], [0], [1], [1], [2]]      # (steps 5 and 6: the same batch, so their norms are neighbours)
    res, bound = {}, None
    for use_graph in (False, "list"):
        model, _ = _model()
        ts = PoolTrainStep(model, _variant_pool(), lr=LR, use_graph=use_graph, max_grad_norm=1e30, skip_nonfinite=True)
        coefs, recorded = [], []
        for k, idx in enumerate(seq):
            if k == 1:
                if bound is None:
                    bound = 0.05 * ts.guard_stats()["norm"]     # (measured once, by the eager run; the same value for both)
                ts.max_grad_norm = bound
            if k == 6:
                ts.max_grad_norm = 0.1 * bound
            ts.step(idx)
            coefs.append(ts.guard_stats()["coef"])
            recorded.append(ts.stats()["recorded"])
        res[use_graph] = (_named_bits(ts), coefs, recorded, ts.stats(), ts.guard_stats())
    bits, coefs, recorded, stats, gst = res["list"]
    assert stats["replayed"] > 0 and stats["recorded"] == 1
    assert _same(res[False][0], bits)
    assert coefs == res[False][1]
    # steps 5 and 6 are both replays of the one list; the bound moved in between and the coefficient followed, nothing re-recorded
    assert recorded[5] == recorded[6] == recorded[7] == 1
    assert coefs[0] == 1.0 and coefs[5] < 1.0 and coefs[6] < 0.5 * coefs[5]
    assert gst["clipped"] >= 2 and gst["skipped_nonfinite"] == 0


def test_guarded_step_through_rccl_one_rank_is_bit_identical():
    """distributed=True, world_size=1: the identity all-reduce path of tests/test_rccl_gpu.py with max_grad_norm on - the guard
    sits behind the all-reduce in the data-parallel tail and the bits are those of the non-distributed run."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grad_guard_rccl_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29700 + (os.getpid() % 90)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), worker], capture_output=True, text=True, timeout=600, env=env)
    lines = re.findall(r"GUARDRESULT mode=(\S+) same=(\d) clipped=(\d+) backend=(\S+) world=(\d+)", r.stdout)
    assert r.returncode == 0 and len(lines) == 2 and "GUARDOK 1" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    for mode, same, clipped, backend, world in lines:
        assert backend == "nccl" and world == "1"
        assert same == "1", f"{mode}: a one-rank RCCL step with the guard on must be bit-identical to the non-distributed one"
        assert int(clipped) >= 1
