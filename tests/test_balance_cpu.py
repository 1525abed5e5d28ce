"""CPU: the host side of the loss balancing (gfv/balance.py, csrc/balance.hip): the entry point is declared, exported and bound and
refuses bad arguments before anything touches a device; the record a new object packs sits where include/gfv.h states; a state
goes round; the constructor refusals; and the properties of the rule, shown on tests/balance_ref.py - the restatement the GPU tests
compare the kernel with.  Nothing here touches a GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import balance_ref as R
import cases

W0 = (6e4, 5e4, 1.0)
U = 2.0 ** -53          # the unit roundoff of float64


def _terms(cont, mom, press, B=3):
    """B rows whose batch means are (cont, mom, press) up to rounding: mom split over its two columns."""
    return [[cont * (1 + 0.1 * (b - (B - 1) / 2)), 0.25 * mom, 0.75 * mom, press] for b in range(B)]


def test_balance_entry_point_is_declared_exported_and_bound():
    from gfv import balance as Bal
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    name = "gfv_loss_balance"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert len(getattr(handle, name).argtypes) == 6
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert name not in cmdlist._QUERIES
    for macro, value in (("RECORD", lib.BALANCE_RECORD), ("LANES", lib.BALANCE_LANES), ("INVERSE", lib.BALANCE_INVERSE),
                         ("PROGRESS", lib.BALANCE_PROGRESS)):
        assert int(re.search(rf"#define GFV_BALANCE_{macro} (\d+)", header).group(1)) == value, macro
    assert (R.INVERSE, R.PROGRESS, R.LANES) == (lib.BALANCE_INVERSE, lib.BALANCE_PROGRESS, lib.BALANCE_LANES)
    section = header[header.index("Loss balancing: the three residual weights"):header.index("#define GFV_BALANCE_RECORD")]
    for word, idx in (("kind", Bal.W_KIND), ("warmup", Bal.W_WARMUP), ("every", Bal.W_EVERY), ("n", Bal.W_N),
                      ("n_applied", Bal.W_N_APPLIED), ("n_updates", Bal.W_N_UPDATES), ("n_skipped", Bal.W_N_SKIPPED)):
        assert re.search(rf"\bw\[{idx}\]\s+{word}\b", section), word
    for word, idx in (("decay", Bal.D_DECAY), ("floor", Bal.D_FLOOR), ("alpha", Bal.D_ALPHA), ("tau", Bal.D_TAU),
                      ("power", Bal.D_POWER)):
        assert re.search(rf"\bd\[{idx}\]\s+{word}\b", section), word
    for word, idx in (("g", Bal.D_G), ("w0", Bal.D_W0), ("m", Bal.D_M), ("s", Bal.D_S), ("s_ref", Bal.D_SREF), ("lam", Bal.D_LAM),
                      ("w", Bal.D_W)):
        assert re.search(rf"\bd\[{idx}\.\.{idx + 2}\]\s+{word}\b", section), word
    assert Bal.D_W + 3 <= lib.BALANCE_RECORD and 2 * Bal.D_DECAY > Bal.W_N_SKIPPED


def test_loss_balance_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    ok = dict(losses=p, B=3, rec=p, hyper=p, hold=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_loss_balance(a["losses"], a["B"], a["rec"], a["hyper"], a["hold"], None)
    assert call(losses=None) == -1 and call(rec=None) == -1 and call(hyper=None) == -1
    assert call(B=0) == -1 and call(B=-5) == -1
    assert call(rec=p + 4) == -1                                           # not 8-byte aligned
    assert call(rec=p + 4, hold=None) == -1


def test_a_new_objects_record_is_what_the_header_states():
    from gfv import balance as Bal
    from gfv import lib as L
    inv = Bal.Inverse(shares=(2, 1, 0.5), decay=0.8, warmup=3, every=2, floor=1e-20)
    with pytest.raises(ValueError, match="base weights are not known"):
        inv.pack()
    inv.set_base(W0)
    d = inv.pack()
    w = d.view(torch.int32)
    assert d.numel() == L.BALANCE_RECORD and d.dtype == torch.float64
    assert [int(w[i]) for i in range(8)] == [L.BALANCE_INVERSE, 3, 2, 0, 0, 0, 0, 0]
    assert [float(v) for v in d[4:8]] == [0.8, 1e-20, 0.0, 0.0]
    assert [float(v) for v in d[8:14]] == [2.0, 1.0, 0.5, *W0]
    assert float(d[14]) == 1.0 and [float(v) for v in d[15:24]] == [0.0] * 9
    assert [float(v) for v in d[24:30]] == [1.0, 1.0, 1.0, *W0] and [float(v) for v in d[30:32]] == [0.0, 0.0]
    pro = Bal.Progress(alpha=0.7, tau=0.5)
    pro.set_base((1.0, 2.0, 3.0))
    d = pro.pack()
    w = d.view(torch.int32)
    assert [int(w[i]) for i in range(3)] == [L.BALANCE_PROGRESS, 10, 1]
    assert [float(v) for v in d[4:8]] == [0.9, 1e-30, 0.7, 0.5] and [float(v) for v in d[8:11]] == [1.0, 1.0, 1.0]
    assert [float(v) for v in d[Bal.D_W:Bal.D_W + 3]] == [1.0, 2.0, 3.0]
    # the defaults the issue names
    a, b = Bal.Inverse(), Bal.Progress()
    assert (a.shares, a.decay, a.warmup, a.every, a.floor) == ((1.0, 1.0, 1.0), 0.9, 10, 1, 1e-30)
    assert (b.alpha, b.tau, b.decay, b.warmup, b.every, b.floor) == (0.9, 1.0, 0.9, 10, 1, 1e-30)


def test_a_state_goes_round_through_a_packed_record():
    from gfv import balance as Bal
    ref = R.Balance(R.PROGRESS, W0, decay=0.5, warmup=1, every=1, alpha=0.6, tau=0.8)
    for i in range(4):
        ref.observe(_terms(1e-3 / (i + 1), 2e-3 / (i + 1) ** 2, 0.5))
    pro = Bal.Progress(alpha=0.6, tau=0.8, decay=0.5, warmup=1)
    pro.set_base(W0)
    sd = dict(ref.words(), power=ref.power, w0=list(W0), ema=ref.m, last=ref.s, s_ref=ref.s_ref, lam=ref.lam, weights=ref.w)
    d = Bal.state_into(sd, pro.pack())
    assert Bal.state_of(d) == sd                                           # exact: doubles in, doubles out
    w = d.view(torch.int32)
    assert [int(w[i]) for i in (Bal.W_KIND, Bal.W_WARMUP, Bal.W_EVERY)] == [R.PROGRESS, 1, 1]      # host words stay
    assert [int(w[i]) for i in (Bal.W_N, Bal.W_N_APPLIED, Bal.W_N_UPDATES, Bal.W_N_SKIPPED)] == [4, 4, 3, 0]
    assert [float(d[Bal.D_LAM + k]).hex() for k in range(3)] == [v.hex() for v in ref.lam]
    assert float(d[Bal.D_ALPHA]) == 0.6 and float(d[Bal.D_TAU]) == 0.8
    d2 = Bal.state_into(Bal.state_of(d), pro.pack())
    assert torch.equal(d2.view(torch.int64), d.view(torch.int64))
    with pytest.raises(RuntimeError, match="no device record"):
        pro.state_dict()
    with pytest.raises(ValueError, match="does not load into"):
        pro.load_state_dict(dict(sd, kind="Inverse"))


def test_argument_checks_and_refusals():
    from gfv import balance as Bal
    from gfv.march import check_step_args
    for bad in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(warmup=-1), dict(warmup=1.5), dict(every=0),
                dict(every=True), dict(floor=0.0), dict(floor=float("inf")), dict(shares=(1, 1)), dict(shares=(1, 0, 1)),
                dict(shares=(1, -1, 1)), dict(shares=(1, float("nan"), 1))):
        with pytest.raises(ValueError):
            Bal.Inverse(**bad)
    for bad in (dict(alpha=1.0), dict(alpha=-0.5), dict(tau=0.0), dict(tau=-1.0), dict(decay=2.0), dict(every=0)):
        with pytest.raises(ValueError):
            Bal.Progress(**bad)
    inv = Bal.Inverse()
    with pytest.raises(ValueError):
        inv.set_base((1.0, 2.0))
    with pytest.raises(ValueError):
        inv.set_base((1.0, -2.0, 1.0))
    with pytest.raises(RuntimeError, match="no device record"):
        inv.observe(torch.zeros(4), 1)
    with pytest.raises(RuntimeError, match="no device record"):
        inv.stats()
    # the step objects' refusals
    Bal.check_balance(None, True, 4)
    with pytest.raises(TypeError):
        Bal.check_balance("Inverse")
    with pytest.raises(ValueError, match="data parallelism"):
        Bal.check_balance(Bal.Inverse(), dist_on=True)
    with pytest.raises(ValueError, match="data parallelism"):
        Bal.check_balance(Bal.Inverse(), dist_on=False, world_size=2)
    taken = Bal.Inverse()
    taken._owner = object()
    with pytest.raises(ValueError, match="already attached"):
        Bal.check_balance(taken)
    with pytest.raises(ValueError, match="already attached"):
        taken._attach(object())
    with pytest.raises(ValueError, match="balance= is not supported"):
        check_step_args("list", dict(balance=Bal.Inverse()))
    check_step_args("list", dict(balance=None))


# ---- the rule itself, on the restatement ---------------------------------------------------------------------------------------------
def test_the_statistic_is_the_batch_mean_in_the_stated_order():
    losses = [[1e-3 * (b + 1), 2.0 ** -b, 3.0, 1e8 + b] for b in range(200)]
    s = R.statistic(losses)
    exact = [math.fsum(R.f32(r[0]) for r in losses) / 200, math.fsum(R.f32(r[1]) + R.f32(r[2]) for r in losses) / 200,
             math.fsum(R.f32(r[3]) for r in losses) / 200]
    for got, want in zip(s, exact):
        assert abs(got - want) <= 200 * 2.0 ** -53 * want
    # B = 1 .. 3: no rounding beyond the division
    assert R.statistic([[0.5, 0.25, 0.125, 2.0]]) == [0.5, 0.375, 2.0]
    assert R.statistic([[1.0, 1.0, 2.0, 4.0], [3.0, 0.0, 1.0, 0.0]]) == [2.0, 2.0, 2.0]
    # the order: b and b + 64 meet first, then the halves
    big = [[0.0] * 4 for _ in range(65)]
    big[0][0], big[64][0], big[32][0] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert R.statistic(big)[0] == 1.0 / 65                                # (1 + 2^-53) rounds to 1, twice
    big[32][0] = 0.0
    big[1][0], big[33][0] = 2.0 ** -53, 2.0 ** -53
    assert R.statistic(big)[0] == (1.0 + 2.0 ** -52) / 65                 # the two small ones meet first (j = 1, j = 33)


@pytest.mark.parametrize("shares", [(1, 1, 1), (3, 1, 0.25)])
def test_inverse_gives_every_class_its_share_of_the_base_residual(shares):
    ref = R.Balance(R.INVERSE, W0, g=shares, decay=0.7, warmup=2, every=1)
    hyper = [0.0] * 8
    published = 0
    for i in range(9):
        did = ref.observe(_terms(3e-4 / (i + 1), 7e-4 * 0.8 ** i, 0.2 + 0.01 * i, B=5), hyper=hyper)
        assert did == (i >= 2)
        if not did:
            assert ref.w == list(W0) and hyper[5:8] == [0.0] * 3
            continue
        published += 1
        G = sum(float(v) for v in shares)
        total = 0.0
        for k in range(3):
            part = ref.w[k] * ref.mh[k]
            # four roundings lie between g_k / G and this quotient (* R0, / mh, * mh, / R0), one more in the test's own g_k / G
            assert abs(part / ref.R0 - shares[k] / G) <= 6 * U * (shares[k] / G), (i, k)
            total += part
        # three roundings in every part (the shares themselves sum to 1 within 2 more), two in the test's sum
        assert abs(total - ref.R0) <= 8 * U * ref.R0
        assert hyper[5:8] == [R.f32(v) for v in ref.w]
    assert ref.n_updates == published == 7 and ref.n == ref.n_applied == 9
    # decay 0: the average is the statistic itself
    z = R.Balance(R.INVERSE, W0, decay=0.0, warmup=0)
    z.observe(_terms(1e-3, 2e-3, 0.5))
    assert z.mh == z.s == z.m and z.power == 0.0
    # the floor binds where a term vanishes: the weight stays finite
    f = R.Balance(R.INVERSE, W0, decay=0.0, warmup=0, floor=1e-6)
    f.observe(_terms(1e-3, 2e-3, 0.0))
    assert f.w[2] == ((1.0 / 3.0) * f.R0) / 1e-6 and math.isfinite(f.w[2])


def test_progress_keeps_the_sum_of_the_multipliers_and_ignores_a_common_rate():
    ref = R.Balance(R.PROGRESS, W0, decay=0.5, warmup=0, every=1, alpha=0.8, tau=0.3)
    for i in range(40):
        assert ref.observe(_terms(1e-3 * 0.9 ** i, 5e-3 * 0.99 ** i, 0.3 * 0.8 ** i))
        # per publish the sum of 3 * e_k / E is 3 within 12 U (two roundings in E, one per quotient and per product), the blend
        # adds (1 - alpha) * 6 U + 3 alpha U + 3 U: 9 U in all at alpha = 0.8, carried on with weight alpha - 9 U / (1 - alpha) = 45 U
        # at most, and 6 U for the test's own sum of three numbers near 1
        assert abs(sum(ref.lam) - 3.0) <= 51 * U
        assert ref.w == [W0[k] * ref.lam[k] for k in range(3)]
    assert ref.n_updates == 40
    assert ref.lam[1] > 1.0 > ref.lam[0] > ref.lam[2]                      # the slowest term gained weight, the fastest lost
    # all three terms fall at the same rate (powers of two: every quotient is exact): lam stays (1, 1, 1)
    same = R.Balance(R.PROGRESS, W0, decay=0.0, warmup=0, every=1, alpha=0.5, tau=1.0)
    for i in range(20):
        assert same.observe([[3.0 * 2.0 ** -i, 1.0 * 2.0 ** -i, 0.5 * 2.0 ** -i, 7.0 * 2.0 ** -i]])
        assert same.lam == [1.0, 1.0, 1.0] and same.w == list(W0)
    assert same.s_ref == same.mh


@pytest.mark.parametrize("kind", [R.INVERSE, R.PROGRESS])
def test_a_nan_or_negative_statistic_changes_nothing_but_n_skipped(kind):
    ref = R.Balance(kind, W0, decay=0.5, warmup=0, every=1)
    hyper = [0.0] * 8
    ref.observe(_terms(1e-3, 2e-3, 0.5), hyper=hyper)
    for n_bad, bad in enumerate((_terms(float("nan"), 2e-3, 0.5), _terms(1e-3, -2e-3, 0.5), _terms(1e-3, 2e-3, float("inf")),
                                 [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, -3.0]])):
        before = (dict(ref.words()), {k: list(v) for k, v in ref.doubles().items()}, list(hyper))
        assert ref.observe(bad, hyper=hyper) is False
        want = dict(before[0], n_skipped=n_bad + 1)
        assert ref.words() == want and ref.doubles() == before[1] and hyper == before[2]
    # a negative TERM whose batch mean is not negative is not rejected: the rule is about s
    assert ref.observe([[1.0, 1.0, 1.0, 3.0], [1.0, 1.0, 1.0, -1.0]], hyper=hyper) is True


def test_warmup_every_and_hold_gate_publishes_exactly_as_written():
    ref = R.Balance(R.INVERSE, W0, decay=0.5, warmup=3, every=2)
    holds = [None, 1, 0, 0, 1, 1, 0, 1, None, 0, 1, 1]
    got = [ref.observe(_terms(1e-3, 2e-3, 0.5), hold=h) for h in holds]
    n, n_applied, want = 0, 0, []
    for h in holds:
        n += 1
        applied = h is None or h != 0
        n_applied += 1 if applied else 0
        want.append(applied and n > 3 and n_applied % 2 == 0)
    assert got == want and sum(want) == 3 and want[:4] == [False] * 4
    assert (ref.n, ref.n_applied, ref.n_updates, ref.n_skipped) == (12, 8, 3, 0)
    # a held observation still moves the average, and nothing is published behind it even where n_applied % every == 0 holds
    h = R.Balance(R.INVERSE, W0, decay=0.5, warmup=0, every=1)
    assert h.observe(_terms(1e-3, 2e-3, 0.5), hold=0) is False
    assert h.n == 1 and h.n_applied == 0 and h.m[0] > 0.0 and h.w == list(W0)
    assert h.observe(_terms(1e-3, 2e-3, 0.5), hold=1) is True
