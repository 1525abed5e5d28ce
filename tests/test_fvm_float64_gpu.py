"""GPU: the finite-volume kernels of csrc/fvm.hip alone - no network in front of them - against the float64 restatement of
tests/fvm_float64.py, stage by stage and one loss of one graph at a time, on meshes whose per-graph PDE coefficients are all
distinct (`distinct_coefficients`: a kernel reading theta[2] for theta[3], sigma[3b] for sigma[3b+1], theta[9b] for theta[9b+1],
another graph's dt or dropping the source computes something else; tests/test_fvm_float64_cpu.py holds each of these to move a
compared column by more than 100 x its tolerance).

How a comparison is made, everywhere below: per column - each channel of each stage, each residual column, each loss of each
graph, each channel of the decoder-output gradient - normalised by that column's reference maximum over the rows of ONE graph.
The tolerance comes from the reference: the float32 oracle's own error against the float64 reference on the same inputs,
measured inside the test, times 4 (the kernels sum CSR rows in another order than torch's scatter, and a column's error is a
maximum over ~1e3 rows), with a floor of 2^-22.  A column whose reference is identically zero (pads, the outlet term of a graph
without an outlet) must be exactly zero.  Derived bounds instead of measured ones in (a) - 8 * 2^-24: a few float32 roundings and
tanhf - and in (e) - 2 (ceil(n / 1024) + 11) 2^-24 of a sum of non-negative addends.

Measured on the MI355X (largest column of each family over all cases, per-graph max-normalised; yardstick = the float32 oracle
on the same inputs, of which the tolerance is 4 x per column):

    family                                   yardstick             kernels
    phi against the closed form (a)          bound 4.8e-07         values 5.5e-08, gradients 7.6e-08
    2nd order: grad                          1.9e-06 ... 2.1e-06   8.1e-08 ... 1.3e-07   (the kernels' LU runs in double)
               Ff, phic, gradc               7.3e-07 ... 1.7e-06   1.1e-07 ... 1.5e-07
               cres                          1.6e-06 ... 1.7e-06   1.5e-07 ... 4.2e-07
               sums, losses                  3.6e-07 ... 9.4e-07   4.4e-08 ... 2.3e-07
               uvp_node, uvp_cell, raw       4.7e-07 ... 7.0e-07   1.1e-07 ... 2.0e-07
    1st order: all stages                    9.2e-08 ... 7.2e-07   6.1e-08 ... 3.1e-07
    phi, node field without smoothing        5.7e-08 ... 1.5e-07   6.9e-08 ... 1.2e-07
    one-hot gdec (c), 2nd order              1.7e-06 ... 8.5e-06   3.8e-07 ... 1.2e-06   (largest: 1 - tanh^2 at the +-60 rows)
    one-hot gdec (c), 1st order              5.4e-07 ... 7.1e-07   4.8e-07 ... 1.2e-06
    per-graph sums / losses (e)              bound 22 ... 62 ulp   <= 1.6 ulp of the float64 sum
    training loss / gloss of the tail (e)    1.9e-05 / 4.5e-06     8.9e-07 / 2.1e-07
"""
import functools
import math

import pytest
import torch

import cases
import fvm_float64 as F

pytestmark = pytest.mark.gpu

MESHES = ("cyl_b3", "cyl_cavity_b2")
SEED_COEF, SEED_DEC = 7, 11
ULP = 2.0 ** -24


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(mesh, order):
    """The mesh with distinct coefficients, its plan on the device, dec and uv_old (float32) - built once per mesh and order."""
    from gfv import plan
    c = _Case()
    c.graphs = F.distinct_coefficients(cases.make_graphs(mesh, order=order), SEED_COEF)
    c.dev_graphs = tuple(g.clone().to("cuda") for g in c.graphs)
    c.plan = plan.build_plan(*c.dev_graphs)
    c.N = c.graphs[0].x.shape[0]
    c.dec, c.uv_old = F.draw_dec(c.N, SEED_DEC), F.uv_old_of(c.graphs)
    c.dec_d, c.uv_old_d = c.dec.cuda(), c.uv_old.cuda()
    if order in ("1st", "2nd"):
        c.G64, c.G32 = F.graph_tensors(c.graphs), F.graph_tensors(c.graphs, torch.float32)
    return c


@functools.lru_cache(maxsize=None)
def _reference(mesh, conserved, integrator, order):
    """float64 stages, and the float32 oracle's own column errors against them (the yardstick)."""
    c = _case(mesh, order)
    ref = F.detached(F.stages(c.dec.double(), c.uv_old.double(), c.G64, conserved, integrator, order))
    o32 = F.detached(F.stages(c.dec, c.uv_old, c.G32, conserved, integrator, order))
    return ref, F.column_errors(o32, ref, c.G64)


@functools.lru_cache(maxsize=None)
def _reference_gradients(mesh, conserved, integrator, order):
    c = _case(mesh, order)
    ref = F.one_hot_gradients(c.dec.double(), c.uv_old.double(), c.G64, conserved, integrator, order)
    o32 = F.one_hot_gradients(c.dec, c.uv_old, c.G32, conserved, integrator, order)
    return ref, F.gradient_errors(o32, ref, c.G64)


def _engine(conserved=True, integrator="imex", order="2nd", fused=True, smooth=True):
    from gfv.engine import Engine
    e = Engine(integrator=integrator, ncn_smooth=smooth, conserved_form=conserved, order=order)
    e._fvm_fuse = fused
    return e


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in d.items() if v is not None}


def _report(title, err, yard):
    fe, fy = F.family_max(err), F.family_max(yard)
    print(title + ": " + ", ".join(f"{k} {fe[k]:.1e} (oracle32 {fy[k]:.1e})" for k in fe))


# ---- a. phi forward and backward at the C ABI -----------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", F.MODES)
def test_phi_kernels_against_the_closed_form(integrator):
    """gfv_phi_fwd / gfv_phi_bwd, N = 300 (one full 256-thread block and a partial one), node types cycling through all six
    values: values, the zero pad column and the gradient - exactly zero at Dirichlet nodes (u, v) and at the PRESS node (p)."""
    from gfv import lib as L
    lib = L.load()
    N, mode = 300, F.MODES.index(integrator)
    g = torch.Generator().manual_seed(31)
    nt = (torch.arange(N) % 6).to(torch.int64)
    y, uvo = torch.randn(N, 2, generator=g), torch.randn(N, 2, generator=g)
    dec, gphi = F.draw_dec(N, 32), torch.randn(N, 8, generator=g)       # (columns 5 .. 7 of gphi must be ignored)
    dd = dec.double().requires_grad_(True)
    ref = F.phi_stage(dd, y.double(), nt, uvo.double(), integrator)
    gref = torch.autograd.grad((ref[:, 0:5] * gphi[:, 0:5].double()).sum(), dd)[0]
    d = lambda t: t.cuda().contiguous()
    nt_d, dec_d, y_d, uvo_d, gphi_d = d(nt.to(torch.int32)), d(dec), d(y), d(uvo), d(gphi)   # (held: the launches are asynchronous)
    phi = torch.full((N + 1, 8), 7.0, device="cuda")                     # one guard row behind the partial block
    L.check(lib.gfv_phi_fwd(dec_d.data_ptr(), y_d.data_ptr(), nt_d.data_ptr(), uvo_d.data_ptr(), phi.data_ptr(), N, mode,
                            L.stream_ptr()), "phi_fwd")
    gdec = torch.full((N + 1, 3), 7.0, device="cuda")
    L.check(lib.gfv_phi_bwd(gphi_d.data_ptr(), dec_d.data_ptr(), nt_d.data_ptr(), gdec.data_ptr(), N, mode, L.stream_ptr()),
            "phi_bwd")
    torch.cuda.synchronize()
    phi, gdec = phi.cpu(), gdec.cpu()
    assert bool((phi[N] == 7.0).all()) and bool((gdec[N] == 7.0).all())
    bound = 8 * ULP
    e = F.col_err(phi[:N], ref.detach())
    eg = F.col_err(gdec[:N], gref)
    print(f"phi {integrator}: values {float(e.max()):.1e}, gradients {float(eg.max()):.1e} (bound {bound:.1e})")
    assert bool((e <= bound).all()), e
    assert bool((phi[:N, 7] == 0).all())
    assert bool((eg <= bound).all()), eg
    dirichlet = (nt == 1) | (nt == 3) | (nt == 4) | (nt == 5)
    assert bool((gdec[:N][dirichlet][:, 0:2] == 0).all()) and bool((gdec[:N][nt == 4][:, 2] == 0).all())
    assert float(gref[~dirichlet][:, 0:2].abs().min()) > 0 and float(gref[nt != 4][:, 2].abs().min()) > 0


# ---- b. forward stages ------------------------------------------------------------------------------------------------------------
def _forward(c, conserved, integrator, order, fused):
    """Every forward output of the section: the saved stages, the losses and the fields for the four values of `smooth`."""
    eng = _engine(conserved, integrator, order, fused)
    losses, uvp_node, uvp_cell, sv = eng.fvm_fwd(c.dec_d, c.uv_old_d, c.plan)
    got = {k: sv[k] for k in ("phi", "grad", "Ff", "phic", "cres", "sums", "gradc")}
    got.update(losses=losses, uvp_node=uvp_node, uvp_cell=uvp_cell)
    raw = eng.fvm_core_fwd(sv["phi"], c.plan, raw_outputs=True)
    got.update(node_raw=raw[1], cell_raw=raw[2])
    plain = _engine(conserved, integrator, order, fused, smooth=False)
    ns = plain.fvm_fwd(c.dec_d, c.uv_old_d, c.plan)
    got["node_nosmooth"] = ns[1]
    got["node_nosmooth_raw"] = plain.fvm_core_fwd(ns[3]["phi"], c.plan, raw_outputs=True)[1]
    return eng, sv, got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("order", ["1st", "2nd"])
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
@pytest.mark.parametrize("mesh", MESHES)
def test_forward_stages(mesh, conserved, order, fused):
    """grad, Ff, phic, cres, gradc, sums, losses and the node / cell fields (smoothed and not, raw and re-dimensionalised) of one
    forward, each column against the float64 stage; the pad columns exactly zero."""
    c = _case(mesh, order)
    ref, yard = _reference(mesh, conserved, "imex", order)
    _, _, got = _forward(c, conserved, "imex", order, fused)
    got = _cpu(got)
    assert ("gradc" in got) == (not conserved)
    for name, cols in (("phi", slice(7, 8)), ("grad", slice(14, 16)), ("Ff", slice(15, 16)), ("phic", slice(7, 8)),
                       ("gradc", slice(10, 16))):
        if name in got:
            assert bool((got[name][:, cols] == 0).all()), name
    err = F.column_errors(got, ref, c.G64)
    assert set(err) == set(ref), set(ref) ^ set(err)
    _report(f"stages {mesh} {'conserved' if conserved else 'non-conserved'} {order} {'fused' if fused else 'unfused'}", err, yard)
    bad = F.failures(err, F.tolerance(yard))
    assert not bad, bad


# ---- c. adjoint, one loss of one graph at a time ----------------------------------------------------------------------------------
ADJOINT_CASES = ([(v, i, "2nd") for v in ("conserved-fused", "conserved-unfused", "non-conserved") for i in F.MODES]
                 + [("conserved-fused", "imex", "1st")])


@pytest.mark.parametrize("variant,integrator,order", ADJOINT_CASES)
@pytest.mark.parametrize("mesh", MESHES)
def test_adjoint_one_loss_of_one_graph_at_a_time(mesh, variant, integrator, order):
    """fvm_bwd with a one-hot gloss [B,4] -> gdec [N,3] against float64 autograd of that one loss, per channel over the rows of
    that graph; rows of the other graphs - and everything, for a loss that does not depend on dec - exactly zero."""
    conserved, fused = variant != "non-conserved", variant != "conserved-unfused"
    c = _case(mesh, order)
    ref, yard = _reference_gradients(mesh, conserved, integrator, order)
    eng = _engine(conserved, integrator, order, fused)
    _, _, _, sv = eng.fvm_fwd(c.dec_d, c.uv_old_d, c.plan, want_outputs=False)
    B = c.plan.B
    got = {}
    for b in range(B):
        for l in range(4):
            gloss = torch.zeros(B, 4, device="cuda")
            gloss[b, l] = 1.0
            got[(b, l)] = eng.fvm_bwd(sv, gloss, c.plan)
    got = _cpu(got)
    for key in set(got) - set(ref):
        assert key[1] == 3 and bool((got[key] == 0).all()), key      # no OUTFLOW face: S3 = 0, guarded
    assert len(ref) >= 4 * B - 1
    err = F.gradient_errors(got, ref, c.G64)
    print(f"adjoint {mesh} {variant} {integrator} {order}: {max(float(e.max()) for e in err.values()):.1e} "
          f"(oracle32 {max(float(e.max()) for e in yard.values()):.1e})")
    bad = F.failures(err, F.tolerance(yard))
    assert not bad, bad


# ---- d. fused against unfused, bit for bit ----------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("integrator,order", [("explicit", "2nd"), ("implicit", "2nd"), ("imex", "1st"), ("imex", "3rd"),
                                              ("imex", "4th")])
def test_fused_launches_equal_the_unfused_ones_bit_for_bit(integrator, order):
    """The forward tail as one launch and the backward as three against the launches they replace, conserved form, where no other
    test looks: integrators explicit / implicit and the reconstruction orders 1st / 3rd / 4th - every forward output and gdec,
    compared as bit patterns (identity does not depend on the conditioning of the 3rd / 4th-order systems)."""
    c = _case("cyl_b3", order)
    gloss = (0.5 + torch.rand(c.plan.B, 4, generator=torch.Generator().manual_seed(41))).cuda()
    res = {}
    for fused in (True, False):
        eng, sv, got = _forward(c, True, integrator, order, fused)
        got["gdec"] = eng.fvm_bwd(sv, gloss, c.plan)
        res[fused] = _cpu(got)
    assert res[True].keys() == res[False].keys() and "gdec" in res[True] and "sums" in res[True]
    for k in res[True]:
        assert torch.equal(_bits(res[True][k]), _bits(res[False][k])), k
    if order in ("1st", "2nd"):
        assert float(res[True]["gdec"].abs().max()) > 0 and bool(torch.isfinite(res[True]["gdec"]).all())


# ---- e. per-graph norms at the loop boundaries, at the C ABI ---------------------------------------------------------------------
NORM_SIZES = [0, 1, 1023, 1024, 1025, 7168, 7169, 8191, 8192, 8193, 8192 + 3 * 1024 + 5, 20000]


def _norm_batch():
    g = torch.Generator().manual_seed(51)
    B, total = len(NORM_SIZES), sum(NORM_SIZES)
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor(NORM_SIZES).cumsum(0)
    scale = torch.repeat_interleave(0.5 + torch.arange(B, dtype=torch.float32), torch.tensor(NORM_SIZES))
    cres = torch.randn(total, 4, generator=g) * scale[:, None]
    cres[:, 3] = cres[:, 3] ** 2                                          # lp2 is a sum of squares already
    theta = 0.5 + torch.rand(B, 9, generator=g)
    sigma = 0.5 + torch.rand(B, 3, generator=g)
    return cres, ptr.to(torch.int32), theta, sigma


def _tail_mesh(L, B, C_, ptr, theta, sigma):
    m = L.FvmMesh(N=0, E=0, C=C_, B=B, terms=5, mode=2, smooth=0, reserved=0)
    m.gcell_ptr, m.theta, m.sigma = ptr.data_ptr(), theta.data_ptr(), sigma.data_ptr()
    return m


def test_graph_norms_at_the_loop_boundaries():
    """gfv_graph_loss and gfv_fvm_fwd_tail on graphs of 0 ... 20 000 cells in one batch: below, at and above one 1024-cell stride
    and the 8 x 1024 unrolled trip (entered from 7169 cells on), two trips and a remainder.  Sums within 2 (ceil(n / 1024) + 11)
    2^-24 of the float64 sum (n / 1024 additions per thread, 10 levels of the tree, one squaring; doubled), losses one rounding
    more; the two entry points bit for bit; the empty graph exactly zero; the training loss and its gradient of the tail launch
    against float64, its arrival counter back at zero after every launch."""
    from gfv import lib as L
    lib = L.load()
    cres, ptr, theta, sigma = _norm_batch()
    B, total = len(NORM_SIZES), sum(NORM_SIZES)
    assert int(ptr[-1]) == total == cres.shape[0]
    rsums, rlosses = F.graph_norms(cres, ptr, theta, sigma)
    cres_d, ptr_d, theta_d, sigma_d = cres.cuda(), ptr.cuda(), theta.cuda(), sigma.cuda()
    st = L.stream_ptr()
    sums, losses = torch.full((B, 4), -1.0, device="cuda"), torch.full((B, 4), -1.0, device="cuda")
    L.check(lib.gfv_graph_loss(cres_d.data_ptr(), ptr_d.data_ptr(), theta_d.data_ptr(), sigma_d.data_ptr(), sums.data_ptr(),
                               losses.data_ptr(), B, st), "graph_loss")
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    sums_t, losses_t = torch.full((B, 4), -1.0, device="cuda"), torch.full((B, 4), -1.0, device="cuda")
    mesh = _tail_mesh(L, B, total, ptr_d, theta_d, sigma_d)
    L.check(lib.gfv_fvm_fwd_tail(mesh, cres_d.data_ptr(), None, None, sums_t.data_ptr(), losses_t.data_ptr(), None, None, None,
                                 None, counter.data_ptr(), st), "fvm_fwd_tail")
    torch.cuda.synchronize()
    assert int(counter[0]) == 0
    assert torch.equal(_bits(sums), _bits(sums_t)) and torch.equal(_bits(losses), _bits(losses_t))
    sums, losses = sums.cpu().double(), losses.cpu().double()
    assert bool((sums[0] == 0).all()) and bool((losses[0] == 0).all())                  # the empty graph
    n = torch.tensor(NORM_SIZES, dtype=torch.float64)
    bound = (2 * (torch.ceil(n / 1024) + 11) * ULP)[:, None]
    es, el = (sums - rsums).abs() / rsums.clamp(min=1e-300), (losses - rlosses).abs() / rlosses.clamp(min=1e-300)
    print("graph norms: sums", (es / ULP).amax(1).tolist(), "ulp; losses", (el / ULP).amax(1).tolist(), "ulp; bound",
          (bound[:, 0] / ULP).tolist())
    assert bool((rsums[1:] > 0).all())
    assert bool((es <= bound).all()), es / bound
    assert bool((el <= bound + ULP).all()), el / (bound + ULP)

    # the training loss behind the norms, on the batch without the empty graph (log 0 otherwise), twice in a row
    B1 = B - 1
    ptr1, theta1, sigma1 = ptr_d[1:].contiguous(), theta_d[1:].contiguous(), sigma_d[1:].contiguous()
    assert int(ptr1[0]) == 0
    mesh1 = _tail_mesh(L, B1, total, ptr1, theta1, sigma1)
    wc, wm, wp = 6e4, 5e4, 1.0
    hyper = torch.tensor([0, 0, 0, 0, 0, wc, wm, wp], dtype=torch.float32, device="cuda")
    w = torch.tensor([wc, wm, wm, wp], dtype=torch.float64)
    tot = (rlosses[1:] * w).sum(1)
    rloss, rgloss = tot.log().mean(), w[None, :] / (tot[:, None] * B1)
    bl = float((bound[1:] + ULP).max())
    tol_loss = bl + 8 * ULP + (B1 + 3) * ULP * float(tot.log().abs().mean())
    tol_gloss = bl + 12 * ULP
    for _ in range(2):
        s1, l1 = torch.full((B1, 4), -1.0, device="cuda"), torch.full((B1, 4), -1.0, device="cuda")
        loss, gloss = torch.full((1,), -1.0, device="cuda"), torch.full((B1, 4), -1.0, device="cuda")
        L.check(lib.gfv_fvm_fwd_tail(mesh1, cres_d.data_ptr(), None, None, s1.data_ptr(), l1.data_ptr(), None, hyper.data_ptr(),
                                     loss.data_ptr(), gloss.data_ptr(), counter.data_ptr(), st), "fvm_fwd_tail")
        torch.cuda.synchronize()
        assert int(counter[0]) == 0
        assert torch.equal(_bits(s1), _bits(sums_t[1:])) and torch.equal(_bits(l1), _bits(losses_t[1:]))
        e_loss = abs(float(loss) - float(rloss))
        e_gloss = float(((gloss.cpu().double() - rgloss).abs() / rgloss).max())
        print(f"tail: loss {e_loss:.1e} (tolerance {tol_loss:.1e}), gloss {e_gloss:.1e} (tolerance {tol_gloss:.1e})")
        assert e_loss <= tol_loss and e_gloss <= tol_gloss


def test_backward_of_a_graph_with_zero_residuals_is_zero_and_finite():
    """gfv_fvm_bwd_ex where one graph's cres is all zero (S = 0: the `S > 0` guards): finite everywhere, the per-cell loss
    gradients gc of that graph exactly zero."""
    from gfv import lib as L
    lib = L.load()
    c = _case("cyl_b3", "2nd")
    pl = c.plan
    eng = _engine(fused=False)
    _, _, _, sv = eng.fvm_fwd(c.dec_d, c.uv_old_d, pl, want_outputs=False)
    lo, hi = int(pl.gcell_ptr[1]), int(pl.gcell_ptr[2])
    cres = sv["cres"].clone()
    cres[lo:hi] = 0.0
    st = L.stream_ptr()
    N, E, Cn, B = pl.N, pl.E, pl.C, pl.B
    sums, losses = torch.empty(B, 4, device="cuda"), torch.empty(B, 4, device="cuda")
    L.check(lib.gfv_graph_loss(cres.data_ptr(), pl.gcell_ptr.data_ptr(), pl.theta.data_ptr(), pl.sigma.data_ptr(), sums.data_ptr(),
                               losses.data_ptr(), B, st), "graph_loss")
    gloss = torch.ones(B, 4, device="cuda")
    nan = float("nan")
    gc, gFf = torch.full((Cn, 4), nan, device="cuda"), torch.full((E, 16), nan, device="cuda")
    gphi, ggrad = torch.full((N, 8), nan, device="cuda"), torch.full((N, 16), nan, device="cuda")
    L.check(lib.gfv_fvm_bwd_ex(cres.data_ptr(), sums.data_ptr(), gloss.data_ptr(), sv["Ff"].data_ptr(), pl.cbatch.data_ptr(),
                               pl.theta.data_ptr(), pl.sigma.data_ptr(), pl.dt.data_ptr(), pl.frow.data_ptr(), pl.fk.data_ptr(),
                               pl.kcell.data_ptr(), pl.kS.data_ptr(), pl.ftype.data_ptr(), pl.n_rowptr.data_ptr(),
                               pl.n_col_edge2.data_ptr(), pl.nrow.data_ptr(), pl.ncell.data_ptr(), pl.crow.data_ptr(),
                               pl.pos.data_ptr(), pl.fpos.data_ptr(), pl.centroid.data_ptr(), pl.area.data_ptr(), gc.data_ptr(),
                               gFf.data_ptr(), gphi.data_ptr(), ggrad.data_ptr(), N, E, Cn, 0, None, None, st), "fvm_bwd")
    torch.cuda.synchronize()
    assert bool((sums[1] == 0).all()) and bool((sums[0] > 0).all()) and bool((sums[2] > 0).all())
    for t in (gc, gFf, gphi, ggrad):
        assert bool(torch.isfinite(t).all())
    assert bool((gc[lo:hi] == 0).all())
    assert float(gc[:lo].abs().max()) > 0 and float(gc[hi:].abs().max()) > 0
    assert math.isfinite(float(gphi.abs().max())) and float(gphi.abs().max()) > 0
