"""GPU: the MLP backward chains judged ROW BY ROW against float64 autograd (tests/chain_rows.py): the small-tile kernel
(csrc/cbwd.hip, one fragment scale per 32 rows), the column-owner persistent kernel (csrc/colchain_kernel.h, one per 64 rows, in
its read and recompute forms) with one tile per workgroup, with two to three, and - in a fresh child process with 3 and 8
workgroups - with 5 to 14; the row-owner chain (per-row scales) as control; the Transolver backward.  Row layouts put different
scales into neighbouring tiles (the accumulator rescale), ratios 2^0 ... 2^-20 into every tile (`mixed`), 2^-40 behind a cliff
(the scale cap) and all-zero tiles into the walk.  Interior rows keep 1e-5; the others 1e-5 + the quantisation floor of the scale
the kernel reports.  `ROWACC family shape layout exponent e_max` lines record the measured accuracy ("Per-row accuracy
of the backward chains")."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_rows as R  # noqa: E402

pytestmark = pytest.mark.gpu

M = 1317      # a ragged last tile (5 rows: a last group of 5) for both tile sizes, 6.86 layout regions


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from gfv import lib
    lib.load()
    return torch.device("cuda:0")


def _run(impl, shape, layout, M, flat=False):
    c = R.case(shape, M)
    out = impl.run(c, layout)
    L = R.checks(c, layout, out, flat=flat)
    if layout in ("mixed", "cliff_down"):
        print("\n".join(R.rowacc(impl.name, c, layout, out)))
    return L


def _all_pass(L):
    print(R.report(L))
    assert not R.failed(L), R.report(R.failed(L))


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("rows", [M, 33])
def test_small_tile_backward_row_by_row(dev, shape, rows):
    """csrc/cbwd.hip: input gradient(s), gz1, gz2 and g3 row by row, the weight gradients through the weight-gradient launch
    with the scales the chain wrote."""
    impl, L = R.Gpu("cbwd"), []
    for layout in R.LAYOUTS:
        L += _run(impl, shape, layout, rows)
    _all_pass(L)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("form", ["col_read", "col_rc"])
def test_column_owner_backward_row_by_row_one_tile_per_workgroup(dev, shape, form):
    """csrc/colchain_kernel.h at 21 workgroups of one tile each: input gradient(s) and gz1 row by row, the fused weight-gradient
    blocks summed, the first Linear's through the weight-gradient launch."""
    from gfv import lib as L_
    assert L_.load().gfv_rowtile_dw_partials_m(M) == (M + 63) // 64
    impl, L = R.Gpu(form), []
    for layout in R.LAYOUTS:
        L += _run(impl, shape, layout, M)
    _all_pass(L)


@pytest.mark.parametrize("form", ["col_read", "col_rc"])
def test_column_owner_backward_two_to_three_tiles_per_workgroup(dev, form):
    """The same kernel on its real grid, every workgroup walking two to three tiles: neighbouring tiles of different scales
    (the accumulator rescale: a wrong ratio is an O(1) error in dW3 / dW2), falling stairs, and all-zero tiles at the head, in
    the middle and at the tail of a walk."""
    from gfv import lib as L_
    rows = 2 * 64 * L_.load().gfv_rowtile_dw_partials() + 37
    assert L_.load().gfv_rowtile_dw_partials_m(rows) == L_.load().gfv_rowtile_dw_partials()
    impl, L = R.Gpu(form), []
    for layout in ("zigzag", "stairs_down", "zeros"):
        L += _run(impl, "edge", layout, rows)
    _all_pass(L)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_row_owner_chain_is_flat_on_every_row(dev, shape):
    """Control: the row-owner chain scales every row by itself - every non-zero row of every layout at 1e-5, the rows at 2^-20
    of their neighbours and those behind the cliff included."""
    impl, L = R.Gpu("row"), []
    for layout in R.LAYOUTS:
        L += _run(impl, shape, layout, M, flat=True)
    _all_pass(L)


@pytest.mark.parametrize("n", [3, 8])
def test_deep_walks_in_a_child_process(n):
    """GFV_COLCHAIN_WGS = 3 / 8 (read once per process: a fresh interpreter): 14 / 5 tiles per workgroup at M = 2597, tile starts
    off 64-row alignment, the identity / the permuted workgroup order; the same checks, by name, as the list built on fp32
    autograd.  At 3 workgroups the middle one straddles the cliff of `cliff_down`: its groups behind the cliff report capped g3
    scales, the last workgroup's uncapped ones."""
    import chain_rows_worker as W
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chain_rows_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GFV_COLCHAIN_WGS=str(n)))
    tail = r.stdout[-6000:] + r.stderr[-4000:]
    assert r.returncode == 0, tail
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("ROWACC", "ROWCLIFF"))))
    lines = re.findall(r"^ROWCHECK (\S+) ([01]) (\S+) (\S+)$", r.stdout, re.M)
    done = re.search(r"^ROWDONE (\d+)$", r.stdout, re.M)
    assert done and int(done.group(1)) == len(lines), tail
    want = []
    for fam in W.FAMILIES:
        for shape, layout in W.plan(R):
            c = R.case(shape, W.M)
            want += [f"{fam}/{k.name}" for k in R.checks(c, layout, R.Torch32().run(c, layout), names=R.ROWS_COL[shape])]
    assert [l[0] for l in lines] == want, tail
    assert all(l[1] == "1" for l in lines), "\n".join(" ".join(l) for l in lines if l[1] != "1") + "\n\n" + tail
    cliff = re.findall(r"^ROWCLIFF (\S+) (\S+)$", r.stdout, re.M)
    assert [f for f, _ in cliff] == list(W.FAMILIES), tail
    if n == 3:
        assert all(float(v) >= 10 for _, v in cliff), cliff      # capped and uncapped groups: otherwise move the cliff


# ---- the Transolver backward (gfv_trans_mlp_bwd) -----------------------------------------------------------------------------------
TRANS_FLAT = ("flat", "zigzag", "stairs_down", "stairs_up", "cliff_up", "zeros")


@pytest.mark.parametrize("small", [1, 0])
def test_transolver_backward_row_by_row(dev, small, gfv_limits):
    """g_z, g_fx1 and g_out_x of one launch row by row: 1e-5 on every interior row of the layouts without a small row inside a
    tile, zero rows exactly zero.  Its g_z fragments carry one scale per tile, which the launch does not report: on `mixed` only
    finiteness and the global tolerance are asserted and the row errors printed."""
    from gfv import lib as L_, ops
    gfv_limits(GFV_CTRANS=small)
    g = torch.Generator().manual_seed(17)
    s = lambda *sh: torch.randn(*sh, generator=g)
    P = {"Wout": s(128, 128) * 0.09, "bout": s(128) * 0.1, "gamma": 1 + 0.1 * s(128), "beta": 0.1 * s(128),
         "Wpre": s(256, 128) * 0.09, "bpre": s(256) * 0.1, "Wpost": s(128, 256) * 0.06, "bpost": s(128) * 0.1}
    x, res, go0, ga0 = s(M, 128), s(M, 128), s(M, 128), s(M, 128) * 0.1
    Pg = {k: v.double() for k, v in P.items()}
    xg = x.double().requires_grad_(True)
    fx1 = xg @ Pg["Wout"].T + Pg["bout"] + res.double()
    fx1.retain_grad()
    z = F.layer_norm(fx1, (128,), Pg["gamma"], Pg["beta"], 1e-5) @ Pg["Wpre"].T + Pg["bpre"]
    out = F.gelu(z) @ Pg["Wpost"].T + Pg["bpost"] + fx1
    d = lambda t: t.to(dev).contiguous()
    Pd = {k: d(v) for k, v in P.items()}
    wi = ops.WeightImages(dev, torch.stack([v.abs().max() for k, v in P.items() if k.startswith("W")]).max().reshape(1).to(dev))
    wi.static = [(0, 1 << 62)]
    prev = ops.set_weight_images(wi)
    try:
        Wpost_t, Wpre_t, Wout_t = ops.transpose(Pd["Wpost"]), ops.transpose(Pd["Wpre"]), ops.transpose(Pd["Wout"])
        zd, f1d = d(z.detach().float()), d(fx1.detach().float())
        for layout in R.LAYOUTS:
            m = R.multipliers(layout, M)[:, None]
            go, ga = (go0.double() * m).float(), (ga0.double() * m).float()
            gtot = go.double() + ga.double()
            ref = dict(zip(("g_z", "g_fx1", "g_out_x"), torch.autograd.grad(out, [z, fx1, xg], grad_outputs=gtot, retain_graph=True)))
            new = lambda *sh: torch.full(sh, float("nan"), device=dev)
            got = {"g_z": new(M, 256), "g_fx1": new(M, 128), "g_out_x": new(M, 128)}
            gsum, part = new(M, 128), new(ops.ln_rows(M), 2, 128)
            gs = torch.zeros(3, ops.gscale_ld(M), device=dev)
            assert ops.trans_mlp_bwd(d(go), d(ga), gsum, zd, f1d, Wpost_t, Wpre_t, Wout_t, Pd["gamma"], got["g_z"], got["g_fx1"],
                                     got["g_out_x"], part, gs[0])
            torch.cuda.synchronize()
            nfill = L_.load().gfv_trans_mlp_ln_rows(M)
            assert bool(torch.isfinite(part[:nfill]).all()) and bool(torch.isfinite(gs).all())
            mult = m[:, 0]
            nz, easy = mult != 0, R.interior(mult) & (mult != 0)
            fam = "ctrans" if small else "transmlp"
            for name, t in got.items():
                assert bool(torch.isfinite(t).all()), (layout, name)
                e = R.row_err(t, ref[name])
                assert R.rel(t, ref[name]) < R.TOL_ROW, (layout, name, R.rel(t, ref[name]))
                assert not bool((t.cpu()[~nz] != 0).any()), (layout, name, "zero rows")
                rest = nz & ~easy
                print(f"TRANSROWS {fam} {layout} {name} interior {float(e[easy].max()) if bool(easy.any()) else 0.0:.2e} "
                      f"other {float(e[rest].max()) if bool(rest.any()) else 0.0:.2e}")
                if layout in TRANS_FLAT:
                    assert float(e[easy].max()) < R.TOL_ROW, (layout, name, float(e[easy].max()))
                if layout in ("mixed", "cliff_down") and name == "g_out_x":
                    print("\n".join(R.rowacc_lines(fam, "trans", layout, e)))
            flags = L_.C.c_int32(0)
            L_.check(L_.load().gfv_status_flags(L_.C.byref(flags)), "gfv_status_flags")
            assert flags.value == 0, layout
    finally:
        ops.set_weight_images(prev)
