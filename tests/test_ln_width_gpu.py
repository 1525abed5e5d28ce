"""GPU: every kernel that takes LayerNorm statistics, at hidden 16 / 32 / 64 / 112 / 128 in both padded layouts, against the float64
statements of tests/ln_width.py, with LayerNorm input rows whose |mean| / std is 0, 8 and 32 and exact zeros inside real columns.
M = 197 rows: 3 tiles of 64 + 5, 6 tiles of 32 + 5, one 128-row block + 69 (csrc/lin1.hip, which takes no launch below 1024 rows:
1221 = 9 blocks + the same 69).

Sites (each pinned, and the path code / partial-row count asserted so that a test runs the kernel it names):
  row-owner chain (csrc/tchain_kernel.h)  GFV_FIN_LN with fin_presave + fin_stats, GFV_IN_LN, GFV_IN_LNBWD (statistics recomputed
                                          from in_aux), GFV_FIN_LNBWD                                  family = CHAIN_ROW_OWNER
  csrc/cfwd.hip                           GFV_FIN_LN (per-wave partials, combined)                     GFV_CFWD = 1
  csrc/cbwd.hip                           GFV_IN_LNBWD reading in_stats = the forward launch's own fin_stats   GFV_CBWD = 1
  csrc/lin1s.hip, csrc/lin1.hip           LayerNorm prologue, LayerNorm-backward epilogue              GFV_LIN1S = 1 / 0
  csrc/ctrans.hip, csrc/transmlp.hip      gfv_trans_mlp_fwd (ln_2 inside), gfv_trans_mlp_bwd            GFV_CTRANS = 1 / 0
  gfv_seg_gather_sum_ln                   fed the forward launch's y3 and fin_stats
(csrc/dw.hip's LayerNorm on load: tests/test_dw_float64_gpu.py.)

Asserted everywhere: outputs and input gradients row by row, (mean, 1 / std) where a launch exposes them, dgamma / dbeta on the real
columns, the padded columns of every forward output and of every gradient that has passed a padded weight exactly zero, status
word 0, two runs bit-equal.  (The LayerNorm-backward result itself - in_save of GFV_IN_LNBWD, the output of GFV_FIN_LNBWD, g_fx1 -
holds rstd (0 - m1 - xhat_pad m2) in its padded columns by design; the weight rows that meet them are zero.  Those tensors are
judged on the real columns, and `test_padded_columns_of_the_layernorm_backward_do_not_reach_the_weight_gradient` shows that the
group scales they may set do not cost dW3 / db3 their accuracy.)  Every run prints `LNW site h layout offset e_max limit`; the
largest figures measured per site are in DESIGN.md 5w (offset 32: 1.8e-6 .. 1.2e-5 against limits of 1.0e-5 .. 3.4e-5)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_rows as CR  # noqa: E402
import ln_width as W  # noqa: E402

pytestmark = pytest.mark.gpu

PIN = {"cfwd_fin_ln": dict(GFV_CFWD=1), "cbwd_in_lnbwd": dict(GFV_CBWD=1, GFV_CFWD=1), "lin1s_in_ln": dict(GFV_LIN1S=1),
       "lin1_in_ln": dict(GFV_LIN1S=0), "lin1s_fin_lnbwd": dict(GFV_LIN1S=1), "lin1_fin_lnbwd": dict(GFV_LIN1S=0),
       "ctrans": dict(GFV_CTRANS=1), "transmlp": dict(GFV_CTRANS=0)}
PATH = {"row": 5, "cfwd": 5 + 64, "cbwd": 5 + 128, "lin1s": 5 + 32, "lin1": 5 + 32}
MEAN_TOL = 1e-6       # the mean against float64 of the launch's own rows, relative to the largest: one sum and one product
# (1 / std goes into every output of its row as a factor: its limit is the row limit of the case's LayerNorm output)


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from gfv import lib
    lib.load()
    return torch.device("cuda:0")


def _after(gpu, p, got, checks, names_zero=None):
    print(W.lnw_line(gpu.site, p, checks))
    bad = W.failed(checks)
    assert not bad, W.report(bad)
    for n in (gpu.pad_zero if names_zero is None else names_zero):
        assert W.padding_is_zero(got[n], p.real), (gpu.site, p.tag, n, "padded columns not exactly zero")
    assert gpu.status == 0, (gpu.site, p.tag, gpu.status)
    assert gpu.bit_equal, (gpu.site, p.tag, "two runs differ")
    fam = gpu.site.split("_")[0]
    if fam in PATH:
        assert gpu.path == PATH[fam], (gpu.site, gpu.path)


def _stats_checks(p, got):
    """(mean, 1 / std) the launch wrote against float64 statistics of the rows the same launch wrote (fin_presave)."""
    mean, rstd = W.stats64(got["y3"], p.real)
    em, er = CR.rel(got["stats"][:, 0:1], mean), float(((got["stats"][:, 1:2].double() - rstd).abs() / rstd).max())
    return [(f"{p.tag}/mean", em, MEAN_TOL, em <= MEAN_TOL), (f"{p.tag}/rstd", er, W.limit(p, "out"), er <= W.limit(p, "out"))]


def _rows(site):
    """M = 197 everywhere but on csrc/lin1.hip, which leaves launches below 1024 rows to the other families."""
    return W.M_LIN1 if site.startswith("lin1_") else W.M


def _cases(h):
    return [(lay, off) for lay in W.LAYOUTS for off in W.OFFSETS]


@pytest.mark.parametrize("h", W.WIDTHS)
@pytest.mark.parametrize("site", ["row_fin_ln", "cfwd_fin_ln"])
def test_final_layernorm_of_the_mlp(site, h, gfv_limits):
    gfv_limits(**PIN.get(site, {}))
    for kind in ("mlp", "mlp_dense"):
        for lay, off in _cases(h):
            p, gpu = W.problem(kind, h, lay, off), W.Gpu(site)
            got = gpu.run(p)
            _after(gpu, p, got, W.judge(p, got, names=("y3", "out")) + _stats_checks(p, got))


@pytest.mark.parametrize("h", W.WIDTHS)
@pytest.mark.parametrize("site", ["row_in_ln", "lin1s_in_ln", "lin1_in_ln"])
def test_layernorm_prologue(site, h, gfv_limits):
    gfv_limits(**PIN.get(site, {}))
    for lay, off in _cases(h):
        p, gpu = W.problem("fwd", h, lay, off, _rows(site)), W.Gpu(site)
        got = gpu.run(p)
        _after(gpu, p, got, W.judge(p, got, names=("out",)))


@pytest.mark.parametrize("h", W.WIDTHS)
def test_layernorm_backward_prologue_recomputing_the_statistics(h):
    for lay, off in _cases(h):
        p, gpu = W.problem("bwd", h, lay, off), W.Gpu("row_in_lnbwd")
        got = gpu.run(p)
        _after(gpu, p, got, W.judge(p, got, names=("g3", "ge", "gamma_in", "beta_in")))


@pytest.mark.parametrize("h", W.WIDTHS)
def test_small_tile_backward_on_the_forward_launch_statistics(h, gfv_limits):
    """cfwd.hip writes y3 and (mean, 1 / std); cbwd.hip reads both: the backward of those rows against float64 of those rows."""
    gfv_limits(**PIN["cbwd_in_lnbwd"])
    for kind in ("mlp", "mlp_dense"):
        for lay, off in _cases(h):
            fwd = W.Gpu("cfwd_fin_ln")
            f = fwd.run(W.problem(kind, h, lay, off))
            assert fwd.path == PATH["cfwd"]
            q = W.problem("bwd", h, lay, off).with_rows(f["y3"])
            gpu = W.Gpu("cbwd_in_lnbwd")
            got = gpu.run(q, stats=f["stats"].cuda().contiguous())
            assert gpu.last["ln_rows"] == (W.M + 31) // 32
            _after(gpu, q, got, W.judge(q, got, names=("g3", "ge", "gamma_in", "beta_in")))


@pytest.mark.parametrize("h", W.WIDTHS)
@pytest.mark.parametrize("site", ["row_fin_lnbwd", "lin1s_fin_lnbwd", "lin1_fin_lnbwd"])
def test_layernorm_backward_epilogue(site, h, gfv_limits):
    gfv_limits(**PIN.get(site, {}))
    for lay, off in _cases(h):
        p, gpu = W.problem("bwd", h, lay, off, _rows(site)), W.Gpu(site)
        got = gpu.run(p)
        _after(gpu, p, got, W.judge(p, got, names=("gx", "gamma", "beta")))


@pytest.mark.parametrize("h", W.WIDTHS)
@pytest.mark.parametrize("site", ["ctrans", "transmlp"])
def test_transolver_chain(site, h, gfv_limits):
    from gfv import ops
    gfv_limits(**PIN[site])
    for lay, off in _cases(h):
        p, gpu = W.problem("trans", h, lay, off), W.Gpu(site)
        got = gpu.run(p)
        assert gpu.ln_rows == ((W.M + 31) // 32 if site == "ctrans" else ops.rowtile_tiles(W.M)), (site, gpu.ln_rows)
        _after(gpu, p, got, W.judge(p, got, names=p.rows + p.sums))


@pytest.mark.parametrize("h,lay", [(32, "edge"), (16, "edge")])
def test_seg_gather_sum_of_the_layernorm(h, lay, gfv_limits):
    """gfv_seg_gather_sum_ln normalises y3 half-rows with the statistics the forward launch saved: fed the fixed forward's y3 and
    fin_stats at offset 32, against float64 LayerNorm of those rows."""
    from gfv import ops
    gfv_limits(**PIN["cfwd_fin_ln"])
    p = W.problem("mlp_dense", h, lay, 32)
    f = W.Gpu("cfwd_fin_ln").run(p)
    g = torch.Generator().manual_seed(h)
    n_rows, per = 50, 4
    col = torch.randint(0, 2 * W.M, (n_rows * per,), generator=g)
    rowptr = torch.arange(0, n_rows * per + 1, per)
    ln = W.ln64(f["y3"], p.gamma, p.beta, p.real)                    # float64 of the launch's own rows
    halves = ln.view(W.M * 2, 64)
    ref = halves[col].view(n_rows, per, 64).sum(1)
    out = ops.seg_gather_sum_ln(f["y3"].cuda(), f["stats"].cuda().contiguous(), p.gamma.cuda(), p.beta.cuda(), rowptr.int().cuda(),
                                col.int().cuda(), n_rows)
    torch.cuda.synchronize()
    e, lim = float(CR.row_err(out, ref).max()), W.limit(p, "out")
    print(f"LNW seg_gather_sum_ln {h} {lay} 32 {e:.2e} {lim:.2e}")
    assert e <= lim, (e, lim)
    assert bool((out.cpu()[:, ~p.real[:64]] == 0).all())      # (edge layout: both halves of a row hold the same real columns)


@pytest.mark.parametrize("h", [16, 32])
def test_padded_columns_of_the_layernorm_backward_do_not_reach_the_weight_gradient(h):
    """ln_bwd leaves rstd (0 - m1 - xhat_pad m2) in the padded columns of g3; with an offset xhat_pad is about -offset, so these
    entries can exceed the real ones and set the group scale the weight-gradient launch is handed.  dW3 / db3 on the real entries,
    through that launch with the scales the chain reported, against float64 (chain_rows.TOL_SUM)."""
    from gfv import ops
    for lay in W.LAYOUTS:
        p, gpu = W.problem("bwd", h, lay, 32), W.Gpu("row_in_lnbwd")
        gpu.run(p)
        a2 = F.gelu(p.z2.double())
        dW, db = ops.linear_dw(gpu.last["g3"], 128, [ops.Seg(a2.float().cuda().contiguous())], W.M, gscale=gpu.last["gs"][0])
        torch.cuda.synchronize()
        g3 = p.ref()["g3"]
        refW, refb = g3.T @ a2.float().double(), g3.sum(0)
        r = p.real
        eW, eb = CR.rel(dW.cpu()[r][:, r], refW[r][:, r]), CR.rel(db.cpu()[r], refb[r])
        pad_over_real = float(gpu.last["g3"].cpu()[:, ~r].abs().max() / gpu.last["g3"].cpu()[:, r].abs().max())
        print(f"LNW dW3 {h} {lay} 32 dW {eW:.2e} db {eb:.2e} limit {CR.TOL_SUM:.0e} (padded / real entries of g3: {pad_over_real:.1f})")
        assert eW < CR.TOL_SUM and eb < CR.TOL_SUM, (eW, eb)
