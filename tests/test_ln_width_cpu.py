"""CPU: the float64 statement of LayerNorm at hidden < 128 (tests/ln_width.py) is sound before the GPU tests lean on it.

* float32 eager torch over the h real columns - the reference implementation's arithmetic - keeps a quarter of every limit on every
  case, so the limits are not vacuous;
* the kernels' rule in float32 (`Emu()`: non-zero entries + counted zeros) passes every case;
* the parent revision's rule (`Emu(old=True)`: sum over all 128 columns, npad mean^2 taken out again) fails where the cancellation
  bites and passes at offset 0 and at h = 128, where it is the same arithmetic;
* the exact zeros inside real columns separate a correct zero count from "every zero is padding", and the other mutations of the
  rule (1 / 128 at a narrow width, edge layout taken for node layout) fail too.

Figures (largest value / limit over the outputs of a case, M = 197 rows; `test_old_rule_fails_where_the_subtraction_cancels` prints
them as LNW-EMU lines): Emu() stays at 0.02 .. 0.55 of the limit on every case; Emu(old=True) on the directly fed cases reaches
4.2 .. 71 (h = 16), 1.7 .. 44 (h = 32) and 2.9 .. 9.6 (h = 64, offset 32) of it, 109 / 233 on the MLP without a zero column."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_rows as CR  # noqa: E402
import ln_width as W  # noqa: E402

KINDS = ("fwd", "bwd", "mlp", "mlp_dense", "trans")


# Where the parent's rule is expected to leave the limit: offsets 8 and 32 at h = 16 / 32 / 64 - but for two groups of cases whose
# loss stays below the limit on 197 rows, by the estimate (mean / std)^2 (128 - h) / h ulps of var, half of it in the output:
#   * offset 8 at h = 64: 64 ulps of var = 3.8e-6, 1.9e-6 in rstd (measured: 0.46 - 0.75 of the limit);
#   * the MLP whose y3 has an exactly-zero real column: that column holds |mean| / std at about h / sqrt(h - 1) = 4.1 / 5.7 / 8.1
#     for h = 16 / 32 / 64 whatever the offset (measured: 0.30 - 1.17 of the limit).  The same MLP without the zero column
#     ("mlp_dense") is where the final LayerNorm of the 3-layer chain meets the offsets.
NOT_BEYOND = {(k, 64, 8) for k in KINDS} | {("mlp", h, off) for h in (16, 32, 64) for off in (8, 32)}


def _worst(checks):
    return max(c[1] / c[2] for c in checks)


@pytest.mark.parametrize("kind", KINDS)
def test_float32_torch_keeps_a_quarter_of_every_limit(kind):
    bad = []
    for h, lay, off in W.cases():
        p = W.problem(kind, h, lay, off)
        bad += W.failed(W.judge(p, W.Torch32().run(p), margin=0.25))
    assert not bad, W.report(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_new_rule_passes_every_case(kind):
    bad = []
    for h, lay, off in W.cases():
        p = W.problem(kind, h, lay, off)
        got = W.Emu().run(p)
        bad += W.failed(W.judge(p, got))
        for n in ("out", "ln"):
            if n in got and got[n].shape[1] == 128:
                assert W.padding_is_zero(got[n], p.real), (p.tag, n)
    assert not bad, W.report(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_old_rule_fails_where_the_subtraction_cancels(kind):
    lines, wrong = [], []
    for h, lay, off in W.cases():
        p = W.problem(kind, h, lay, off)
        new, old = _worst(W.judge(p, W.Emu().run(p))), _worst(W.judge(p, W.Emu(old=True).run(p)))
        lines.append(f"LNW-EMU {kind} {h} {lay} {off} new {new:.2f} old {old:.2f} (of the limit)")
        if off in (8, 32) and h in (16, 32, 64) and (kind, h, off) not in NOT_BEYOND:
            if old < 1.0:
                wrong.append(lines[-1] + "  <- the old rule should fail here")
        elif off in (8, 32) and h in (16, 32, 64):
            if not new < old:
                wrong.append(lines[-1] + "  <- the old rule should at least be worse here")
        elif off == 0 or h == 128:
            if old >= 1.0:
                wrong.append(lines[-1] + "  <- the old rule should pass here")
    print("\n".join(lines))
    assert not wrong, "\n".join(wrong)


def test_old_rule_at_128_is_the_new_rule():
    g = torch.Generator().manual_seed(5)
    x = W.direct_rows(g, 128, "node", 32)
    a, b = W.stats32(x, 128, "node", "new"), W.stats32(x, 128, "node", "old")
    # (the float64 statement of both: no padded zero, the count of real zeros times mean^2 is what the plain sum holds)
    assert CR.rel(a[1], b[1]) < 2e-7 and torch.equal(a[0], b[0])


@pytest.mark.parametrize("kind", ("fwd", "bwd", "trans"))
@pytest.mark.parametrize("h,lay", [(16, "node"), (32, "edge"), (112, "node")])
def test_real_zeros_are_not_padding(kind, h, lay):
    """Every zero taken for padding (no count term): the rows with an exact zero in a real column leave the limit, the other
    rows of the same case do not.  The count without its - (128 - h) is wrong on every row."""
    p = W.problem(kind, h, lay, 8)
    assert W.failed(W.judge(p, W.Emu(rule="nocorr").run(p)))
    got, ref = W.Emu(rule="allpad").run(p), p.ref()
    n = p.rows[0] if kind != "bwd" else "gx"
    e = CR.row_err(got[n][:, p.real], ref[n][:, p.real])
    zero_rows = torch.zeros(W.M, dtype=torch.bool)
    zero_rows[::W.ZERO_EVERY] = True
    if kind == "trans":
        n = "z"
        e = CR.row_err(got[n], ref[n])
    lim = W.limit(p, n)
    assert float(e[zero_rows].min()) > lim, (float(e[zero_rows].min()), lim)
    assert float(e[~zero_rows].max()) < lim, (float(e[~zero_rows].max()), lim)


def test_zero_column_of_the_mlp_is_not_padding():
    for h, lay in ((16, "node"), (32, "edge"), (64, "node")):
        p = W.problem("mlp", h, lay, 8)
        assert bool((p.ref()["y3"][:, p.zero_col] == 0).all()) and bool(p.real[p.zero_col])
        assert W.failed(W.judge(p, W.Emu(rule="allpad").run(p))), p.tag
        assert not W.failed(W.judge(p, W.Emu().run(p))), p.tag


@pytest.mark.parametrize("kind", KINDS)
def test_other_mutations_of_the_rule_fail(kind):
    for h in (16, 64, 112):
        p = W.problem(kind, h, "node", 0)
        assert W.failed(W.judge(p, W.Emu(rule="inv128").run(p))), ("inv128", p.tag)
    for h in (16, 32, 64, 112):
        for off in W.OFFSETS:
            p = W.problem(kind, h, "edge", off)
            assert W.failed(W.judge(p, W.Emu(rule="edge_as_node").run(p))), ("edge_as_node", p.tag)


def test_reference_normalises_the_real_columns_only():
    p = W.problem("fwd", 32, "edge", 8)
    ln = p.ref()["ln"]
    assert W.padding_is_zero(ln, p.real)
    xh = (ln[:, p.real] - p.beta.double()[p.real]) / p.gamma.double()[p.real]
    assert float(xh.mean(1).abs().max()) < 1e-12 and float((xh.var(1, unbiased=False) - 1).abs().max()) < 1e-4
