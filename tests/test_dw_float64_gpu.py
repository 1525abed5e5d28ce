"""GPU: every path of csrc/dw.hip against the float64 statements of tests/dw_float64.py, entry by entry - the fp32 MFMA body
(gfv_set_f16split(0)), the split-fp16 body in its 3-product (1) and hi x hi (2) forms, the bf16 instantiation (3) and
dw_narrow_kernel; FULL and guarded tiles, vector and scalar loads, gather, in_add, GELU / LayerNorm on load at hidden 128 / 64 /
32, column scales, handed and own slab scales, the bias-gradient fold, row tails wherever the slab partition puts them, and
gfv_dw_multi called the way the engine calls it.  Every case runs twice and must give equal bits; outputs are views inside
sentinel-filled buffers; the device status word must stay 0.

Limits and where they come from (tests/dw_float64.py; tests/test_dw_float64_cpu.py shows that a float32 torch evaluation keeps a
quarter of each), with the worst figure measured on the MI355X per case family, forms 0 / 1 / 2 / 3:
  sum limit 2e-6 of sum|terms| per entry (test_rowtile_and_dw_extreme_dynamic_range; forms 2 / 3: of the rounded operands' terms,
  against D.Emu - TIGHT of tests/test_bf16_form_gpu.py):
    row geometry                         2.6e-7 / 5.2e-7 / 1.2e-7 / 8.4e-8
    width geometry, M = 97               2.0e-7 / 1.1e-7 / 8.0e-8 / 8.0e-8        M = 333   8.7e-8 / 6.7e-8 / 4.3e-8 / 4.0e-8
    on-load operations, M = 97           2.4e-7 / 1.5e-7 / 6.7e-8 / 5.4e-8        M = 1100  5.7e-8 / 4.0e-8 / 2.3e-8 / 1.7e-8
    LayerNorm of rows 8 / 32 std from zero, hidden 16 .. 128 (in units of max(2e-6, 4 e32), D.judge), M = 97
                                         7.5e-7 / 7.3e-7 / 3.5e-8 / 3.5e-8        M = 1100  3.6e-7 / 3.5e-7 / 1.4e-8 / 1.4e-8
    scales                               3.6e-7 / 4.5e-7 / 4.8e-7 / 2.7e-7
    group scales, M = 33 / 97 / 3001     2.3e-7 / 5.0e-7 / 2.3e-7 / 2.3e-7 (the largest of the three)
    six tiles, M = 97                    2.1e-7 / 1.4e-7 / 6.4e-8 / 6.3e-8        M = 3019  3.5e-8 / 2.7e-8 / 1.4e-8 / 1.2e-8
    integer cases of every family        bit for bit in all four forms
  chained limit 2e-3 of max|ref| (forms 2 / 3 with a_op 1 / 2; CHAINED of tests/test_bf16_form_gpu.py):
    on-load operations                   4.0e-5 / 1.2e-4                          six tiles  5.0e-5 / 4.7e-4
  unscaled activations of 1e-3 / 1e-4 / 1e-6, split form (1): limit 2e-6 sum|terms| + 2^-25 sum|G| (the fp16 subnormal quantum):
    0.28 of that bound at M = 97 (0.09 / 0.02 at 1100 / 20011, as the emulation of the split predicts); with no floor granted the
    1e-6 columns are 1.2e-2 of sum|terms| from the float64 product (the O(1) columns 4.9e-8 in a CPU emulation); column-scaled, the same inputs keep
    the plain limit (1.5e-7).  A finding about the inputs, not the kernel: a single row (M = 1) with |a| = 3e-4 is 1.9e-5 from
    the float64 product in the split form, the figure a CPU emulation of the split gives - activations are split unscaled, so
    the random activations of every other case keep |a| >= 2^-4 (D.A_MIN) and the floor is asserted negligible there.
"""
import contextlib
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dw_float64 as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from gfv import lib
    lib.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def product_form(f):
    from gfv import lib as L
    lib = L.load()
    assert lib.gfv_f16split_enabled() == 1 and lib.gfv_hidden_size() == 128
    lib.gfv_set_f16split(f)
    try:
        yield lib
    finally:
        lib.gfv_set_f16split(1)
        lib.gfv_set_hidden_size(128)


@pytest.fixture(params=[0, 1, 2, 3])
def form(request):
    with product_form(request.param):
        yield request.param


def _status():
    from gfv import lib as L
    flags = C.c_int32(0)
    L.check(L.load().gfv_status_flags(C.byref(flags)), "gfv_status_flags")
    return flags.value


@pytest.fixture(autouse=True)
def status_word_stays_zero(dev):
    _status()
    yield
    assert _status() == 0, "a weight-gradient launch of these tests raised a range flag"


def _same_partition(c):
    """The restated slab rule must be the library's for this case, or the row tails are not where the case wants them."""
    from gfv import lib as L
    rows = C.c_int32(0)
    slabs = L.load().gfv_dw_slabs(c.M, len(c.tiles), C.byref(rows))
    if (rows.value, slabs) != D.dw_slabs(c.M, len(c.tiles)):
        pytest.skip(f"{c.name}, M = {c.M}: the library partitions into {slabs} slabs of {rows.value} rows, the default rule into "
                    f"{D.dw_slabs(c.M, len(c.tiles))} - GFV_DW_WGS / GFV_DW_WGS_SMALL set?")


def _twice(gpu, c, **kw):
    """A case's results, run twice on the same device tensors: the kernel claims a fixed summation order."""
    from gfv import lib as L
    _same_partition(c)
    L.check(L.load().gfv_set_hidden_size(c.hidden), "gfv_set_hidden_size")
    try:
        up = gpu.upload(c)
        a, b = gpu.run(c, up=up, **kw), gpu.run(c, up=up, **kw)
    finally:
        L.load().gfv_set_hidden_size(128)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.dW, y.dW) and (x.db is None or torch.equal(x.db, y.db)), f"{c.name} M {c.M} tile {i}: two runs differ"
    return a


def _judge(dev, cases, family):
    gpu, ck = D.Gpu(dev), D.Checks()
    for c in cases:
        D.judge(c, _twice(gpu, c), ck)
    print(f"FIGURE {family}: sum {ck.worst('sum'):.2e} chained {ck.worst('chained'):.2e} unequal {ck.worst('equal'):.0f} "
          f"no floor {ck.worst('raw'):.2e} of the bound {ck.worst('used'):.2f} ({len(ck)} checks)")
    bad = ck.failed()
    assert not bad, "\n".join(f"{c.kind} {c.value:.3e} {c.name}" for c in bad)


def test_row_geometry(dev, form):
    """128 x 128, with and without a gather (indices with repeats, out of order, into more and into fewer source rows than M),
    M = 1 .. 129 around the 32-row sub-tile and the 64-row minimum slab, and one M per segment count whose slabs are 96 rows
    with a last slab of a full sub-tile plus a tail that is no multiple of 4 (the index prefetch runs one sub-tile ahead)."""
    _judge(dev, D.row_cases(form, False), f"rows form {form}")


def test_row_geometry_bit_for_bit(dev, form):
    """Small integers in G and A: every product and partial sum is exact in every form, so dW and db are the integer result bit
    for bit - a shifted, dropped or doubled row has no tolerance to hide in."""
    _judge(dev, D.row_cases(form, True), f"rows exact form {form}")


@pytest.mark.parametrize("M", [97, 333])
def test_width_geometry(dev, form, M):
    """(n_out, ldg) x (width, ld): vector and scalar loads, guarded tiles, column offsets, one to three segments of mixed
    widths, and widths <= 16 both where dw_narrow_kernel takes them and where it must not (in_add, idx, a later segment) -
    bit for bit on integers and against float64 on random rows; the sentinels around dW and db survive (D.Gpu)."""
    _judge(dev, D.width_cases(form, True, M), f"widths exact form {form} M {M}")
    _judge(dev, D.width_cases(form, False, M), f"widths form {form} M {M}")


@pytest.mark.parametrize("M", [97, 1100])
def test_on_load_operations(dev, form, M):
    """in_add, in_add + gather + GELU, LayerNorm on load at hidden 128, 64 (node layout) and 32 (edge layout: halves at columns
    0 and 64) with zero dead columns and gamma = beta = 0 there - the reference normalises over the real columns only."""
    _judge(dev, D.onload_cases(form, M), f"on-load form {form} M {M}")


@pytest.mark.parametrize("M", [97, 1100])
def test_on_load_layernorm_of_rows_far_from_zero(dev, form, M):
    """LayerNorm on load at hidden 16 / 32 / 64 / 112 / 128 of rows whose mean is 8 / 32 standard deviations from zero, with exact
    zeros inside real columns, and at hidden 16 / 112 without an offset (D.ln_offset_cases): the limits of every on-load case."""
    _judge(dev, D.ln_offset_cases(form, M), f"on-load LayerNorm offsets form {form} M {M}")


def test_scales(dev, form):
    """An all-zero slab of G beside O(1) ones, an all-zero column of A under column scales, columns spanning 1e-6 .. 1e+6 at the
    tail shapes, and activations of 1e-3 / 1e-4 / 1e-6 beside O(1) ones: unscaled (the split form owes the float64 product up to
    the fp16 floor of tests/dw_float64.py, which excuses nothing on the O(1) columns) and column-scaled (plain 2e-6)."""
    cases = list(D.scale_cases(form))
    ck = D.Checks()
    for c in cases:
        if c.floor:
            D.floor_conditions(c, ck)
    assert not ck.failed(), ck.report()
    _judge(dev, cases, f"scales form {form}")


def _chain_scales(dev, G, M):
    """The gscale rows a dX chain launch leaves for its gradient rows, made as test_chain_group_scales_feed_the_weight_gradient
    makes them (slot 0: the launch's input rows G); None where no chain family with group scales takes the launch."""
    from gfv import lib as L, ops
    g = torch.Generator().manual_seed(21)
    d = lambda t: t.to(dev).contiguous()
    z2, z1 = d(torch.randn(M, 128, generator=g)), d(torch.randn(M, 128, generator=g))
    W3t, W2t = d(torch.randn(128, 128, generator=g) * 0.1), d(torch.randn(128, 128, generator=g) * 0.1)
    wi = ops.WeightImages(dev, torch.maximum(W3t.abs().max(), W2t.abs().max()).reshape(1).clone())
    wi.static = [(0, 1 << 62)]
    gz2, gz1 = torch.empty(M, 128, device=dev), torch.empty(M, 128, device=dev)
    gs = torch.zeros(3, ops.gscale_ld(M), device=dev)
    have = ops.rowtile_chain(M, [ops.Seg(d(G))], [ops.LayerSpec(W3t, None, L.OP_MUL_DGELU, save=gz2, aux=z2),
                                                  ops.LayerSpec(W2t, None, L.OP_MUL_DGELU, aux=z1)], [gz1], wimg=wi, gscale=gs)
    torch.cuda.synchronize()
    return gs[0].cpu() if have else None


@pytest.mark.parametrize("M", [33, 97, 3001])
@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_handed_group_scales_give_the_bits_of_the_own_pass(dev, f, M):
    """gscale handed over (per 16 rows, as a chain launch writes them - by the rule, and from an actual chain launch) against
    the kernel's own pass over G: the same slab scale, so the same bits; and both are right."""
    gpu = D.Gpu(dev)
    own, handed = D.gscale_case(f, M, False), D.gscale_case(f, M, True)
    chain = _chain_scales(dev, own.tiles[0].G, M)        # (in the default form, before the switch)
    n16 = (M + 15) // 16
    if chain is not None:
        assert torch.equal(chain[:n16], handed.tiles[0].gscale), "a chain launch's group scales are not the stated rule's"
    with product_form(f):
        a, b = _twice(gpu, own), _twice(gpu, handed)
        assert torch.equal(a[0].dW, b[0].dW) and torch.equal(a[0].db, b[0].db)
        if chain is not None:
            handed.tiles[0].gscale = chain.clone()
            c = _twice(gpu, handed)
            assert torch.equal(a[0].dW, c[0].dW)
        ck = D.judge(own, a)
        assert not ck.failed(), ck.report()
        print(f"FIGURE gscale form {f} M {M}: sum {ck.worst('sum'):.2e} (chain-made scales: {chain is not None})")


@pytest.mark.parametrize("M", [97, 3019])
def test_dw_multi_called_directly(dev, form, M):
    """gfv_dw_multi as the engine calls it: six tiles on three gradient tensors, tiles without a bias gradient, a zeroed
    workspace; grad_block with accumulate 0 (over a block of garbage) and 1 (onto a non-zero block), and grad_block = NULL
    followed by the caller's gfv_reduce_partials_2d over the slab workspace."""
    gpu = D.Gpu(dev)
    c = D.multi_case(form, M)
    junk = torch.full((c.block_floats,), 3.0e7)
    ck = D.judge(c, _twice(gpu, c, prior=junk))
    D.judge(c, _twice(gpu, c, reduce="2d"), ck)
    x = D.multi_case(form, M, exact=True)
    want = D.expected_block(x, D.reference(x))
    prior = torch.randint(-5, 6, (x.block_floats,), generator=torch.Generator().manual_seed(M)).float()
    _same_partition(x)
    up = gpu.upload(x)
    for kw, ref in ((dict(prior=junk), want), (dict(prior=prior, accumulate=True), want + prior.double()),
                    (dict(reduce="2d"), want)):
        one, two = gpu.multi(x, up=up, **kw), gpu.multi(x, up=up, **kw)
        assert torch.equal(one, two)
        ck.equal(f"multi-exact {sorted(kw)} block", one, ref)
    # the slab workspace as grad_block = NULL leaves it: its slab sum is the block, padding slots still zero
    ws = gpu.multi(x, up=up, reduce=False)
    ck.equal("multi-exact slab workspace, summed", ws.double().sum(0), want)
    print(f"FIGURE multi form {form} M {M}: sum {ck.worst('sum'):.2e} chained {ck.worst('chained'):.2e}")
    assert not ck.failed(), ck.report()


@pytest.mark.parametrize("M", [97, 6001])
def test_linear_dw_accumulates(dev, form, M):
    """accumulate=True on ops.linear_dw (gfv_linear_dw_gs): onto non-zero dW and db, integers, bit for bit."""
    gpu = D.Gpu(dev)
    c = D.linear_case("accumulate", M, form, n_out=35, ldg=35, segs=D.ROW_SEGS[3] if M > 97 else D.ROW_SEGS[2], idx="fewer", exact=True)
    _same_partition(c)
    want = D.expected_block(c, D.reference(c))[:c.tiles[0].db_off + 35]
    prior = torch.randint(-5, 6, (want.numel(),), generator=torch.Generator().manual_seed(M)).float()
    up = gpu.upload(c)
    for acc, ref in ((True, want + prior.double()), (False, want)):
        one, two = (gpu.linear(c, up=up, accumulate=acc, prior=prior) for _ in range(2))
        assert torch.equal(one, two) and torch.equal(one.double(), ref), (acc, int((one.double() != ref).sum()))


@pytest.mark.parametrize("accumulate", [False, True])
def test_no_rows(dev, form, accumulate):
    """M = 0 (include/gfv.h): accumulate = 0 writes zeros to dW and db, accumulate = 1 leaves them unchanged, and neither reads
    the workspace - which holds NaN here (gfv_linear_dw_gs used to reduce an unwritten region of it into the outputs)."""
    gpu = D.Gpu(dev)
    for c in D.empty_cases():
        n = c.tiles[0].db_off + c.tiles[0].n_out
        prior = torch.arange(n).float() - 7.0
        got = gpu.linear(c, accumulate=accumulate, prior=prior)
        assert torch.equal(got, prior if accumulate else torch.zeros(n)), c.name
    m = D.multi_case(form, 97)
    m.M = 0
    prior = torch.arange(m.block_floats).float() - 7.0
    got = gpu.multi(m, accumulate=accumulate, prior=prior, workspace_fill=float("nan"))
    assert torch.equal(got, prior if accumulate else torch.zeros(m.block_floats))
    assert gpu.multi(m, reduce=False).shape[0] == 0
