"""CPU: the row-by-row checks of tests/chain_rows.py on reference backends - fp32 eager autograd keeps the flat per-row tolerance
on every layout, the emulated design (float64 arithmetic, fp16 hi + lo fragments behind the kernels' per-tile scales) keeps
TOL_ROW + F_i and the two conditions exactly as the kernels must (tests/test_chain_rows_gpu.py) - and the checks bite: an
emulator that flushes fp16 subnormals, scales its fragments 2^4 too small or reports scales it does not use fails them, and so
do two exchanged small rows that a global max|a - b| / max|b| lets through."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_rows as R  # noqa: E402

M = 1317      # 41 tiles of 32 rows + 5 rows; 6.86 regions of 192 rows


def _run(backend, shape, layout, M=M, scale=0.3, **kw):
    c = R.case(shape, M, scale)
    return R.checks(c, layout, backend.run(c, layout), **kw)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp32_autograd_keeps_the_flat_tolerance_on_every_row(shape):
    for layout in R.LAYOUTS:
        L = _run(R.Torch32(), shape, layout)
        assert not R.failed(L), R.report(R.failed(L))
        flat = [c.value for c in L if c.name.endswith("rows_flat")]
        assert len(flat) == len(R.ROWS_ALL[shape]) and max(flat) < 2.5e-6      # (1.1e-6 measured: a quarter of the tolerance)


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_emulated_design_keeps_tolerance_plus_floor(shape, tile):
    for layout in R.LAYOUTS:
        L = _run(R.Emu(tile), shape, layout)
        assert not R.failed(L), R.report(R.failed(L))
        # ... with room: the floor is a bound on the design's error, not a fit to it
        assert max(c.value for c in L if c.name.endswith("rows_floor")) < 0.25, R.report(L)


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("scale", [0.06, 1.0])
def test_emulated_design_at_other_weight_scales(scale, tile):
    """The floor follows the weights' column norms: small (0.06) and large (1.0) weights, every ratio inside every tile."""
    L = _run(R.Emu(tile), "edge", "mixed", scale=scale)
    assert not R.failed(L), R.report(R.failed(L))
    assert max(c.value for c in L if c.name.endswith("rows_floor")) < 0.25, R.report(L)


def test_small_launch_of_33_rows():
    for be in (R.Torch32(), R.Emu(32)):
        for layout in R.LAYOUTS:
            L = _run(be, "edge", layout, M=33)
            assert not R.failed(L), R.report(R.failed(L))


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("mutation", [dict(flush=True), dict(shift=-4), dict(report_shift=6)])
def test_wrong_emulators_fail(mutation, tile):
    """fp16 subnormals flushed (the rows below 2^-10 of their tile lose their low halves, then their high ones); fragment
    scales 2^4 too small (rows pass against the floor the emulator then reports - the exponent-0 rows' floor does not);
    reported scales 2^6 above the used ones (the floor shrinks under the error, and the scale breaks the overflow bound)."""
    bad = R.failed(_run(R.Emu(tile, **mutation), "edge", "mixed"))
    want = {"flush": "rows_floor", "shift": "floor_of_top_rows", "report_shift": "rows_floor"}[next(iter(mutation))]
    assert any(c.name.endswith(want) for c in bad), R.report(bad)
    if "report_shift" in mutation:
        assert any(c.name.endswith("g3_scale_bound") for c in bad), R.report(bad)
        # a layout without a small row beside a large one sees the wrong report through the overflow bound alone
        bad = R.failed(_run(R.Emu(tile, **mutation), "node", "zigzag"))
        assert any(c.name.endswith("g3_scale_bound") for c in bad), R.report(bad)


def test_exchanged_small_rows_fail_row_by_row_and_pass_globally():
    c = R.case("edge", M)
    out = R.Torch32().run(c, "mixed")
    i, j = 20, 41                                 # both at 2^-20 of their neighbours
    assert R.exponents("mixed", M)[0][[i, j]].tolist() == [-20, -20]
    ge = out.rows["ge"].clone()
    ge[[i, j]] = ge[[j, i]]
    rows = dict(out.rows, ge=ge)
    bad = R.failed(R.checks(c, "mixed", out._replace(rows=rows)))
    assert [b.name for b in bad] == [f"edge/{M}/mixed/ge/rows_flat"] and bad[0].value > 0.5
    assert R.rel(ge, c.ref("mixed")[0]["ge"]) < R.TOL_ROW          # what every earlier test of these kernels measured
    # the same exchange judged with reported scales (the emulator's): the floor does not excuse it either
    out = R.Emu(64).run(c, "mixed")
    ge = out.rows["ge"].clone()
    ge[[i, j]] = ge[[j, i]]
    bad = R.failed(R.checks(c, "mixed", out._replace(rows=dict(out.rows, ge=ge))))
    assert [b.name for b in bad] == [f"edge/{M}/mixed/ge/rows_floor"]


def test_check_names_do_not_depend_on_the_backend():
    c = R.case("node", M)
    a = [k.name for k in R.checks(c, "zeros", R.Torch32().run(c, "zeros"), names=R.ROWS_COL["node"])]
    b = [k.name for k in R.checks(c, "zeros", R.Emu(64).run(c, "zeros"), names=R.ROWS_COL["node"])]
    assert a == b and len(a) == 3 * 3 + len(R.SUMS) + 4


def test_layouts_and_interior_rows():
    m = R.multipliers("zigzag", 1000)
    assert m[[0, 191, 192, 400, 600, 800, 960]].tolist() == [1.0, 1.0, 8.0, 0.5, 4.0, 0.25, 1.0]
    it = R.interior(m)
    assert bool(it[:129].all()) and not bool(it[129:255].any()) and bool(it[255:321].all()) and not bool(it[321])
    assert bool(it[831:897].all()) and not bool(it[897:].any())      # (the last run, 40 rows, is too short to hold an interior row)
    assert not bool(R.interior(R.multipliers("mixed", 500)).any())
    assert R.multipliers("stairs_down", 400)[[0, 192, 384]].tolist() == [1.0, 2.0 ** -6, 2.0 ** -12]
    assert R.multipliers("stairs_up", 400)[[0, 192, 384]].tolist() == [1.0, 2.0 ** 6, 2.0 ** 12]
    assert R.multipliers("stairs_down", 3100)[[3071, 3072]].tolist() == [2.0 ** -90, 1.0]      # a second staircase
    cd, cu = R.multipliers("cliff_down", 1000), R.multipliers("cliff_up", 1000)
    assert cd[449] == 1 and cd[450] == 2.0 ** -40 and torch.equal(cu, cd.flip(0))
    assert not bool(R.flat_rows("cliff_down", 1000)[450:].any()) and bool(R.flat_rows("cliff_up", 1000)[:487].all())
    z = R.multipliers("zeros", 1317)
    assert int((z == 0).sum()) == 600 and z[199] == 0 and z[200] == 1 and z[658] == 0 and z[1117] == 0 and z[1116] == 1
    assert set(R.multipliers("mixed", 100)[:32].log2().tolist()) == set(float(-k) for k in range(21))


def test_tile_spread_on_a_hand_made_array():
    rows = torch.zeros(10, 3)
    rows[0, 1], rows[1, 0], rows[2, 2] = 4.0, -1.0, 0.5      # tile 0: 4 / 0.5 (row 3 is zero: left out)
    rows[4, 0], rows[5, 1] = 2.0, -2.0                       # tile 1: 1
    rows[9, 2] = 7.0                                         # tile 2 (ragged): tile of rows 8, 9: one non-zero row
    assert R.tile_spread(rows, 4).tolist() == [8.0, 1.0, 1.0]
    assert R.tile_spread(rows, 10).tolist() == [14.0]
    assert R.tile_spread(torch.zeros(5, 2), 4).tolist() == [1.0, 1.0]
