"""CPU: the host side of the evaluation (gfv/evaluate.py, csrc/eval.hip): the new entry point is declared, exported and bound,
every bad argument is refused before anything touches a device, the batching of the indices, the guards, and the report formed
from a hand-made table against the formula of pre_train_Adam.py:177-184 in float64 - nothing here touches a GPU."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

import cases


def _cpu_model(**kw):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    return NNmodel(default_params(**kw))


def test_eval_entry_point_is_declared_exported_and_bound():
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    name = "gfv_eval_collect"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert len(getattr(handle, name).argtypes) == 17
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert name not in cmdlist._QUERIES                                    # it launches
    assert int(re.search(r"#define GFV_EVAL_RECORD (\d+)", header).group(1)) == lib.EVAL_RECORD == 16


def test_eval_collect_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 16 == 0
    ent = (C.c_int32 * 80)(*range(80))
    flg = (C.c_int32 * 80)()
    flg1 = (C.c_int32 * 80)(0, 1)
    ok = dict(uvp=p, xr=p, tgt=p, N=4, cb=p, ce=p, gp=p, nc=1, B=2, losses=p, ent=C.addressof(ent), flg=C.addressof(flg),
              table=p, ne=80, ws=p, cnt=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_eval_collect(a["uvp"], a["xr"], a["tgt"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["losses"],
                                    a["ent"], a["flg"], a["table"], a["ne"], a["ws"], a["cnt"], None)
    for name in ("uvp", "xr", "cb", "ce", "gp", "losses", "ent", "flg", "table", "ws", "cnt"):
        assert call(**{name: None}) == -1, name
    assert call(tgt=None, flg=C.addressof(flg1)) == -1             # a flag is set: the targets are read
    for name in ("N", "nc", "B", "ne"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(B=65) == -1                                                # GFV_POOL_MAX_GRAPHS
    assert call(ne=1) == -1                                                # entry 1 is outside [0, 1)
    for bad in ((0, -1), (3, 80), (7, 7), (7, 2, 7)):                      # outside [0, n_entries); one row, two writers
        arr = (C.c_int32 * len(bad))(*bad)
        assert call(ent=C.addressof(arr), B=len(bad)) == -1, bad
    assert call(xr=p + 4) == -1 and call(xr=p + 8) == -1                   # the state rows are read 16 bytes at a time


def test_batches_are_consecutive_runs_with_a_short_tail():
    from gfv.evaluate import check_indices, split_batches
    assert split_batches([4, 1, 5, 0, 3, 2], 2) == [[4, 1], [5, 0], [3, 2]]
    assert split_batches([1, 3, 0], 2) == [[1, 3], [0]]
    assert split_batches([2, 0, 3, 1], 4) == [[2, 0, 3, 1]]
    assert split_batches([2, 0, 3, 1], 8) == [[2, 0, 3, 1]]
    assert split_batches(range(7), 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert split_batches([5], 1) == [[5]]
    with pytest.raises(ValueError):
        split_batches([0, 1], 0)
    assert check_indices(None, 4) == [0, 1, 2, 3]
    assert check_indices([3, 0], 4) == [3, 0]
    assert check_indices(torch.tensor([2, 1]), 4) == [2, 1]
    with pytest.raises(ValueError, match="no entries"):
        check_indices([], 4)
    with pytest.raises(ValueError, match="no entries"):
        check_indices(None, 0)


def test_repeats_and_entries_outside_the_pool_are_refused():
    from gfv.evaluate import check_indices
    for bad in ([0, 0], [1, 2, 1], [3, 1, 2, 3]):
        with pytest.raises(ValueError, match="more than once"):
            check_indices(bad, 4)
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(ValueError, match="does not exist"):
            check_indices(bad, 4)


def _cpu_pool():
    graphs = cases.make_graphs("cavity_mixed_b1")
    return types.SimpleNamespace(x=[graphs[0].x], n=1, device=torch.device("cpu"))


def test_an_accumulating_normalizer_is_refused_with_sweeps_message():
    from gfv.evaluate import Evaluate
    from gfv.sweep import Sweep
    model = _cpu_model(dataset_size=100)
    assert model.node_norm.should_accumulate()
    with pytest.raises(ValueError, match="Normalizer") as want:
        Sweep(model, _cpu_pool(), max_graphs=1)
    with pytest.raises(ValueError, match="Normalizer") as got:
        Evaluate(model, _cpu_pool(), max_graphs=1)
    assert str(got.value) == str(want.value)


def test_cpu_tensors_and_bad_modes_are_refused():
    from gfv import functions as GF
    from gfv.evaluate import Evaluate
    pool = _cpu_pool()
    with pytest.raises(RuntimeError) as want:
        GF.require_gpu(pool.x[0])
    with pytest.raises(RuntimeError) as got:
        Evaluate(_cpu_model(dataset_size=1), pool, max_graphs=1)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="launch_mode"):
        Evaluate(_cpu_model(dataset_size=1), pool, launch_mode="hipgraph")
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_graphs"):
            Evaluate(_cpu_model(dataset_size=1), pool, max_graphs=bad)


# ---- the report ---------------------------------------------------------------------------------------------------------------
def _table(rows):
    t = torch.full((len(rows), 16), float("nan"), dtype=torch.float32)
    for k, r in enumerate(rows):
        t[k, :len(r)] = torch.tensor(r, dtype=torch.float32)
    return t


def _formula(row, w_cont, w_mom, w_press):
    """pre_train_Adam.py:177-184 on one row of stored fp32 values, in float64 (Python floats)."""
    cont, mom_x, mom_y, press = (float(v) for v in row[0:4])
    return w_press * press + w_cont * cont + w_mom * (mom_x + mom_y)


@pytest.mark.parametrize("weights", [None, (3.0, 0.7, 1.3)])
def test_the_report_is_the_formula_in_float64(weights):
    from gfv.evaluate import make_report
    from gfv.params import default_params
    p = default_params(dataset_size=1)
    w = weights or (p.loss_cont, p.loss_mom, p.loss_press)
    gen = torch.Generator().manual_seed(5)
    rows = []
    for k in range(11):
        loss = (torch.rand(4, generator=gen) * 10.0 ** -(k % 7)).tolist()
        norms = (torch.rand(12, generator=gen) + 0.1).tolist()
        rows.append(loss + norms)
    rows[3][13:16] = [float("nan")] * 3          # an entry without a target
    rows[3][10:13] = [float("nan")] * 3
    rows[5][7] = 0.0                             # a zero norm below a non-zero update, and 0 / 0
    rows[6][4], rows[6][7] = 0.0, 0.0
    table = _table(rows)
    entries = [9, 4, 7, 0, 3, 10, 2, 8, 1, 6, 5]
    rep = make_report(entries, table, w)
    assert rep.entries == entries and rep.nonfinite == 0
    assert rep.losses.dtype == torch.float32 and torch.equal(rep.losses, table[:, 0:4])
    want = [_formula(table[k], *w) for k in range(11)]
    assert rep.loss_batch.dtype == torch.float64 and rep.loss_batch.tolist() == want          # exactly
    total = 0.0
    for v in want:
        total += math.log(v)
    assert rep.objective == total / 11 and math.isfinite(rep.objective)                       # exactly
    assert rep.rel_update.dtype == rep.rel_error.dtype == torch.float64
    for k in range(11):
        for c in range(3):
            d, n = float(table[k, 4 + c]), float(table[k, 7 + c])
            got = float(rep.rel_update[k, c])
            if n == 0.0:
                assert (math.isnan(got) if d == 0.0 else got == math.inf), (k, c, got)
            else:
                assert got == d / n
            e, t = float(table[k, 10 + c]), float(table[k, 13 + c])
            got = float(rep.rel_error[k, c])
            assert math.isnan(got) if k == 3 else got == e / t
    assert torch.equal(rep.table.view(torch.int32), table.view(torch.int32))


def test_nonfinite_entries_stay_in_the_table_and_the_objective_says_so():
    from gfv.evaluate import make_report
    w = (2.0, 0.5, 1.0)
    good = [1e-3, 2e-4, 3e-4, 5e-2] + [1.0] * 12
    nan_row = [float("nan"), 2e-4, 3e-4, 5e-2] + [1.0] * 12
    inf_row = [1e-3, float("inf"), 3e-4, 5e-2] + [1.0] * 12
    rep = make_report([0, 1, 2], _table([good, nan_row, good]), w)
    assert rep.nonfinite == 1 and math.isnan(rep.objective)
    assert math.isnan(rep.loss_batch[1]) and rep.loss_batch[0] == _formula(_table([good])[0], *w)
    assert torch.isnan(rep.losses[1, 0]) and rep.losses.shape == (3, 4)
    rep = make_report([5, 6], _table([inf_row, good]), w)
    assert rep.nonfinite == 1 and rep.objective == math.inf
    rep = make_report([5, 6], _table([inf_row, nan_row]), w)
    assert rep.nonfinite == 2 and not math.isfinite(rep.objective)
    # a finite but non-positive loss_batch (negative weights): finite entries, the logarithm says it as torch.log would
    rep = make_report([0], _table([good]), (-2.0, -0.5, -1.0))
    assert rep.nonfinite == 0 and math.isnan(rep.objective)
    rep = make_report([0, 1], _table([good, good]), (0.0, 0.0, 0.0))
    assert rep.nonfinite == 0 and rep.objective == -math.inf
