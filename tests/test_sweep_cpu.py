"""CPU: the host side of the sweep (gfv/sweep.py, csrc/sweep.hip): the new entry points are declared, exported and bound, every
bad argument is refused before anything touches a device, the slot scheduler, and the guards - nothing here touches a GPU."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import cases

NEW = ("gfv_sweep_advance", "gfv_sweep_mirror_create", "gfv_sweep_mirror_free")


def _cpu_model(**kw):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    return NNmodel(default_params(**kw))


def test_sweep_entry_points_are_declared_exported_and_bound():
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    for name in NEW:
        assert name in declared and name in lib.declared_symbols() and hasattr(handle, name), name
        assert getattr(handle, name).argtypes is not None
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3                                   # additive: the version stays
    # the mirror pair launches nothing: never part of a recorded list; the advance launch is
    assert {"gfv_sweep_mirror_create", "gfv_sweep_mirror_free"} <= cmdlist._QUERIES
    assert "gfv_sweep_advance" not in cmdlist._QUERIES


def test_sweep_advance_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 16 == 0
    ok = dict(uvp=p, xb=p, x=p, N=4, cb=p, ce=p, gp=p, nc=1, B=1, losses=p, ws=p, ctl=p, slots=p, last=p, state3=p, mirror=p,
              state=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_sweep_advance(a["uvp"], a["xb"], a["x"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["losses"],
                                     a["ws"], a["ctl"], a["slots"], a["last"], a["state3"], a["mirror"], a["state"], None)
    for name in ("uvp", "xb", "x", "cb", "ce", "gp", "losses", "ws", "ctl", "slots", "last", "state3", "mirror", "state"):
        assert call(**{name: None}) == -1, name
    for name in ("N", "nc", "B"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(xb=p + 4) == -1        # the node state rows are read and written 16 bytes at a time
    assert call(x=p + 8) == -1


def test_sweep_mirror_pair_rejects_bad_arguments():
    from gfv import lib as L
    lib = L.load(raw=True)
    host, dev = C.POINTER(C.c_int32)(), C.c_void_p()
    assert lib.gfv_sweep_mirror_create(0, C.byref(host), C.byref(dev)) == -1
    assert lib.gfv_sweep_mirror_create(-5, C.byref(host), C.byref(dev)) == -1
    assert lib.gfv_sweep_mirror_create(4, None, C.byref(dev)) == -1
    assert lib.gfv_sweep_mirror_create(4, C.byref(host), None) == -1
    assert not host and not dev.value
    assert lib.gfv_sweep_mirror_free(None) == -1


# ---- the scheduler ------------------------------------------------------------------------------------------------------------
def _drive(entries, sig, n_slots, lifetime):
    """Run a SlotScheduler to the end: entry e is finished `lifetime(e)` steps after it was loaded.  -> (every batch as loaded,
    batch signature per load, the slot of every entry)."""
    from gfv.sweep import SlotScheduler
    s = SlotScheduler(entries, sig, n_slots)
    cur = s.start()
    left = {b: lifetime(e) for b, e in enumerate(cur)}
    slot_of = {e: b for b, e in enumerate(cur)}
    loads, sigs = [list(cur)], [s.batch_signature()]
    for _ in range(10000):
        for b in left:
            left[b] = max(left[b] - 1, 0)
        retired = [b for b, n in left.items() if n == 0]
        if len(retired) == len(cur) and not s.pending:
            return loads, sigs, slot_of
        before = list(s.slots)
        new = s.replace(retired)
        for b, e in enumerate(s.slots):
            if b not in new:
                assert e == before[b], "an entry that was not replaced moved"
        for b, e in new.items():
            assert b in retired and e not in slot_of
            slot_of[e] = b
            left[b] = lifetime(e)
        if new:
            loads.append(list(s.slots))
            sigs.append(s.batch_signature())
    raise AssertionError("the schedule did not terminate")


def test_scheduler_schedules_every_entry_exactly_once_and_never_moves_a_live_one():
    entries = [7, 3, 9, 0, 4, 8, 1]
    loads, sigs, slot_of = _drive(entries, lambda e: "a", 3, lambda e: 1 + e % 4)
    assert sorted(slot_of) == sorted(entries)
    assert loads[0] == [7, 3, 9]
    seen = [e for e in loads[0]]
    for prev, cur in zip(loads, loads[1:]):
        seen += [e for b, e in enumerate(cur) if prev[b] != e]
    assert sorted(seen) == sorted(entries) and len(seen) == len(entries)
    assert len(set(sigs)) == 1


def test_scheduler_prefers_the_same_signature_and_keeps_the_batch_signature():
    from gfv.sweep import SlotScheduler
    sig = {0: "a", 1: "b", 2: "b", 3: "a", 4: "c", 5: "a"}
    s = SlotScheduler([0, 1, 2, 3, 4, 5], sig.get, 2)
    assert s.start() == [0, 1] and s.batch_signature() == ("a", "b")
    assert s.replace([0]) == {0: 3}                        # not 2, the head of the queue: 3 has slot 0's signature
    assert s.slots == [3, 1] and s.batch_signature() == ("a", "b")
    assert s.replace([1]) == {1: 2}
    assert s.batch_signature() == ("a", "b")
    assert s.replace([0, 1]) == {0: 5, 1: 4}               # slot 1: no "b" is pending - the first pending entry of any signature
    assert s.batch_signature() == ("a", "c")
    assert not s.pending


def test_scheduler_mixed_queue_terminates_and_retired_slots_stay():
    from gfv.sweep import SlotScheduler
    sig = lambda e: "abc"[e % 3]
    entries = list(range(11))
    loads, sigs, slot_of = _drive(entries, sig, 4, lambda e: 1 + (e * 5) % 3)
    assert sorted(slot_of) == entries
    assert len(loads[-1]) == 4                             # the batch is never shrunk
    s = SlotScheduler([0, 1, 2], sig, 2)
    assert s.start() == [0, 1]
    assert s.replace([1]) == {1: 2}
    assert s.replace([0, 1]) == {} and s.slots == [0, 2]   # nothing pending: the retired slots keep their entries
    few = SlotScheduler([5], sig, 4)
    assert few.start() == [5] and few.replace([0]) == {}
    with pytest.raises(ValueError):
        SlotScheduler([0], sig, 0)


# ---- guards -------------------------------------------------------------------------------------------------------------------
def _cpu_pool():
    graphs = cases.make_graphs("cavity_mixed_b1")
    return types.SimpleNamespace(x=[graphs[0].x], n=1, device=torch.device("cpu"))


def test_sweep_refuses_cpu_tensors_like_require_gpu():
    from gfv import functions as GF
    from gfv.sweep import Sweep
    pool = _cpu_pool()
    with pytest.raises(RuntimeError) as want:
        GF.require_gpu(pool.x[0])
    with pytest.raises(RuntimeError) as got:
        Sweep(_cpu_model(dataset_size=1), pool, max_graphs=1)
    assert str(got.value) == str(want.value)


def test_duplicate_and_out_of_range_entries_are_refused():
    from gfv.sweep import check_entries
    assert check_entries(None, 4) == [0, 1, 2, 3]
    assert check_entries([3, 0], 4) == [3, 0]
    assert check_entries([], 4) == []
    for bad in ([0, 0], [1, 2, 1], [4], [-1], [0, 7]):
        with pytest.raises(ValueError):
            check_entries(bad, 4)


@pytest.mark.parametrize("bad", [0, -1, float("inf"), float("nan"), 2.5, None, 2 ** 31])
def test_bad_max_steps_is_refused(bad):
    from gfv.sweep import Sweep, check_max_steps
    with pytest.raises(ValueError, match="max_steps"):
        check_max_steps(bad)
    with pytest.raises(ValueError, match="max_steps"):
        Sweep(_cpu_model(dataset_size=1), _cpu_pool(), max_steps=bad)
    assert check_max_steps(1) == 1 and check_max_steps(40000.0) == 40000


def test_an_accumulating_normalizer_is_refused():
    from gfv.sweep import Sweep
    model = _cpu_model(dataset_size=100)
    assert model.node_norm.should_accumulate()
    with pytest.raises(ValueError, match="Normalizer"):
        Sweep(model, _cpu_pool(), max_graphs=1)
