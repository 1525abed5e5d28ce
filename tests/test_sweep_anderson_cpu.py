"""CPU: the host side of Anderson acceleration per slot of a `Sweep` (gfv/sweep.py, gfv/anderson.py SlotAndersonState,
csrc/sweep_anderson.hip, csrc/sweep.hip gfv_sweep_advance_aa): the three entry points are declared, exported and
bound and the ABI version stays; every bad argument is refused before anything touches a device; the `Sweep` argument checks are
those of `gfv.anderson.check_args`; an entry that does not fit the ring stride is refused by a plain function.  Nothing here
touches a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

import cases

NAMES = ("gfv_sweep_anderson_gram", "gfv_sweep_anderson_mix", "gfv_sweep_advance_aa")


def test_entry_points_are_declared_exported_and_bound():
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in lib.declared_symbols() and hasattr(handle, name), name
        assert name not in cmdlist._QUERIES                                # they launch: part of a recorded list
    assert len(handle.gfv_sweep_anderson_gram.argtypes) == 27
    assert len(handle.gfv_sweep_anderson_mix.argtypes) == 17
    assert len(handle.gfv_sweep_advance_aa.argtypes) == len(handle.gfv_sweep_advance.argtypes) + 1 == 19
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert int(re.search(r"#define GFV_ABI_VERSION (\d+)", header).group(1)) == 3
    # the existing entry points keep their signatures
    assert len(handle.gfv_anderson_gram.argtypes) == 25 and len(handle.gfv_anderson_mix.argtypes) == 17
    assert len(handle.gfv_sweep_advance.argtypes) == 18


def _calls():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p16 = p if p % 16 == 0 else p + 8
    gram_ptrs = ("uvp", "xb", "cb", "ce", "gp", "f_prev", "g_prev", "dF", "dG", "state", "r_prev", "gamma", "ws", "cnt", "ctl",
                 "slots", "aa_slot", "aa_count")
    mix_ptrs = ("uvp", "f_cur", "cb", "ce", "gp", "dF", "dG", "gamma", "slots", "aa_slot")
    adv_ptrs = ("uvp", "xb", "x", "cb", "ce", "gp", "losses", "ws", "ctl", "slots", "last", "state3", "mirror", "st", "aa_slot")
    ok = dict({n: p16 for n in gram_ptrs + mix_ptrs + adv_ptrs}, N=4, nc=1, B=2, m=4, reg=1e-10, restart=10.0, start=0, beta=1.0,
              stride=4)

    def gram(**kw):
        a = {**ok, **kw}
        return lib.gfv_sweep_anderson_gram(a["uvp"], a["xb"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["m"], a["reg"],
                                           a["restart"], a["start"], a["stride"], a["f_prev"], a["g_prev"], a["dF"], a["dG"],
                                           a["state"], a["r_prev"], a["gamma"], a["ws"], a["cnt"], a["ctl"], a["slots"],
                                           a["aa_slot"], a["aa_count"], None)

    def mix(**kw):
        a = {**ok, **kw}
        return lib.gfv_sweep_anderson_mix(a["uvp"], a["f_cur"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["m"],
                                          a["beta"], a["stride"], a["dF"], a["dG"], a["gamma"], a["slots"], a["aa_slot"], None)

    def adv(**kw):
        a = {**ok, **kw}
        return lib.gfv_sweep_advance_aa(a["uvp"], a["xb"], a["x"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["losses"],
                                        a["ws"], a["ctl"], a["slots"], a["last"], a["state3"], a["mirror"], a["st"], a["aa_slot"],
                                        None)
    return gram, mix, adv, gram_ptrs, mix_ptrs, adv_ptrs, p16


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    gram, mix, adv, gram_ptrs, mix_ptrs, adv_ptrs, p = _calls()
    nan = float("nan")
    for fn, ptrs in ((gram, gram_ptrs), (mix, mix_ptrs), (adv, adv_ptrs)):
        for name in ptrs:
            assert fn(**{name: None}) == -1, name
        for name in ("N", "nc", "B"):
            assert fn(**{name: 0}) == -1, name
            assert fn(**{name: -3}) == -1, name
    for fn in (gram, mix):
        for m in (0, -1, 9, 64):
            assert fn(m=m) == -1, m
        for stride in (0, -1, -(2 ** 31)):
            assert fn(stride=stride) == -1, stride
    for beta in (0.0, -0.5, 1.0000001, 2.0, nan, float("inf")):
        assert mix(beta=beta) == -1, beta
    for reg in (-1e-30, -1.0, nan):
        assert gram(reg=reg) == -1, reg
    for restart in (-1.0, nan, 1e-3, 0.5, 1.0):                            # 0 (off) and factors above 1 are the valid ones
        assert gram(restart=restart) == -1, restart
    for name in ("r_prev", "gamma", "ws"):                                 # the double buffers are 8-byte aligned
        assert gram(**{name: p + 4}) == -1, name
    assert mix(gamma=p + 4) == -1
    for name in ("xb", "x"):                                               # as gfv_sweep_advance: float4 rows
        assert adv(**{name: p + 8}) == -1, name


def test_sweep_takes_the_arguments_of_rollout_and_checks_them_first():
    from gfv.rollout import Rollout
    from gfv.sweep import Sweep
    sw, ro = inspect.signature(Sweep.__init__).parameters, inspect.signature(Rollout.__init__).parameters
    for name in ("anderson", "anderson_beta", "anderson_reg", "anderson_restart", "anderson_start"):
        assert sw[name].default == ro[name].default, name
    assert (sw["anderson"].default, sw["anderson_beta"].default, sw["anderson_reg"].default, sw["anderson_restart"].default,
            sw["anderson_start"].default) == (0, 1.0, 1e-10, 10.0, 0)
    nan = float("nan")
    # refused by gfv.anderson.check_args before the model or the pool is looked at (None stands in for both: no GPU)
    for bad in (dict(anderson=-1), dict(anderson=9), dict(anderson=2.5), dict(anderson=True),
                dict(anderson_beta=0.0), dict(anderson_beta=1.5), dict(anderson_beta=nan),
                dict(anderson_reg=-1e-12), dict(anderson_reg=nan),
                dict(anderson_restart=-1.0), dict(anderson_restart=0.5), dict(anderson_restart=1.0), dict(anderson_restart=nan),
                dict(anderson_start=-1), dict(anderson_start=1.5), dict(anderson_start=True)):
        with pytest.raises(ValueError, match="anderson"):
            Sweep(None, None, **{"anderson": 4, **bad})


def test_an_entry_must_fit_the_ring_stride():
    from gfv.anderson import check_ring_stride, count_dict, ring_bytes
    assert check_ring_stride([37, 133, 133], 133) == 133
    assert check_ring_stride({5: 4161, 2: 37}, 4161) == 4161
    assert check_ring_stride((), 1) == 1
    with pytest.raises(ValueError, match="entry 1 has 134 nodes"):
        check_ring_stride([37, 134, 4161], 133)
    with pytest.raises(ValueError, match="entry 7 has 4162 nodes"):
        check_ring_stride({3: 12, 7: 4162}, 4161)
    for stride in (0, -5):
        with pytest.raises(ValueError, match="ring stride"):
            check_ring_stride([1], stride)
    assert ring_bytes(8, 25479, 5) == 8 * 25479 * 12 * 12
    assert ring_bytes(2, 4161, 4) == 2 * 4161 * (2 * 4 + 2) * 12
    assert count_dict([3, 1, 0, 2], [0.5, 2.0, 4.0, 0.0]) == \
        {"accelerated": 3, "restarts": {"NONFINITE": 1, "GROWTH": 0, "SINGULAR": 2}, "last_depth": 4}
