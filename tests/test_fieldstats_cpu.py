"""CPU: the host side of the field statistics (gfv/fieldstats.py, csrc/fieldstats.hip): the rule - tests/fieldstats_ref.py, the
reference the GPU tests compare the kernel with - against two-pass float64 statistics and on hand-made windows, the argument
refusals, and the C ABI: the entry point is declared, exported and bound, and every bad argument is refused before anything
touches a device.  Nothing here touches a GPU.

The bounds of the accuracy test are derived, not measured.  The sums run over x - K with K the first sample, so every term is of
the size of the fluctuation f, not of the mean: S1 is a sum of n <= 64 doubles (n roundings of 2^-53 relative to a partial sum
<= n f), S2 likewise with one more rounding per product; mean = K + S1 / n adds two roundings relative to max|x|; the variance
S2 / n - (S1 / n)^2 subtracts two terms each <= max(S2 / n) up to a factor 2.  Altogether below (2 n + 8) 2^-53 < 1.6e-14 relative
to max|x| (mean) and to max(S2 / n) (variance, covariance): 1e-12 leaves a factor 60."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cases
import fieldstats_ref as R

f32, f64 = np.float32, np.float64


def _samples(n=64, rows=301, seed=20250612):
    """fp32 samples [n, rows, 3] whose mean is 1e3 times the fluctuation, u and v correlated."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(1.0, 10.0, (rows, 3)) * rng.choice([-1.0, 1.0], (rows, 3))
    fl = 1e-3 * np.abs(mean) * rng.standard_normal((n, rows, 3))
    fl[:, :, 1] = 0.6 * fl[:, :, 0] * (mean[:, 1] / mean[:, 0]) + 0.8 * fl[:, :, 1]
    return (mean + fl).astype(f32)


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_the_rule_against_two_pass_float64_statistics(n):
    x = _samples(n)
    if n >= 7:
        x64 = x.astype(f64)
        assert float((np.abs(x64.mean(0)) / x64.std(0)).min()) > 300       # the mean is ~1e3 times the fluctuation, every channel
    ref = R.over(x, range(1, n + 1), x.shape[1])
    assert ref.rec[R.N] == n and ref.rec[R.LAST] == n
    s2n = float((ref.sums[3:6] / n).max())
    # the reference itself stays inside the bounds
    R.check_against_two_pass(ref.moments(), x, s2n, f"reference, n = {n}")
    # the module's own float64 plumbing (what FieldStats.read() forms from the raw state) on the same raw state
    from gfv.fieldstats import moments
    got = moments(n, torch.from_numpy(ref.sums), torch.from_numpy(ref.aux))
    R.check_against_two_pass({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}, x, s2n,
                           f"moments(), n = {n}")
    assert got["n"] == n and got["mean"].dtype == torch.float64 and tuple(got["mean"].shape) == (x.shape[1], 3)
    assert tuple(got["cov_uv"].shape) == (x.shape[1],) and got["min"].dtype == torch.float32
    want = ref.moments()
    for k in ("mean", "var", "cov_uv", "min", "max"):
        assert got[k].numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k      # the same formulas: the same bits
    with pytest.raises(RuntimeError, match="n == 0"):
        moments(0, torch.from_numpy(ref.sums), torch.from_numpy(ref.aux))


def _run(window, clocks, rows=5):
    rng = np.random.default_rng(7)
    ref = R.FieldStatsRef(rows, **window)
    fields = [rng.standard_normal((rows, 12)).astype(f32) for _ in clocks]
    return ref, fields, [ref.launch(f, c) for f, c in zip(fields, clocks)]


def test_the_window_rule():
    T, F = True, False
    ref, fields, taken = _run(dict(start=3, stride=2, stop=-1), range(1, 10))
    assert taken == [F, F, T, F, T, F, T, F, T] and ref.rec[R.N] == 4 and ref.rec[R.LAST] == 9
    _, _, taken = _run(dict(start=3, stride=2, stop=7), range(1, 10))
    assert taken == [F, F, T, F, T, F, F, F, F]                            # stop is exclusive: 7 itself is not sampled
    _, _, taken = _run(dict(start=0, stride=1, stop=0), range(0, 3))
    assert taken == [F, F, F]
    # an unchanged clock samples once; state and n stay
    ref, fields, taken = _run(dict(start=1, stride=1), [1, 1, 1, 2, 2, 3])
    assert taken == [T, F, F, T, F, T] and ref.rec[R.N] == 3
    once = R.over([fields[0], fields[3], fields[5]], [1, 2, 3], 5, start=1, stride=1)
    assert once.sums.tobytes() == ref.sums.tobytes() and once.aux.tobytes() == ref.aux.tobytes()
    # a stride < 1 is read as 1
    for stride in (0, -5):
        _, _, taken = _run(dict(start=2, stride=stride), range(1, 6))
        assert taken == [F, T, T, T, T], stride
    # enabled = 0 pauses; the clock is still followed (last moves), so re-enabling does not sample a clock already seen
    ref, fields, _ = _run(dict(start=1, stride=1, enabled=0), [1, 2])
    assert ref.rec[R.N] == 0 and ref.rec[R.LAST] == 2
    ref.rec[R.ENABLED] = 1
    assert ref.launch(fields[0], 2) is False and ref.launch(fields[1], 3) is True and ref.rec[R.N] == 1
    assert (ref.aux[0:3].T == fields[1][:, 0:3]).all() and (ref.sums == 0).all() and not np.signbit(ref.sums).any()
    # a reset starts over from whatever the state holds: the first sample overwrites every element
    ref.sums[:], ref.aux[:] = np.nan, np.nan
    ref.reset()
    assert ref.rec[R.LAST] == -1 and ref.rec[R.N] == 0
    assert ref.launch(fields[0], 3) is True                                # (the same clock again: last was reset)
    assert (ref.aux[3:6].T == fields[0][:, 0:3]).all() and (ref.sums == 0).all() and not np.signbit(ref.sums).any()
    # a clock that runs backwards (an owner's reset) is followed like any change
    ref, _, taken = _run(dict(start=1, stride=1), [1, 2, 1])
    assert taken == [T, T, T] and ref.rec[R.LAST] == 1
    assert ref.rec[R.COUNTER] == 0 and ref.rec[7] == 0


def test_nan_samples_leave_the_extremes_and_poison_the_sums():
    x = np.array([[[1, 2, 3]], [[np.nan, 5, 1]], [[0.5, np.nan, 4]]], dtype=f32)
    ref = R.over(x, [1, 2, 3], 1)
    assert ref.aux[3:6, 0].tolist() == [0.5, 2.0, 1.0] and ref.aux[6:9, 0].tolist() == [1.0, 5.0, 4.0]
    assert np.isnan(ref.sums[[0, 1, 3, 4, 6], 0]).all() and ref.sums[2, 0] == -1.0 and ref.sums[5, 0] == 5.0
    # a NaN first sample: the shift is NaN (every sum stays NaN), the extremes recover with the next sample
    ref = R.over(x[[1, 0]], [1, 2], 1)
    assert np.isnan(ref.aux[0, 0]) and ref.aux[3, 0] == 1.0 and ref.aux[6, 0] == 1.0 and np.isnan(ref.sums[0, 0])


def test_argument_refusals_need_no_device():
    from gfv.fieldstats import NO_STOP, FieldStats, check_field, check_field_stats_args
    from gfv.march import MarchStep
    from gfv.rollout import check_field_stats
    assert check_field_stats_args() == (1, 1, NO_STOP, 1)
    assert check_field_stats_args(1, 3, 10, False) == (1, 3, 10, 0)
    for bad in (dict(start=-1), dict(start=0), dict(start=1.5), dict(start=True), dict(stride=0), dict(stride=-2), dict(stride=2.0), dict(stop=-1),
                dict(stop=3.5), dict(stop=False), dict(start=2 ** 31), dict(stop=2 ** 31), dict(enabled="yes"), dict(start=None)):
        with pytest.raises(ValueError):
            check_field_stats_args(**bad)
        if "enabled" not in bad:
            with pytest.raises(ValueError):
                FieldStats(**bad)
    fs = FieldStats(start=3, stride=2, stop=9)
    assert (fs.start, fs.stride, fs.stop, fs.enabled) == (3, 2, 9, True)
    fs.set_window(stride=4)                                                 # before it is attached: the host words alone
    assert (fs.start, fs.stride, fs.stop, fs.enabled) == (3, 4, 9, True)
    fs.set_window(stop=None, enabled=False)
    assert (fs.start, fs.stride, fs.stop, fs.enabled) == (3, 4, None, False)
    with pytest.raises(ValueError, match="stride"):
        fs.set_window(start=5, stride=0)
    assert fs.start == 3                                                    # checked before anything changes
    for call in (fs.read, fs.count, fs.raw, fs.reset):
        with pytest.raises(RuntimeError, match="not attached"):
            call()
    # the field tensor
    assert check_field.__doc__ and check_field_stats.__doc__
    for bad in (torch.zeros(4, 11), torch.zeros(4, 12, dtype=torch.float64), torch.zeros(12, 8).t(), torch.zeros(0, 12), None):
        with pytest.raises(ValueError):
            check_field(bad)
    with pytest.raises(ValueError, match="GPU"):
        check_field(torch.zeros(4, 12))                                     # a CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        FieldStats().attach(object(), torch.zeros(4, 12), torch.zeros(1, dtype=torch.int32))
    # the owners
    check_field_stats(None, 3)
    check_field_stats(FieldStats(), 0)
    with pytest.raises(ValueError, match="anderson"):
        check_field_stats(FieldStats(), 2)
    with pytest.raises(ValueError, match="FieldStats"):
        check_field_stats(dict(start=1), 0)
    with pytest.raises(ValueError, match="field_stats"):
        MarchStep(None, None, field_stats=dict(start=1))                    # refused before the model or a device is looked at


def test_field_stats_entry_point_is_declared_exported_and_bound():
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    name = "gfv_field_stats_update"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert len(getattr(handle, name).argtypes) == 7
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert name not in cmdlist._QUERIES                                    # it launches: part of a recorded list
    for macro, value in (("RECORD", lib.FIELD_STATS_RECORD), ("SUMS", lib.FIELD_STATS_SUMS), ("AUX", lib.FIELD_STATS_AUX)):
        assert int(re.search(rf"#define GFV_FIELD_STATS_{macro} (\d+)", header).group(1)) == value == getattr(R, macro)
    from gfv import fieldstats as F
    assert [F.START, F.STRIDE, F.STOP, F.LAST, F.N_SAMPLES, F.COUNTER, F.ENABLED] == list(range(7)) \
        == [R.START, R.STRIDE, R.STOP, R.LAST, R.N, R.COUNTER, R.ENABLED]


def test_field_stats_update_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 16 == 0
    ok = dict(xb=p, N=4, clock=p, rec=p, sums=p, aux=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_field_stats_update(a["xb"], a["N"], a["clock"], a["rec"], a["sums"], a["aux"], None)
    for name in ("xb", "clock", "rec", "sums", "aux"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=-3) == -1
    assert call(xb=p + 4) == -1 and call(xb=p + 8) == -1                    # the rows are read 16 bytes at a time
    assert bytes(buf) == bytes(8 * 64)                                     # nothing was written
