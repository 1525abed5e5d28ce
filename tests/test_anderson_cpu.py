"""CPU: the host side of the Anderson acceleration of the rollout (gfv/anderson.py, csrc/anderson.hip): the two
entry points are declared, exported and bound; every bad argument is refused before anything touches a device; the Python
argument checks; and the numpy restatement of the algorithm (tests/anderson_ref.py) against itself on the rank-3 linear
contraction of the issue - AA(4) reaches a relative residual of 1e-5 by step index 6 where the plain iteration is above 1e-3 at
index 8, and nothing is NaN over 40 steps (the residual reaches exactly 0 on the way).  Nothing here touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import anderson_ref as R
import cases

NAMES = ("gfv_anderson_gram", "gfv_anderson_mix")


def test_anderson_entry_points_are_declared_exported_and_bound():
    from gfv import anderson as AA
    from gfv import cmdlist, lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    for name in NAMES:
        assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
        assert name not in cmdlist._QUERIES                                # they launch: part of a recorded list
    assert len(handle.gfv_anderson_gram.argtypes) == 25 and len(handle.gfv_anderson_mix.argtypes) == 17
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    define = lambda n: int(re.search(rf"#define {n} (\d+)", header).group(1))
    assert define("GFV_AA_MAX_DEPTH") == AA.MAX_DEPTH == R.MAX_DEPTH == 8
    assert define("GFV_AA_PARTIALS") == AA.PARTIALS == 8 * 9 // 2 + 8 + 2
    assert (define("GFV_AA_NONFINITE"), define("GFV_AA_GROWTH"), define("GFV_AA_SINGULAR")) == \
        (AA.NONFINITE, AA.GROWTH, AA.SINGULAR) == (R.NONFINITE, R.GROWTH, R.SINGULAR) == (1, 2, 4)


def _calls():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    assert p % 8 == 0
    gram_ptrs = ("uvp", "xb", "cb", "ce", "gp", "f_prev", "g_prev", "dF", "dG", "state", "r_prev", "gamma", "ws", "cnt", "table", "step")
    mix_ptrs = ("uvp", "f_cur", "cb", "ce", "gp", "dF", "dG", "gamma", "table", "step")
    ok = dict({n: p for n in gram_ptrs + mix_ptrs}, N=4, nc=1, B=2, K=8, m=4, reg=1e-10, restart=10.0, start=0, beta=1.0)

    def gram(**kw):
        a = {**ok, **kw}
        return lib.gfv_anderson_gram(a["uvp"], a["xb"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["m"], a["reg"],
                                     a["restart"], a["start"], a["f_prev"], a["g_prev"], a["dF"], a["dG"], a["state"], a["r_prev"],
                                     a["gamma"], a["ws"], a["cnt"], a["table"], a["K"], a["step"], None)

    def mix(**kw):
        a = {**ok, **kw}
        return lib.gfv_anderson_mix(a["uvp"], a["f_cur"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["m"], a["beta"],
                                    a["dF"], a["dG"], a["gamma"], a["table"], a["K"], a["step"], None)
    return gram, mix, gram_ptrs, mix_ptrs, p


def test_anderson_entry_points_reject_bad_arguments_before_touching_a_device():
    gram, mix, gram_ptrs, mix_ptrs, p = _calls()
    nan = float("nan")
    for fn, ptrs in ((gram, gram_ptrs), (mix, mix_ptrs)):
        for name in ptrs:
            assert fn(**{name: None}) == -1, name
        for name in ("N", "nc", "B", "K"):
            assert fn(**{name: 0}) == -1, name
            assert fn(**{name: -3}) == -1, name
        for m in (0, -1, 9, 64):
            assert fn(m=m) == -1, m
    for beta in (0.0, -0.5, 1.0000001, 2.0, nan, float("inf")):
        assert mix(beta=beta) == -1, beta
    for reg in (-1e-30, -1.0, nan):
        assert gram(reg=reg) == -1, reg
    for restart in (-1.0, nan, 1e-3, 0.5, 1.0):                            # 0 (off) and factors above 1 are the valid ones
        assert gram(restart=restart) == -1, restart
    for name in ("r_prev", "gamma", "ws"):                                 # the double buffers are 8-byte aligned
        assert gram(**{name: p + 4}) == -1, name
    assert mix(gamma=p + 4) == -1


def test_python_argument_checks():
    from gfv.anderson import check_args
    assert check_args() == (0, 1.0, 1e-10, 10.0, 0)
    assert check_args(8, 0.5, 0.0, 0.0, 3) == (8, 0.5, 0.0, 0.0, 3)
    assert check_args(1, 1, 1e-6, 1.5, 0) == (1, 1.0, 1e-6, 1.5, 0)
    nan = float("nan")
    for bad in (dict(anderson=-1), dict(anderson=9), dict(anderson=2.5), dict(anderson=True),
                dict(beta=0.0), dict(beta=-1.0), dict(beta=1.5), dict(beta=nan),
                dict(reg=-1e-12), dict(reg=nan),
                dict(restart=-1.0), dict(restart=nan), dict(restart=0.5), dict(restart=1.0),
                dict(start=-1), dict(start=1.5), dict(start=True)):
        with pytest.raises(ValueError):
            check_args(**{"anderson": 4, **bad})


@pytest.fixture(scope="module")
def problem():
    return R.BatchMap()


def test_problem_is_the_one_of_the_issue(problem):
    """rng order: U from standard_normal((3n, 3)), then x*, then the offset of x0; eigenvalues 0.9 / 0.8 / -0.7."""
    for n, seed, mp in zip(R.SIZES, R.SEEDS, problem.maps):
        rng = np.random.default_rng(seed)
        U, _ = np.linalg.qr(rng.standard_normal((3 * n, 3)))
        xs = rng.standard_normal(3 * n)
        x0 = xs + rng.standard_normal(3 * n)
        assert np.array_equal(U, mp.U) and np.array_equal(xs, mp.xs) and np.array_equal(x0.astype(np.float32).reshape(n, 3), mp.x0)
        M = U @ np.diag([0.9, 0.8, -0.7]) @ U.T if n < 200 else None
        if M is not None:
            x = rng.standard_normal(3 * n).astype(np.float32)
            want = (xs + M @ (x.astype(np.float64) - xs)).astype(np.float32)
            assert np.abs(mp(x.reshape(n, 3)).reshape(-1).astype(np.float64) - want).max() < 1e-6
    cb, ce, gcp = R.chunk_tables(R.SIZES)
    assert gcp.tolist() == [0, 1, 4, 70] and (ce - cb).max() == 64 and ce[0] - cb[0] == 37


def test_reference_aa4_converges_where_the_plain_iteration_does_not(problem):
    table, gammas, _ = R.iterate(problem, problem.x0, 40, R.AndersonRef(R.SIZES, 4))
    rel = table[:, :, 0].astype(np.float64) / table[:, :, 1]
    first = [int(np.argmax(rel[:, b] < 1e-5)) for b in range(3)]
    print("AA(4): first step index below 1e-5 per graph", first, "| restarts flagged", int((table[:, :, 3] != 0).sum()))
    assert all(bool((rel[:, b] < 1e-5).any()) and first[b] <= 6 for b in range(3)), first
    assert not np.isnan(table).any() and not np.isnan(gammas).any()
    assert bool((table[:, :, 0] == 0).any()), "the residual is expected to reach exactly 0 within 40 steps"
    assert table[0, :, 2].tolist() == [0, 0, 0] and table[1:5, 0, 2].tolist() == [1, 2, 3, 4]     # the ring fills one column a step
    plain, _, _ = R.iterate(problem, problem.x0, 9)
    rel_p = plain[:, :, 0].astype(np.float64) / plain[:, :, 1]
    print("plain iteration at step index 8:", rel_p[8].tolist())
    assert bool((rel_p[8] > 1e-3).all()), rel_p[8]
    assert bool((plain[:, :, 2] == 0).all())


@pytest.mark.parametrize("m,beta", [(8, 0.5), (3, 1.0), (1, 1.0)])
def test_reference_other_depths_stay_finite(problem, m, beta):
    table, gammas, x = R.iterate(problem, problem.x0, 40, R.AndersonRef(R.SIZES, m, beta=beta))
    assert not np.isnan(table).any() and not np.isnan(gammas).any() and np.isfinite(x).all()
    if m >= 3:      # the map has rank 3: a depth of 3 spans it (AA(1) is only asked to stay finite)
        assert float((table[-1, :, 0] / table[-1, :, 1]).max()) < 1e-5


def test_reference_decisions():
    """Growth, a NaN and a zero Gram matrix on one small graph, in the order of the kernel's decisions."""
    rng = np.random.default_rng(5)
    n = 9
    ref = R.AndersonRef([n], 4)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    g = x + np.float32(0.1) * rng.standard_normal((n, 3)).astype(np.float32)
    _, row, _ = ref.step(0, x, g)
    assert row[0, 2:].tolist() == [0, 0] and ref.st[0].has_prev == 1 and ref.st[0].cnt == 0
    g2 = g + np.float32(0.05) * rng.standard_normal((n, 3)).astype(np.float32)
    out, row, gam = ref.step(1, g, g2)
    assert row[0, 2:].tolist() == [1, 0] and ref.st[0].cnt == 1 and gam[0, 0] != 0 and not np.array_equal(out, g2)
    far = out + 20 * (g2 - g) / np.float32(0.05) * np.float32(0.1)
    _, row, gam = ref.step(2, out, far.astype(np.float32))                    # the residual grows 20 x and more
    assert row[0, 2:].tolist() == [0, R.GROWTH] and ref.st[0].cnt == 0 and ref.st[0].restarts == 1 and ref.st[0].has_prev == 1
    bad = g2.copy()
    bad[3, 1] = np.nan
    out, row, gam = ref.step(3, g2, bad)
    assert row[0, 2:].tolist() == [0, R.NONFINITE] and ref.st[0].has_prev == 0 and not np.isnan(gam).any()
    assert ref.st[0].restarts == 2
    for k in range(4, 8):                                                  # x = g: f = 0, every column 0
        out, row, gam = ref.step(k, g2, g2)
        assert np.array_equal(out, g2) and not np.isnan(gam).any() and not np.isnan(row).any()
        assert row[0, 2] == 0 and row[0, 3] in (0, R.SINGULAR)
    assert row[0, 3] == R.SINGULAR
