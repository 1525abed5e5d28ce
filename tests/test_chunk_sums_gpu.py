"""GPU: the summation order of the chunked double sums is a contract (csrc/gfv_reduce.h, "Summation order").

`gfv_rollout_advance`, `gfv_sweep_advance` and `gfv_eval_collect` are called directly on synthetic arrays and compared BIT FOR BIT
with tests/chunk_sums_ref.py, a numpy restatement of that paragraph: the per-chunk doubles the launch leaves in its workspace, the
fp32 norms it writes, the arrival counter back at zero, and a second launch on the same inputs against the first.

One shape (chunk_sums_ref.tables): 3 graphs of 1, 6 and 70 chunks - 77 chunks, no multiple of the 4 waves of a workgroup; one graph
with more than 64 chunks, so that a lane of the fold takes two - 1 to 100 rows per chunk (a lane adds no row, one, or two), the last
chunk's end past N.  Evaluation: the middle graph has no target.  Sweep: the middle slot is already done.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import chunk_sums_ref as R

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def case():
    """Tables, fields and the numpy sums: computed once, shared by the three tests, left unchanged."""
    cb, ce, gcp, N, row_graph = R.tables()
    f = R.fields(N, 20240607)
    c = dict(cb=cb, ce=ce, gcp=gcp, N=N, B=len(gcp) - 1, nc=len(cb), row_graph=row_graph, **f)
    chunk_graph = np.repeat(np.arange(c["B"]), np.diff(gcp))
    c["chunk_graph"] = chunk_graph
    c["adv_partial"] = R.chunk_sums(R.diff_norm_terms(f["uvp"], f["x_backup"][:, 0:3]), cb, ce, N)
    c["adv_norms"] = R.norm32(R.graph_sums(c["adv_partial"], gcp))
    return c


def _tables_dev(c):
    return _dev(c["cb"]), _dev(c["ce"]), _dev(c["gcp"])


def _rollout(c):
    from gfv import lib as L
    K_max, k0 = 4, 2
    cb, ce, gcp = _tables_dev(c)
    uvp, xb, losses = _dev(c["uvp"]), _dev(c["x_backup"]), _dev(c["losses"])
    x = torch.full_like(xb, 7.0)
    partial = torch.full((c["nc"], 2), -1.0, dtype=torch.float64, device="cuda")
    history = torch.full((K_max, c["B"], 6), -3.0, dtype=torch.float32, device="cuda")
    state = torch.tensor([k0, 0], dtype=torch.int32, device="cuda")
    L.check(L.load().gfv_rollout_advance(
        uvp.data_ptr(), xb.data_ptr(), x.data_ptr(), c["N"], cb.data_ptr(), ce.data_ptr(), gcp.data_ptr(), c["nc"], c["B"],
        losses.data_ptr(), partial.data_ptr(), history.data_ptr(), K_max, state.data_ptr(), L.stream_ptr()), "gfv_rollout_advance")
    torch.cuda.synchronize()
    return dict(partial=partial.cpu().numpy(), history=history.cpu().numpy(), state=state.tolist(), xb=xb.cpu().numpy(),
                x=x.cpu().numpy(), k0=k0)


def test_rollout_advance_bits(case):
    c = case
    o = _rollout(c)
    assert o["state"] == [o["k0"] + 1, 0]                                  # the step advanced, the arrival counter back at zero
    assert _same_bits(o["partial"], c["adv_partial"])
    h = o["history"]
    assert _same_bits(h[o["k0"], :, 4:6], c["adv_norms"])
    assert _same_bits(h[o["k0"], :, 0:4], c["losses"])
    assert (np.delete(h, o["k0"], axis=0) == -3.0).all()
    want = c["x_backup"].copy()
    want[:, 0:3] = c["uvp"]
    assert _same_bits(o["xb"], want) and _same_bits(o["x"], want)
    again = _rollout(c)
    for k in ("partial", "history", "xb", "x"):
        assert _same_bits(o[k], again[k]), k
    assert again["state"] == o["state"]


SLOTS0 = np.array([[3, 1, 0, 0], [7, 2, 1, 0], [4, 0, 0, 0]], dtype=np.int32)     # the middle slot is done
TOL, MIN_STEPS, MAX_STEPS, PATIENCE = 1e30, 1, 5, 2                               # (every finite ratio is below tol)


def _sweep(c):
    from gfv import lib as L
    cb, ce, gcp = _tables_dev(c)
    B = c["B"]
    uvp, xb, losses = _dev(c["uvp"]), _dev(c["x_backup"]), _dev(c["losses"])
    x = torch.full_like(xb, 7.0)
    state3 = torch.full((c["N"], 3), 7.0, dtype=torch.float32, device="cuda")
    partial = torch.full((c["nc"], 2), -1.0, dtype=torch.float64, device="cuda")
    last = torch.full((B, 6), -3.0, dtype=torch.float32, device="cuda")
    ctl = np.zeros(4, dtype=np.int32)
    ctl[0:1] = np.array([TOL], dtype=np.float32).view(np.int32)
    ctl[1:4] = (MIN_STEPS, MAX_STEPS, PATIENCE)
    ctl, slots = _dev(ctl), _dev(SLOTS0)
    state = torch.tensor([10, 0], dtype=torch.int32, device="cuda")
    words = 1 + 2 * B
    host, devp = C.POINTER(C.c_int32)(), C.c_void_p()
    L.check(L.load(raw=True).gfv_sweep_mirror_create(words, C.byref(host), C.byref(devp)), "gfv_sweep_mirror_create")
    try:
        L.check(L.load().gfv_sweep_advance(
            uvp.data_ptr(), xb.data_ptr(), x.data_ptr(), c["N"], cb.data_ptr(), ce.data_ptr(), gcp.data_ptr(), c["nc"], B,
            losses.data_ptr(), partial.data_ptr(), ctl.data_ptr(), slots.data_ptr(), last.data_ptr(), state3.data_ptr(),
            devp.value, state.data_ptr(), L.stream_ptr()), "gfv_sweep_advance")
        torch.cuda.synchronize()
        mirror = [int(host[i]) for i in range(words)]
    finally:
        torch.cuda.synchronize()
        L.load(raw=True).gfv_sweep_mirror_free(host)
    return dict(partial=partial.cpu().numpy(), last=last.cpu().numpy(), slots=slots.cpu().numpy(), state=state.tolist(),
                xb=xb.cpu().numpy(), x=x.cpu().numpy(), state3=state3.cpu().numpy(), mirror=mirror)


def test_sweep_advance_bits(case):
    c = case
    o = _sweep(c)
    live = SLOTS0[:, 2] == 0
    assert o["state"] == [11, 0]
    want_partial = c["adv_partial"].copy()
    want_partial[~live[c["chunk_graph"]]] = 0.0                              # a frozen slot's chunks sum nothing
    assert _same_bits(o["partial"], want_partial)
    assert _same_bits(o["last"][live, 4:6], c["adv_norms"][live])
    assert _same_bits(o["last"][live, 0:4], c["losses"][live])
    assert (o["last"][~live] == -3.0).all()
    # the slots: rel = dn / un in fp32 against tol; slot 0 converges on this step (done 1), slot 2 runs out of steps (done 2)
    rel = c["adv_norms"][:, 0] / c["adv_norms"][:, 1]
    want_slots = SLOTS0.copy()
    for b in np.flatnonzero(live):
        age, streak = SLOTS0[b, 0] + 1, (SLOTS0[b, 1] + 1 if rel[b] < np.float32(TOL) else 0)
        done = 1 if streak >= PATIENCE and age >= MIN_STEPS else 2 if age >= MAX_STEPS else 0
        want_slots[b, 0:3] = (age, streak, done)
    assert np.array_equal(o["slots"], want_slots)
    assert o["mirror"] == [11] + [int(v) for b in range(c["B"]) for v in (want_slots[b, 2], want_slots[b, 0])]
    row_live = live[c["row_graph"]]
    want = c["x_backup"].copy()
    want[row_live, 0:3] = c["uvp"][row_live]
    assert _same_bits(o["xb"], want) and _same_bits(o["x"], want) and _same_bits(o["state3"], want[:, 0:3])
    again = _sweep(c)
    for k in ("partial", "last", "slots", "xb", "x", "state3"):
        assert _same_bits(o[k], again[k]), k
    assert again["state"] == o["state"] and again["mirror"] == o["mirror"]


HAS_TARGET = [1, 0, 1]
ENTRY = [4, 0, 2]
N_ENTRIES = 5


def _eval(c):
    from gfv import lib as L
    cb, ce, gcp = _tables_dev(c)
    B = c["B"]
    uvp, xr, tgt, losses = _dev(c["uvp"]), _dev(c["x_backup"]), _dev(c["target"]), _dev(c["losses"])
    partial = torch.full((c["nc"], 12), -1.0, dtype=torch.float64, device="cuda")
    table = torch.full((N_ENTRIES, L.EVAL_RECORD), -3.0, dtype=torch.float32, device="cuda")
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    ent, flg = (C.c_int32 * B)(*ENTRY), (C.c_int32 * B)(*HAS_TARGET)
    L.check(L.load().gfv_eval_collect(
        uvp.data_ptr(), xr.data_ptr(), tgt.data_ptr(), c["N"], cb.data_ptr(), ce.data_ptr(), gcp.data_ptr(), c["nc"], B,
        losses.data_ptr(), C.addressof(ent), C.addressof(flg), table.data_ptr(), N_ENTRIES, partial.data_ptr(), counter.data_ptr(),
        L.stream_ptr()), "gfv_eval_collect")
    torch.cuda.synchronize()
    return dict(partial=partial.cpu().numpy(), table=table.cpu().numpy(), counter=counter.tolist())


def test_eval_collect_bits(case):
    c = case
    has = np.array(HAS_TARGET, dtype=bool)
    want_partial = R.chunk_sums(R.eval_terms(c["uvp"], c["x_backup"][:, 0:3], c["target"], has[c["row_graph"]]), c["cb"], c["ce"], c["N"])
    want = _bits(R.norm32(R.graph_sums(want_partial, c["gcp"]))).copy()      # [B, 12]: table columns 4 - 15
    want[~has, 6:] = NAN_BITS
    o = _eval(c)
    assert o["counter"] == [0, 0, 0, 0]
    assert _same_bits(o["partial"], want_partial)
    assert np.array_equal(_bits(o["table"])[ENTRY, 4:16], want)
    assert _same_bits(o["table"][ENTRY, 0:4], c["losses"])
    untouched = [e for e in range(N_ENTRIES) if e not in ENTRY]
    assert (o["table"][untouched] == -3.0).all()
    again = _eval(c)
    assert _same_bits(o["partial"], again["partial"]) and _same_bits(o["table"], again["table"]) and again["counter"] == o["counter"]
