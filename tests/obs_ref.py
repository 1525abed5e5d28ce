"""The observation term (include/gfv.h "Observation term", gfv/observe.py), restated in numpy from the header's formulas.

Per element (node i of graph b, channel c):  pred = (phi * uvp_dim[b, c]) * sigma[b, c];  e = pred - t;  an element with weight 0
is skipped before its target enters any arithmetic.  `dtype` is the precision of pred and e: np.float32 is what the kernels do,
np.float64 what a float64 autograd of the same objective does (tests/test_observe_cpu.py).  Products w * (e * e), the row sums
((c0 + c1) + c2) and every sum behind them are float64, in the order of tests/chunk_sums_ref.py.
Per graph:  obs = float32(S / W) (0 when W == 0; `exact` leaves the rounding out);  tot = (wp * l3 + wc * l0 + wm * l1 + wm * l2)
+ w_obs * obs;  loss = mean log tot;  inv = 1 / (tot * B);  gloss = (wc, wm, wm, wp) * inv;  gobs = w_obs * inv.
Gradient:  g_dec[i, c] += gobs_b * (2 w e scale / W_b) * (1 - tanh(dec / 10)^2), scale = uvp_dim * sigma, where w != 0 and the
boundary condition lets gradient through."""
import numpy as np

from chunk_sums_ref import chunk_sums, graph_sums

f64 = np.float64
NORMAL, INFLOW, OUTFLOW, WALL, PRESS, INWALL = range(6)      # node types (csrc/fvm.hip)


def misfit(phi3, target, weight, uvp_dim, sigma, row_graph, dtype=np.float32):
    """-> e [N, 3] of `dtype` (0 where the weight is 0: the target is not touched there), observed [N, 3] bool."""
    phi3, d, s = (np.asarray(a, dtype=dtype) for a in (phi3, np.asarray(uvp_dim)[row_graph], np.asarray(sigma)[row_graph]))
    pred = (phi3 * d) * s
    assert pred.dtype == dtype
    observed = np.asarray(weight) != 0
    t = np.where(observed, np.asarray(target, dtype=dtype), dtype(0))
    return np.where(observed, pred - t, dtype(0)).astype(dtype), observed


def row_terms(e, weight):
    """The two sums per row, float64: ((q0 + q1) + q2) with q = w * (e * e), and ((w0 + w1) + w2)."""
    w, e = np.asarray(weight).astype(f64), np.asarray(e).astype(f64)
    q = w * (e * e)
    return np.stack([(q[:, 0] + q[:, 1]) + q[:, 2], (w[:, 0] + w[:, 1]) + w[:, 2]], axis=1)


def sums(terms, chunk_beg, chunk_end, gchunk_ptr, N):
    """-> the chunk workspace [n_chunks, 2] and the per-graph (S_b, W_b) [B, 2]."""
    partial = chunk_sums(terms, chunk_beg, chunk_end, N)
    return partial, graph_sums(partial, gchunk_ptr)


def record(SW, losses, loss_weights, w_obs, exact=False):
    """SW [B, 2]; losses [B, 4] (cont, mom_x, mom_y, press); loss_weights (w_cont, w_mom, w_press) -> dict of float64 arrays."""
    SW, l = np.asarray(SW, dtype=f64), np.asarray(losses).astype(f64)
    wc, wm, wp = (f64(v) for v in loss_weights)
    B = SW.shape[0]
    S, W = SW[:, 0], SW[:, 1]
    obs = np.where(W == 0, 0.0, S / np.where(W == 0, 1.0, W))
    if not exact:
        obs = obs.astype(np.float32).astype(f64)
    pde = wp * l[:, 3] + wc * l[:, 0] + wm * l[:, 1] + wm * l[:, 2]
    tot = pde + f64(w_obs) * obs
    inv = 1.0 / (tot * B)
    return dict(obs=obs, W=W, pde=pde, tot=tot, loss=f64(np.log(tot).sum() / B), gobs=f64(w_obs) * inv,
                gloss=np.stack([wc * inv, wm * inv, wm * inv, wp * inv], axis=1))


def passes(node_type):
    """[N, 3] bool: where phi_bwd lets gradient through - u, v not at WALL / INFLOW / PRESS / INWALL nodes, p not at PRESS."""
    nt = np.asarray(node_type)
    uv = ~np.isin(nt, (WALL, INFLOW, PRESS, INWALL))
    return np.stack([uv, uv, nt != PRESS], axis=1)


def gdec_increment(rec, e, weight, dec, uvp_dim, sigma, row_graph, node_type):
    """-> the increment of g_dec [N, 3] float64 and `contributes` [N, 3] bool."""
    w, e, dec = (np.asarray(a).astype(f64) for a in (weight, e, dec))
    scale = np.asarray(uvp_dim).astype(f64)[row_graph] * np.asarray(sigma).astype(f64)[row_graph]
    contributes = (np.asarray(weight) != 0) & passes(node_type)
    W = np.where(rec["W"] == 0, 1.0, rec["W"])[row_graph][:, None]
    th = np.tanh(dec / 10.0)
    inc = rec["gobs"][row_graph][:, None] * (2.0 * w * e * scale / W) * (1.0 - th * th)
    return np.where(contributes, inc, 0.0), contributes
