"""A numpy restatement of csrc/anderson.hip (Anderson acceleration of the steady-state rollout): the element
operations in fp32 and in the kernel's order, the sums in float64, the same decisions in the same order, the small system with
`numpy.linalg.cholesky` (is it positive definite?) and `numpy.linalg.solve`.  It is driven with (x_k, g_k) pairs - in the GPU
tests the device's own - and holds the state the kernels hold: f_prev, g_prev, the ring columns, (cnt, head, has_prev,
restarts) and r_prev per graph.

Also the test problem of the issue: the rank-3 linear contraction `G(x) = x* + M (x - x*)`, `M = U diag(0.9, 0.8, -0.7) U^T`.
"""
import numpy as np

MAX_DEPTH = 8
NONFINITE, GROWTH, SINGULAR = 1, 2, 4
SIZES = (37, 133, 4161)     # nodes per graph: a partial chunk, three chunks, 66 chunks (the fold wraps past lane 63)
SEEDS = (11, 12, 13)
EIGS = (0.9, 0.8, -0.7)
CHUNK = 64


def chunk_tables(sizes, chunk=CHUNK):
    """chunk_beg, chunk_end, gchunk_ptr of a batch of graphs with `sizes` nodes, as gfv/plan.py `_batch_part` builds them."""
    gp = np.concatenate(([0], np.cumsum(sizes))).tolist()
    cb, ce, gcp = [], [], [0]
    for b in range(len(sizes)):
        for st in range(gp[b], gp[b + 1], chunk):
            cb.append(st)
            ce.append(min(st + chunk, gp[b + 1]))
        gcp.append(len(cb))
    return np.array(cb, np.int32), np.array(ce, np.int32), np.array(gcp, np.int32)


class Rank3Map:
    """G(x) = x* + U diag(EIGS) U^T (x - x*) on the 3n values of one graph, evaluated in float64 and cast to fp32."""

    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        self.U, _ = np.linalg.qr(rng.standard_normal((3 * n, 3)))
        self.xs = rng.standard_normal(3 * n)
        self.x0 = (self.xs + rng.standard_normal(3 * n)).astype(np.float32).reshape(n, 3)
        self.d = np.array(EIGS)

    def __call__(self, x):
        e = x.astype(np.float64).reshape(-1) - self.xs
        return (self.xs + self.U @ (self.d * (self.U.T @ e))).astype(np.float32).reshape(self.n, 3)


class BatchMap:
    """The maps of a batch, on the concatenated rows [N, 3]."""

    def __init__(self, sizes=SIZES, seeds=SEEDS):
        self.maps = [Rank3Map(n, s) for n, s in zip(sizes, seeds)]
        self.ptr = np.concatenate(([0], np.cumsum(sizes))).tolist()
        self.x0 = np.concatenate([m.x0 for m in self.maps])

    def __call__(self, x):
        return np.concatenate([m(x[self.ptr[b]:self.ptr[b + 1]]) for b, m in enumerate(self.maps)])


def mix(g, f, dF, dG, gamma, beta):
    """uvp_new of one graph: g - (1-beta) f - sum_j gamma_j (dG_j - (1-beta) dF_j), j ascending over the slots with
    gamma_j != 0, in float64, rounded to fp32 once (csrc/anderson.hip anderson_mix_kernel)."""
    omb = 1.0 - float(beta)
    v = g.astype(np.float64)
    if omb != 0.0:
        v = v - omb * f.astype(np.float64)
    acc = np.zeros_like(v)
    for j in range(len(dG)):
        if gamma[j] == 0.0:
            continue
        t = dG[j].astype(np.float64)
        if omb != 0.0:
            t = t - omb * dF[j].astype(np.float64)
        acc = acc + gamma[j] * t
    return (v - acc).astype(np.float32)


class GraphState:
    def __init__(self, n, m):
        self.cnt = self.head = self.has_prev = self.restarts = 0
        self.r_prev = 0.0
        self.f_prev = np.zeros((n, 3), np.float32)
        self.g_prev = np.zeros((n, 3), np.float32)
        self.dF = np.zeros((m, n, 3), np.float32)
        self.dG = np.zeros((m, n, 3), np.float32)


class AndersonRef:
    def __init__(self, sizes, m, beta=1.0, reg=1e-10, restart=10.0, start=0):
        assert 1 <= m <= MAX_DEPTH
        self.sizes, self.m, self.beta, self.reg, self.restart, self.start = list(sizes), m, beta, reg, restart, start
        self.ptr = np.concatenate(([0], np.cumsum(sizes))).tolist()
        self.st = [GraphState(n, m) for n in sizes]
        self.systems = [None] * len(sizes)    # per graph: (slots, regularised matrix, right-hand side) of the last solve

    def gram(self, k, x, g):
        """The gram launch of step k on x, g [N, 3] fp32 -> (table row [B, 4] fp32, gamma [B, 8] float64)."""
        B, m = len(self.sizes), self.m
        row = np.zeros((B, 4), np.float32)
        gamma = np.zeros((B, MAX_DEPTH), np.float64)
        for b, s in enumerate(self.st):
            gb = g[self.ptr[b]:self.ptr[b + 1]].astype(np.float32)
            f = gb - x[self.ptr[b]:self.ptr[b + 1]].astype(np.float32)          # fp32
            has_prev, head, cnt = s.has_prev, s.head, s.cnt
            if has_prev:
                s.dF[head] = f - s.f_prev
                s.dG[head] = gb - s.g_prev
            s.f_prev, s.g_prev = f.copy(), gb.copy()
            mk = min(cnt + has_prev, m)
            slots = sorted((head - a) % m for a in range(mk)) if has_prev else []
            f64 = f.astype(np.float64).reshape(-1)
            with np.errstate(all="ignore"):
                ff = float(f64 @ f64)
                gg = float(gb.astype(np.float64).reshape(-1) @ gb.astype(np.float64).reshape(-1))
                rf = np.sqrt(ff)
            depth = flags = 0
            n_cnt, n_prev = mk, 1
            n_head = (head + 1) % m if has_prev else head
            self.systems[b] = None
            if not np.isfinite(ff):
                flags, n_cnt, n_prev, n_head = NONFINITE, 0, 0, head
                s.restarts += 1
            elif has_prev and self.restart > 0 and rf > self.restart * s.r_prev:
                flags, n_cnt, n_head = GROWTH, 0, head
                s.restarts += 1
            elif mk > 0 and k >= self.start:
                D = s.dF[slots].astype(np.float64).reshape(mk, -1)
                A = D @ D.T
                rhs = D @ f64
                Areg = A + (self.reg * np.trace(A) / mk) * np.eye(mk)
                ok = True
                try:
                    np.linalg.cholesky(Areg)
                    sol = np.linalg.solve(Areg, rhs)
                    ok = bool(np.isfinite(sol).all())
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    depth = mk
                    gamma[b, slots] = sol
                    self.systems[b] = (slots, Areg, rhs)
                else:
                    flags, n_cnt, n_head = SINGULAR, 0, head
                    s.restarts += 1
            s.cnt, s.head, s.has_prev, s.r_prev = n_cnt, n_head, n_prev, float(rf)
            with np.errstate(all="ignore"):
                row[b] = (np.float32(rf), np.float32(np.sqrt(gg)), depth, flags)
        return row, gamma

    def mix(self, g, row, gamma):
        """The mix launch with `gamma` [B, 8] (the reference's own or the device's) -> the new uvp_node [N, 3] fp32; the rows of
        a graph with depth 0 are g's bits."""
        out = g.astype(np.float32).copy()
        for b, s in enumerate(self.st):
            if row[b, 2] > 0:
                sl = slice(self.ptr[b], self.ptr[b + 1])
                out[sl] = mix(g[sl], s.f_prev, s.dF, s.dG, gamma[b, :self.m], self.beta)
        return out

    def step(self, k, x, g):
        row, gamma = self.gram(k, x, g)
        return self.mix(g, row, gamma), row, gamma


def iterate(G, x0, steps, ref=None, sizes=SIZES):
    """x_{k+1} = the accelerated (ref) or plain (ref None) iterate of G from x0 -> (table [steps, B, 4], gammas, final x).
    Without `ref` the table is that of an AndersonRef that never mixes (its columns 0, 1 are || f ||, || g ||)."""
    probe = ref if ref is not None else AndersonRef(sizes, 1, start=steps + 1)
    x = x0.copy()
    rows, gammas = [], []
    for k in range(steps):
        g = G(x)
        x, row, gamma = probe.step(k, x, g)
        rows.append(row)
        gammas.append(gamma)
    return np.stack(rows), np.stack(gammas), x
