"""Row-by-row checks of the MLP backward chains (csrc/colchain_kernel.h, csrc/cbwd.hip, the row-owner chain) against float64
autograd, shared by tests/test_chain_rows_cpu.py, tests/test_chain_rows_gpu.py and tests/chain_rows_worker.py.

The column-owner kernels quantise g3 / gz2 / gz1 as fp16 hi + lo behind ONE power-of-two scale per tile (64 rows in the
persistent kernel, 32 in the small-tile one; DESIGN.md "Scales without a pass over the data").  A global max|a - b| / max|b|
cannot see what that does to a small row beside a large one, so every row tensor is judged row by row here,

    e_i = max_j |out_ij - ref_ij| / max_j |ref_ij|,

under row layouts (a power-of-two multiplier per row of the incoming gradient, so the inputs stay exact) that put different
scales into neighbouring tiles, into one tile, and beyond the persistent kernel's scale cap.  Rows whose whole neighbourhood
carries one multiplier must keep the project's 1e-5; every other row gets, on top of it, the quantisation floor of the scale the
kernel REPORTS for the row's group (`gscale`: a quarter of the fragment scale),

    F_i = 2^-24 L1 / (s_i max_j |ref_ij|),       s_i = 4 gscale[slot][i // 16],

one fp16 subnormal quantum of the last fragment set that feeds the tensor, carried through the chain layer that follows (L1:
its largest column 1-norm, x 1.13 where a GELU' follows).  The floor is derived from the format, not measured; two conditions
keep it from excusing everything: the exponent-0 rows of `mixed` must have F_i < 1e-6, and no reported g3 scale may exceed
what the no-overflow bound allows (s max|g3| <= 2^15).

Backends share one interface (`run(case, layout) -> Out`): `Torch32` (fp32 eager autograd, no scales: flat tolerance on every
row), `Emu(tile)` (float64 arithmetic with the kernels' scale rules and fp16 hi + lo fragments) and `Gpu(family)`.

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import collections
import math

import torch
import torch.nn.functional as F

TOL_ROW = 1e-5          # the project's tolerance, per row
TOL_SUM = 1e-5          # dgamma / dbeta, weight and bias gradients: global rel (sums the large rows rightly dominate)
Q16 = 2.0 ** -24        # one fp16 subnormal quantum
GELU_SLOPE = 1.13       # max |gelu'| (csrc/colchain_kernel.h)
SHAPES = ("edge", "node", "enc")
LAYOUTS = ("flat", "zigzag", "stairs_down", "stairs_up", "cliff_down", "cliff_up", "mixed", "zeros")
REGION = 192
STAIRS = 16            # steps of a staircase: launches of up to 3072 rows hold one
CLIFF_EXP = -40
MIXED_PERIOD = 21
# row tensors a launch of each family leaves (the persistent kernel neither saves g3 nor gz2)
ROWS_COL = {"edge": ("ge", "gz1"), "node": ("gx", "gnbm", "gz1"), "enc": ("gz1",)}
ROWS_ALL = {k: v + ("gz2", "g3") for k, v in ROWS_COL.items()}
FINAL = {"edge": ("ge",), "node": ("gx", "gnbm"), "enc": ("gz1",)}      # what ROWACC lines report
SUMS = ("W3", "b3", "W2", "b2", "W1", "b1", "gamma", "beta")

Check = collections.namedtuple("Check", "name ok value bound")
Out = collections.namedtuple("Out", "rows sums gscale finite status")


# ---- row layouts ---------------------------------------------------------------------------------------------------------------
def exponents(layout, M):
    """Per row: the exponent of its power-of-two multiplier (int64) and whether the row is zeroed."""
    i = torch.arange(M)
    zero = torch.zeros(M, dtype=torch.bool)
    if layout == "flat":
        e = torch.zeros(M, dtype=torch.int64)
    elif layout == "zigzag":
        e = torch.tensor([0, 3, -1, 2, -2])[(i // REGION) % 5]
    elif layout == "stairs_down":           # (a staircase starts again after STAIRS steps: float32 rows must stay normal numbers)
        e = -6 * ((i // REGION) % STAIRS)
    elif layout == "stairs_up":
        e = 6 * ((i // REGION) % STAIRS)
    elif layout == "cliff_down":
        e = torch.where(i < int(0.45 * M), 0, CLIFF_EXP)
    elif layout == "cliff_up":
        e = torch.where(i >= M - int(0.45 * M), 0, CLIFF_EXP)
    elif layout == "mixed":
        e = -(i % MIXED_PERIOD)
    elif layout == "zeros":
        e = torch.zeros(M, dtype=torch.int64)
        for b in (0, M // 2, M - 200):
            zero[max(b, 0):min(b + 200, M)] = True
    else:
        raise KeyError(layout)
    return e.to(torch.int64), zero


def multipliers(layout, M):
    e, zero = exponents(layout, M)
    m = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    m[zero] = 0.0
    return m


def interior(mult, reach=63):
    """Rows all of whose neighbours within +-reach carry the same multiplier: any tile of up to reach + 1 consecutive rows that
    holds such a row is uniform, whatever the tile alignment."""
    M = mult.numel()
    change = torch.ones(M, dtype=torch.bool)
    change[1:] = mult[1:] != mult[:-1]
    idx = torch.arange(M)
    run = change.cumsum(0) - 1
    starts = idx[change]
    ends = torch.cat((starts[1:] - 1, torch.tensor([M - 1])))
    start, end = starts[run], ends[run]                    # first and last row of the row's run of equal multipliers
    return ((idx - start >= reach) | (start == 0)) & ((end - idx >= reach) | (end == M - 1))


def flat_rows(layout, M):
    """Rows judged at TOL_ROW alone (on a backend that reports scales): the interior ones - without the small side of
    `cliff_down`, whose scale the persistent kernel caps by design."""
    mult = multipliers(layout, M)
    keep = interior(mult) & (mult != 0)
    if layout == "cliff_down":
        keep &= exponents(layout, M)[0] == 0
    return keep


def tile_spread(rows, tile):
    """Per tile of `tile` consecutive rows: max_i rowmax_i / min_i rowmax_i over the tile's non-zero rows (1 for a tile
    without any)."""
    rm = rows.detach().double().abs().amax(1)
    out = []
    for b in range(0, rm.numel(), tile):
        t = rm[b:b + tile]
        t = t[t > 0]
        out.append(float(t.max() / t.min()) if t.numel() else 1.0)
    return torch.tensor(out, dtype=torch.float64)


def row_err(got, ref):
    """e_i; a zero reference row: 0 where the output row is exactly zero, inf otherwise."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d, m = (got - ref).abs().amax(1), ref.abs().amax(1)
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    e = d / torch.where(m > 0, m, torch.ones_like(m))
    return torch.where((m == 0) & (d > 0), torch.full_like(e, math.inf), e)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    v = float((a - b).abs().max() / (b.abs().max() + 1e-30))
    return v if v == v else math.inf


# ---- cases and their float64 reference ---------------------------------------------------------------------------------------------
def _params(g, kin, scale=0.3):
    """The weights of tests/test_colchain_gpu.py / tests/test_cbwd_gpu.py."""
    return dict(W1=torch.randn(128, kin, generator=g) * scale / kin ** 0.5 * 4, b1=torch.randn(128, generator=g) * 0.1,
                W2=torch.randn(128, 128, generator=g) * scale / 3, b2=torch.randn(128, generator=g) * 0.1,
                W3=torch.randn(128, 128, generator=g) * scale / 3, b3=torch.randn(128, generator=g) * 0.1,
                gamma=1 + 0.1 * torch.randn(128, generator=g), beta=0.1 * torch.randn(128, generator=g))


def _fwd(P, X):
    z1 = F.linear(X, P["W1"], P["b1"])
    z2 = F.linear(F.gelu(z1), P["W2"], P["b2"])
    y3 = F.linear(F.gelu(z2), P["W3"], P["b3"])
    return z1, z2, y3, F.layer_norm(y3, (128,), P["gamma"], P["beta"], 1e-5)


class Case:
    """One MLP (shape: edge 128 -> 128 with residual and in_add; node 192 -> 128, outputs [gx 128 | gnbm 64]; enc 16 -> 128,
    no input gradient), M rows: float32 weights, inputs and saved tensors, and the float64 reference of every layout."""

    def __init__(self, shape, M, scale=0.3, seed=0):
        self.shape, self.M = shape, M
        g = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + M % 997 + seed)
        kin = {"edge": 128, "node": 192, "enc": 16}[shape]
        self.kin = kin
        if shape == "enc":
            self.x = torch.randn(M, 16, generator=g) * torch.tensor([1.0] * 12 + [1e-3] * 4)
        else:
            self.x = torch.randn(M, kin, generator=g)          # node: [nbm 64 | x 128]
        self.P = _params(g, kin, scale)
        self.go = torch.randn(M, 128, generator=g)
        self.add = torch.randn(M, 128, generator=g) * 0.1 if shape in ("edge", "enc") else None
        self.n_nodes = 300
        self.gagg = torch.randn(self.n_nodes, 64, generator=g) * 0.1
        self.gs = torch.randint(0, self.n_nodes, (M,), generator=g)
        self.gr = torch.randint(0, self.n_nodes, (M,), generator=g)
        self.Pg = {k: v.double().requires_grad_(True) for k, v in self.P.items()}
        self.X = self.x.double().requires_grad_(True)
        self.z1, self.z2, self.y3, self.ln = _fwd(self.Pg, self.X)
        y3 = self.y3.detach()
        self.stats = torch.stack((y3.mean(1), (y3.var(1, unbiased=False) + 1e-5).rsqrt()), 1).float()
        self.saved = tuple(t.detach().float() for t in (self.z1, self.z2, self.y3))      # what the kernels are handed
        self._ref = {}

    def has_gadd(self, layout):
        return self.shape == "edge" and layout == "flat"

    def inputs(self, layout):
        """(go, in_add or None, total float64 gradient of the LayerNorm output) of the layout: float32 rows x 2^k, exact."""
        m = multipliers(layout, self.M)[:, None]
        go = (self.go.double() * m).float()
        assert bool((go.double() == self.go.double() * m).all())
        add = None if self.add is None else (self.add.double() * m).float()
        tot = go.double()
        if add is not None:
            tot = tot + add.double()
        if self.has_gadd(layout):
            tot = tot + torch.cat((self.gagg[self.gs], self.gagg[self.gr]), 1).double()
        return go, add, tot

    def l1(self, name):
        """Largest column 1-norm of the chain layer between the last fragment set and tensor `name` (x 1.13: a GELU' follows)."""
        P = self.P
        col = lambda W: float(W.double().abs().sum(0).max())
        if name == "g3":
            return 1.0
        if name == "gz2":
            return GELU_SLOPE * col(P["W3"])
        if name == "gz1":
            return GELU_SLOPE * col(P["W2"])
        if name == "gx":
            return col(P["W1"][:, 64:])
        if name == "gnbm":
            return col(P["W1"][:, :64])
        return col(P["W1"])

    def ref(self, layout):
        """float64 autograd: every row tensor and every parameter gradient of the layout."""
        if layout not in self._ref:
            go, add, tot = self.inputs(layout)
            names = list(self.P)
            gr = torch.autograd.grad(self.ln, [self.z1, self.z2, self.y3] + [self.Pg[n] for n in names] +
                                     ([] if self.shape == "enc" else [self.X]), grad_outputs=tot, retain_graph=True)
            rows = {"gz1": gr[0], "gz2": gr[1], "g3": gr[2]}
            if self.shape == "edge":
                rows["ge"] = gr[-1] + go.double()
            elif self.shape == "node":
                rows["gx"], rows["gnbm"] = gr[-1][:, 64:] + go.double(), gr[-1][:, :64]
            self._ref[layout] = (rows, dict(zip(names, gr[3:3 + len(names)])))
        return self._ref[layout]


_CASES = {}


def case(shape, M, scale=0.3):
    """Cases are built once and shared (their references are never modified)."""
    key = (shape, M, scale)
    if key not in _CASES:
        _CASES[key] = Case(shape, M, scale)
    return _CASES[key]


# ---- backends --------------------------------------------------------------------------------------------------------------------
class Torch32:
    """fp32 eager autograd of the same MLP: reports no scales."""
    name = "torch32"

    def run(self, c, layout):
        go, add, tot = c.inputs(layout)
        P = {k: v.clone().requires_grad_(True) for k, v in c.P.items()}
        X = c.x.clone().requires_grad_(True)
        z1, z2, y3, ln = _fwd(P, X)
        names = list(P)
        gr = torch.autograd.grad(ln, [z1, z2, y3] + [P[n] for n in names] + ([] if c.shape == "enc" else [X]),
                                 grad_outputs=tot.float())
        rows = {"gz1": gr[0], "gz2": gr[1], "g3": gr[2]}
        if c.shape == "edge":
            rows["ge"] = gr[-1] + go
        elif c.shape == "node":
            rows["gx"], rows["gnbm"] = gr[-1][:, 64:] + go, gr[-1][:, :64]
        return Out(rows, dict(zip(names, gr[3:3 + len(names)])), None, True, 0)


def pow2_scale(m):
    """Power of two s with s m in [2^13, 2^14) (csrc/gfv_split.h; m = 0: 2^126)."""
    return 2.0 ** 126 if m <= 0 else min(2.0 ** (13 - math.floor(math.log2(m))), 2.0 ** 126)


def split16(v, s, flush=False):
    """v quantised as fp16 hi + lo behind the scale s (csrc/gfv_split.h: hi = fp16(s v), lo = fp16(s v - hi))."""
    t = (v * s).float()
    ftz = (lambda h: torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)) if flush else (lambda h: h)
    hi = ftz(t.half())
    lo = ftz((t - hi.float()).half())
    return (hi.double() + lo.double()) / s


def _dgelu(z):
    z = z.double()
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


class Emu:
    """The design on the CPU: float64 arithmetic on the float32 tensors a kernel is handed; g3 / gz2 / gz1 quantised as fp16
    hi + lo behind one scale per tile of `tile` rows, s3 = 2 pow2_scale(13.5 max rstd |gamma dy|), each step down
    2^-ceil(log2(1.13 L1)).  flush: fp16 subnormals flushed to zero; shift: every fragment scale 2^shift off;
    report_shift: reports scales 2^report_shift off what it uses.  (No scale cap: that rule depends on the workgroup's walk.)"""

    def __init__(self, tile, flush=False, shift=0, report_shift=0):
        self.tile, self.flush, self.shift, self.report_shift = tile, flush, shift, report_shift
        self.name = f"emu{tile}"

    def run(self, c, layout):
        go, add, tot = c.inputs(layout)
        M, P = c.M, {k: v.double() for k, v in c.P.items()}
        z1, z2, y3 = (t.double() for t in c.saved)
        mean, rstd = c.stats[:, 0:1].double(), c.stats[:, 1:2].double()
        xh = (y3 - mean) * rstd
        gg = tot * P["gamma"]
        g3 = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
        bound = (gg.abs().amax(1) * rstd[:, 0].abs())
        s3 = torch.empty(M, dtype=torch.float64)
        for b in range(0, M, self.tile):
            s3[b:b + self.tile] = 2.0 * pow2_scale(13.5 * float(bound[b:b + self.tile].max())) * 2.0 ** self.shift
        step = lambda W: 2.0 ** -math.ceil(math.log2(GELU_SLOPE * float(W.abs().sum(0).max())))
        s2 = s3 * step(P["W3"])
        s1 = s2 * step(P["W2"])
        q = lambda v, s: split16(v, s[:, None], self.flush)
        a1, a2 = F.gelu(z1), F.gelu(z2)
        g3q = q(g3, s3)
        gz2 = (g3q @ P["W3"]) * _dgelu(z2)
        gz2q = q(gz2, s2)
        gz1 = (gz2q @ P["W2"]) * _dgelu(z1)
        gz1q = q(gz1, s1)
        rows = {"g3": g3, "gz2": gz2, "gz1": gz1}
        x = c.x.double()
        if c.shape != "enc":
            gin = gz1q @ P["W1"]
            if c.shape == "edge":
                rows["ge"] = gin + go.double()
            else:
                rows["gx"], rows["gnbm"] = gin[:, 64:] + go.double(), gin[:, :64]
        sums = {"W3": g3q.T @ a2, "b3": g3q.sum(0), "W2": gz2q.T @ a1, "b2": gz2q.sum(0), "W1": gz1q.T @ x, "b1": gz1q.sum(0),
                "gamma": (tot * xh).sum(0), "beta": tot.sum(0)}
        ng = (M + 15) // 16
        gs = torch.stack([s[::16][:ng] for s in (s3, s2, s1)]) * 0.25 * 2.0 ** self.report_shift
        return Out(rows, sums, gs, True, 0)


class Gpu:
    """The kernels, through ops.rowtile_chain as tests/test_colchain_gpu.py / tests/test_cbwd_gpu.py launch them, always with a
    gscale buffer.  family: "col_read" / "col_rc" (CHAIN_COLUMN_OWNER, z2 and the LayerNorm input read / recomputed), "cbwd"
    (the library's choice with GFV_CBWD=1: the small-tile kernel), "row" (CHAIN_ROW_OWNER)."""
    PATH = {"col_read": 5 + 16, "col_rc": 5 + 16, "cbwd": 5 + 128, "row": 5}

    def __init__(self, family):
        assert family in self.PATH
        self.family = self.name = family
        self._dev = {}

    def _case_dev(self, c):
        """Device copies of what does not depend on the layout (one case at a time)."""
        from gfv import ops
        if self._dev.get("key") is not c:
            dev = torch.device("cuda:0")
            d = lambda t: t.to(dev).contiguous()
            Pd = {k: d(v) for k, v in c.P.items()}
            if c.shape == "node":                         # rows for x first, then nbm (engine._T(perm=True))
                W1t = torch.empty(192, 128, device=dev)
                ops.transpose(Pd["W1"], out=W1t[0:128], col0=64, ncols=128)
                ops.transpose(Pd["W1"], out=W1t[128:192], col0=0, ncols=64)
            else:
                W1t = ops.transpose(Pd["W1"])
            Ws = [c.P["W2"], c.P["W3"]] + ([] if c.shape == "enc" else [c.P["W1"]])
            wi = ops.WeightImages(dev, torch.stack([w.abs().max() for w in Ws]).max().reshape(1).to(dev))
            wi.static = [(0, 1 << 62)]
            z1, z2, y3 = (d(t) for t in c.saved)
            self._dev = dict(key=c, d=d, dev=dev, Pd=Pd, W1t=W1t, W2t=ops.transpose(Pd["W2"]), W3t=ops.transpose(Pd["W3"]), wi=wi,
                             z1=z1, z2=z2, y3=y3, stats=d(c.stats),
                             xs=[d(c.x[:, :64]), d(c.x[:, 64:])] if c.shape == "node" else [d(c.x)], a1=d(F.gelu(c.saved[0])), a2=d(F.gelu(c.saved[1])),
                             gagg=d(c.gagg), gs=d(c.gs.int()), gr=d(c.gr.int()))
        return self._dev

    def run(self, c, layout):
        from gfv import lib as L, ops
        lib = L.load()
        D = self._case_dev(c)
        d, dev, Pd, M, fam = D["d"], D["dev"], D["Pd"], c.M, self.family
        go, add, _ = c.inputs(layout)
        god = d(go)
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        col = fam.startswith("col")
        rows = {n: nan(M, 64 if n == "gnbm" else 128) for n in (ROWS_COL if col else ROWS_ALL)[c.shape]}
        gs = torch.zeros(3, ops.gscale_ld(M), device=dev)
        kw = dict(in_op=L.IN_LNBWD, in_gamma=Pd["gamma"], in_aux=D["y3"], in_stats=D["stats"], gscale=gs, wimg=D["wi"])
        if add is not None:
            kw["in_add"] = d(add)
        if c.has_gadd(layout):
            kw.update(gadd=D["gagg"], gadd_s=D["gs"], gadd_r=D["gr"])
        z2d = D["z2"]
        if col:
            part = nan(lib.gfv_rowtile_dw_partials_m(M), L.DW_FUSED_FLOATS)
            kw.update(dw_partial=part, family=L.CHAIN_COLUMN_OWNER)
            if fam == "col_rc":
                kw["rc"] = (Pd["W2"], Pd["b2"], Pd["W3"], Pd["b3"])
                kw["in_aux"] = z2d = None
        else:
            part = nan(ops.ln_rows(M), 2, 128)
            kw.update(ln_partial=part, in_save=rows["g3"], family=L.CHAIN_ROW_OWNER if fam == "row" else 0)
        l0 = ops.LayerSpec(D["W3t"], None, L.OP_MUL_DGELU, aux=z2d, save=None if col else rows["gz2"])
        if c.shape == "enc":
            layers = [l0, ops.LayerSpec(D["W2t"], None, L.OP_MUL_DGELU, aux=D["z1"])]
            outs = [rows["gz1"]]
        else:
            layers = [l0, ops.LayerSpec(D["W2t"], None, L.OP_MUL_DGELU, save=rows["gz1"], aux=D["z1"]), ops.LayerSpec(D["W1t"])]
            outs = [rows["ge"]] if c.shape == "edge" else [rows["gx"], (rows["gnbm"], 64)]
            kw["res"] = [god] if c.shape == "edge" else [god, None]
        if col:
            assert ops.rowtile_chain(M, [ops.Seg(god)], layers, outs, query_fused=True, **kw)
            wrote = ops.rowtile_chain(M, [ops.Seg(god)], layers, outs, **kw)
        else:
            with L.limits(GFV_CBWD=1 if fam == "cbwd" else 0):
                wrote = ops.rowtile_chain(M, [ops.Seg(god)], layers, outs, **kw)
        path = lib.gfv_rowtile_last_path()
        assert path == self.PATH[fam], (fam, path)
        assert wrote, "the launch left no gscale"
        # the weight gradients: fused blocks (column-owner persistent kernel) or the weight-gradient launch with the chain's scales
        sums = {}
        xsegs = [ops.Seg(D["xs"][0], width=16, ld=16)] if c.shape == "enc" else [ops.Seg(t) for t in D["xs"]]
        dwkw = dict(col_scale=True) if c.shape == "enc" else {}
        if col:
            tot = part.double().sum(0).cpu()
            sums = {"W3": tot[:16384].view(128, 128), "b3": tot[16384:16512], "W2": tot[16512:16512 + 16384].view(128, 128),
                    "b2": tot[16512 + 16384:16512 + 16384 + 128], "gamma": tot[2 * 16384 + 256:2 * 16384 + 384],
                    "beta": tot[2 * 16384 + 384:2 * 16384 + 512]}
        else:
            n = ops.last_ln_rows()
            tot = part[:n].double().sum(0).cpu()
            sums["gamma"], sums["beta"] = tot[0], tot[1]
            part = part[:n]
            sums["W3"], sums["b3"] = ops.linear_dw(rows["g3"], 128, [ops.Seg(D["a2"])], M, gscale=gs[0])
            sums["W2"], sums["b2"] = ops.linear_dw(rows["gz2"], 128, [ops.Seg(D["a1"])], M, gscale=gs[1])
        sums["W1"], sums["b1"] = ops.linear_dw(rows["gz1"], 128, xsegs, M, gscale=gs[2], **dwkw)
        torch.cuda.synchronize()
        ng = (M + 15) // 16
        finite = bool(torch.isfinite(part).all()) and bool(torch.isfinite(gs).all())
        flags = L.C.c_int32(0)
        L.check(lib.gfv_status_flags(L.C.byref(flags)), "gfv_status_flags")
        return Out({k: v.cpu() for k, v in rows.items()}, {k: v.cpu() for k, v in sums.items()}, gs[:, :ng].double().cpu(), finite,
                   flags.value)


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def floor(c, name, ref_rows, gscale):
    """F_i of tensor `name` from the reported scales [3, groups]."""
    slot = {"g3": 0, "gz2": 0, "gz1": 1}.get(name, 2)
    s = 4.0 * gscale[slot].double().repeat_interleave(16)[:c.M]
    m = ref_rows.abs().amax(1)
    return Q16 * c.l1(name) / (s * torch.where(m > 0, m, torch.ones_like(m)))


def checks(c, layout, out, names=None, flat=False, sums=SUMS):
    """The check list of one run: the same names whatever the backend.  flat: every non-zero row at TOL_ROW (a backend with
    per-row scales, or none); otherwise the interior rows at TOL_ROW, the others at TOL_ROW + F_i from the reported scales."""
    rows_ref, sums_ref = c.ref(layout)
    names = tuple(n for n in ROWS_ALL[c.shape] if n in out.rows) if names is None else names
    flat = flat or out.gscale is None
    mult = multipliers(layout, c.M)
    nz = mult != 0
    easy = nz if flat else flat_rows(layout, c.M)
    hard = nz & ~easy
    tag = f"{c.shape}/{c.M}/{layout}"
    L = []
    for n in names:
        ref = rows_ref[n].detach()
        e = row_err(out.rows[n], ref)
        v = float(e[easy].max()) if bool(easy.any()) else 0.0
        L.append(Check(f"{tag}/{n}/rows_flat", v < TOL_ROW, v, TOL_ROW))
        if flat or not bool(hard.any()):
            v = 0.0
        else:
            v = float((e[hard] / (TOL_ROW + floor(c, n, ref, out.gscale)[hard])).max())
        L.append(Check(f"{tag}/{n}/rows_floor", v < 1.0, v, 1.0))
        z = out.rows[n].detach().double().cpu()[~nz]
        v = float((z != 0).sum()) if z.numel() else 0.0      # (NaN != 0: counted)
        L.append(Check(f"{tag}/{n}/zero_rows", v == 0, v, 0.0))
    for n in sums:
        v = rel(out.sums[n], sums_ref[n])
        L.append(Check(f"{tag}/d{n}", v < TOL_SUM, v, TOL_SUM))
    # (a) the floor must stay small where the design says it is: the exponent-0 rows of `mixed`
    v = 0.0
    if layout == "mixed" and not flat:
        top = exponents(layout, c.M)[0] == 0
        v = max(float(floor(c, n, rows_ref[n].detach(), out.gscale)[top].max()) for n in names)
    L.append(Check(f"{tag}/floor_of_top_rows", v < 1e-6, v, 1e-6))
    # (b) no reported g3 scale beyond the no-overflow guarantee (flat: the scales reported, if any, are not per-tile fragment
    # scales - the row-owner chain's are weight-gradient slab scales of rows it scaled one by one)
    v = 0.0
    if not flat:
        g3 = rows_ref["g3"].detach().abs().amax(1)
        g3 = F.pad(g3, (0, -c.M % 16)).view(-1, 16).amax(1)
        v = float((4.0 * out.gscale[0].double() * g3).max())
    L.append(Check(f"{tag}/g3_scale_bound", v <= 2.0 ** 15 * (1 + 1e-3), v, 2.0 ** 15 * (1 + 1e-3)))
    L.append(Check(f"{tag}/finite", bool(out.finite), 0.0 if out.finite else 1.0, 0.0))
    L.append(Check(f"{tag}/status_word", out.status == 0, float(out.status), 0.0))
    return L


def failed(L):
    return [c for c in L if not c.ok]


def report(L):
    return "\n".join(f"{'ok  ' if c.ok else 'FAIL'} {c.value:.3e} (bound {c.bound:.3e})  {c.name}" for c in L)


def rowacc(family, c, layout, out):
    """`ROWACC family shape layout exponent e_max` lines: the largest e_i of the launch's final row tensor(s) per row exponent."""
    rows_ref, _ = c.ref(layout)
    e = torch.stack([row_err(out.rows[n], rows_ref[n].detach()) for n in FINAL[c.shape]]).amax(0)
    return rowacc_lines(family, c.shape, layout, e)


def rowacc_lines(family, shape, layout, e):
    ex, zero = exponents(layout, e.numel())
    return [f"ROWACC {family} {shape} {layout} {int(k)} {float(e[(ex == k) & ~zero].max()):.2e}"
            for k in sorted(set(ex[~zero].tolist()), reverse=True)]
