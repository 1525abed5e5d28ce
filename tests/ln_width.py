"""LayerNorm at hidden < 128, stated in float64 - shared by tests/test_ln_width_cpu.py and tests/test_ln_width_gpu.py.

A model of hidden size h < 128 runs zero padded to the kernels' 128 columns (FVMmodel/padding.py): node latents in columns
0 .. h - 1, the two halves of an edge latent in columns 0 .. h/2 - 1 and 64 .. 64 + h/2 - 1.  Every kernel takes the LayerNorm
statistics over the h real columns; the padded ones are exactly zero on input and must be exactly zero in every forward output.
The reference here is float64 LayerNorm (eps 1e-5) over the real columns and its backward.

What the suite could not see before: with rows whose mean is several standard deviations from zero, a rule that sums
(0 - mean)^2 over the padded zeros and takes npad mean^2 out again subtracts two numbers of size 128 mean^2 to obtain one of size
h var (`Emu(old=True)`).  The kernels' rule (`Emu()`; csrc/gfv_common.h gfv_lnq_*) adds (x - mean)^2 over the non-zero entries
and mean^2 for every zero beyond the npad padded ones.  OFFSETS is |mean| / std of the LayerNorm input rows; every case carries
exact zeros inside real columns, which a rule that takes every zero for padding gets wrong (`Emu(rule="nocorr")`).

Judging: row by row (chain_rows.row_err).  Offset 0: chain_rows.TOL_ROW.  Offsets 8 / 32: max(1e-5, 4 e32), e32 the largest row
error of float32 eager torch over the h real columns (the reference implementation's arithmetic) on the same inputs - the
"reference keeps a quarter of the limit" rule of tests/test_dw_float64_cpu.py.  dgamma / dbeta: chain_rows.TOL_SUM (x 4 e32 of the
sums likewise).

Backends, one interface `run(problem) -> {name: tensor}`: Torch32, Emu(rule), and Gpu(site) for the launches of
tests/test_ln_width_gpu.py.  Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import math

import torch
import torch.nn.functional as F

import chain_rows as CR

EPS = 1e-5
WIDTHS = (16, 32, 64, 112, 128)
LAYOUTS = ("node", "edge")
OFFSETS = (0, 8, 32)
M = 197                 # 3 tiles of 64 rows + 5, 6 tiles of 32 + 5, one 128-row block + 69
M_LIN1 = 1024 + 197     # csrc/lin1.hip takes launches of 1024 rows and more: 9 blocks of 128 rows + the same 69
ZERO_EVERY = 7          # directly fed inputs: every 7th row has an exact zero in its first real column


def real_cols(h, layout="node"):
    m = torch.zeros(128, dtype=torch.bool)
    if layout == "node":
        m[:h] = True
    else:
        m[:h // 2] = True
        m[64:64 + h // 2] = True
    return m


def cases(widths=WIDTHS, offsets=OFFSETS):
    return [(h, lay, off) for h in widths for lay in LAYOUTS for off in offsets]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def pad_vec(v, real):
    return torch.where(real, v, torch.zeros_like(v))


def direct_rows(g, h, layout, offset, s=1.0, m=M):
    """LayerNorm input rows handed in directly: offset s + randn s on the real columns, padding exactly 0, an exact zero in the
    first real column of every ZERO_EVERY-th row."""
    real = real_cols(h, layout)
    x = (offset * s + torch.randn(m, 128, generator=g) * s) * real
    x[::ZERO_EVERY, 0] = 0.0
    return x.float()


# ---- float64 statements ------------------------------------------------------------------------------------------------------------
def stats64(x, real):
    xr = x.double()[:, real]
    mean = xr.mean(1, keepdim=True)
    var = ((xr - mean) ** 2).mean(1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + EPS)


def ln64(x, gamma, beta, real, stats=None):
    """LayerNorm over the real columns; padding exactly 0."""
    mean, rstd = stats64(x, real) if stats is None else stats
    out = ((x.double() - mean) * rstd * gamma.double() + beta.double()) * real
    return out


def ln_bwd64(y, go, gamma, real, stats=None):
    """Input gradient (padding 0), dgamma, dbeta of LayerNorm over the real columns; go: gradient of the LayerNorm output."""
    mean, rstd = stats64(y, real) if stats is None else stats
    n = float(real.sum())
    xh = (y.double() - mean) * rstd * real
    go = go.double() * real
    gg = go * gamma.double()
    m1, m2 = gg.sum(1, keepdim=True) / n, (gg * xh).sum(1, keepdim=True) / n
    gx = rstd * (gg - m1 - xh * m2) * real
    return gx, (go * xh).sum(0), go.sum(0)


# ---- the kernels' statistics in float32 ----------------------------------------------------------------------------------------------
def stats32(x, h, layout, rule="new"):
    """(mean, rstd) as float64 tensors of float32 values: float32 arithmetic on the 128 columns of float32 rows.
    rule: "new" (non-zero entries + counted zeros), "old" (the subtraction), and the mutations "inv128" (1 / 128 at a narrow
    width), "nocorr" (the - (128 - h) of the zero count dropped), "allpad" (every zero taken for padding: no count term at all -
    only rows with an exact zero in a real column can tell), "edge_as_node" (statistics over columns 0 .. h - 1 whatever the
    layout)."""
    x = x.float()
    npad = torch.tensor(float(128 - h), dtype=torch.float32)
    n = torch.tensor(float(128 if rule == "inv128" else h), dtype=torch.float32)
    if rule == "edge_as_node":
        mask = real_cols(h, "node")
        xr = x[:, mask]
        mean = xr.sum(1, keepdim=True) / n
        ssq = ((xr - mean) * (xr - mean)).sum(1, keepdim=True)
    else:
        mean = x.sum(1, keepdim=True) / n
        d = x - mean
        if rule == "old":
            ssq = (d * d).sum(1, keepdim=True) - npad * (mean * mean)
        else:
            q = torch.where(x != 0, d * d, torch.zeros_like(d)).sum(1, keepdim=True)
            cz = (x == 0).float().sum(1, keepdim=True)
            corr = cz if rule == "nocorr" else (torch.zeros_like(cz) if rule == "allpad" else cz - npad)
            ssq = q + corr * (mean * mean)
    rstd = torch.rsqrt(ssq / n + torch.tensor(EPS, dtype=torch.float32))
    return mean.double(), rstd.double()


# ---- problems --------------------------------------------------------------------------------------------------------------------
def _lin(g, n_out, k, scale):
    return torch.randn(n_out, k, generator=g) * scale


class Problem:
    """Common part: width, layout, offset, the real-column mask, gamma / beta (0 in the padding)."""

    def __init__(self, kind, h, layout, offset, m=M):
        self.kind, self.h, self.layout, self.offset, self.M = kind, h, layout, offset, m
        self.real = real_cols(h, layout)
        self.g = _gen(("fwd", "bwd", "mlp", "trans", "mlp_dense").index(kind), h, LAYOUTS.index(layout), offset)
        self.gamma = pad_vec(1 + 0.1 * torch.randn(128, generator=self.g), self.real)
        self.beta = pad_vec(0.1 * torch.randn(128, generator=self.g), self.real)
        self._ref = None

    @property
    def tag(self):
        return f"{self.kind} h={self.h} {self.layout} offset={self.offset}"

    def pad_w(self, W, rows=True, cols=True):
        W = W.clone()
        if rows:
            W[~self.real, :] = 0
        if cols:
            W[:, ~self.real] = 0
        return W

    def ref(self):
        if self._ref is None:
            self._ref = self.evaluate(torch.float64, lambda x: stats64(x, self.real))
        return self._ref


class Fwd(Problem):
    """out = LayerNorm(x) W^T + b (128 -> 128), x handed in directly (GFV_IN_LN; lin1.hip / lin1s.hip prologue)."""
    rows, sums, stats_of = ("out",), (), "x"

    def __init__(self, h, layout, offset, m=M):
        super().__init__("fwd", h, layout, offset, m)
        self.x = direct_rows(self.g, h, layout, offset, m=m)
        self.W = self.pad_w(_lin(self.g, 128, 128, 0.1))
        self.b = pad_vec(0.1 * torch.randn(128, generator=self.g), self.real)

    def evaluate(self, dt, stats):
        x = self.x.to(dt)
        if stats is None:       # eager torch over the real columns alone
            ln = torch.zeros_like(x)
            ln[:, self.real] = F.layer_norm(x[:, self.real], (self.h,), self.gamma.to(dt)[self.real], self.beta.to(dt)[self.real], EPS)
        else:
            ln = ln64(x, self.gamma, self.beta, self.real, stats(self.x)).to(dt)
        return {"ln": ln, "out": F.linear(ln, self.W.to(dt), self.b.to(dt))}


class Bwd(Problem):
    """gx = LayerNorm-backward(v; y, gamma) with v = gz W^T (256 -> 128), the LayerNorm input y handed in directly
    (GFV_FIN_LNBWD: the `fin_aux`), + dgamma, dbeta; and, for GFV_IN_LNBWD (`in_aux`), the same with v = go handed in and three
    transposed layers behind it (z1 / z2: the saved pre-activations)."""
    rows, sums, stats_of = ("gx", "ge", "g3"), ("gamma", "beta", "gamma_in", "beta_in"), "y"

    def __init__(self, h, layout, offset, m=M):
        super().__init__("bwd", h, layout, offset, m)
        g, M = self.g, m
        self.y = direct_rows(g, h, layout, offset, s=2.0, m=m)
        self.gz = torch.randn(M, 256, generator=g)
        self.Wt = self.pad_w(_lin(g, 128, 256, 0.1), cols=False)          # [128 outputs, 256 inputs]
        self.res = torch.randn(M, 128, generator=g) * 0.01 * self.real
        self.go = (torch.randn(M, 128, generator=g) * self.real).float()
        self.z1 = (torch.randn(M, 128, generator=g) * self.real).float()
        self.z2 = (torch.randn(M, 128, generator=g) * self.real).float()
        self.W1, self.W2, self.W3 = (self.pad_w(_lin(g, 128, 128, 0.1)) for _ in range(3))

    def with_rows(self, y):
        """The same problem on other LayerNorm input rows (those a forward launch left): a new problem, not cached."""
        q = Bwd(self.h, self.layout, self.offset, self.M)
        q.y = y.detach().float().cpu().clone()
        return q

    def evaluate(self, dt, stats):
        y = self.y.to(dt)
        v = F.linear(self.gz.to(dt), self.Wt.to(dt))
        out = {}
        for name, vv in (("gx", v), ("g3", self.go.to(dt))):
            if stats is None:
                yr = y[:, self.real].clone().requires_grad_(True)
                gm, bt = self.gamma.to(dt)[self.real].clone().requires_grad_(True), self.beta.to(dt)[self.real].clone().requires_grad_(True)
                gr = torch.autograd.grad(F.layer_norm(yr, (self.h,), gm, bt, EPS), (yr, gm, bt), vv[:, self.real])
                gx, dg, db = (torch.zeros(self.M, 128, dtype=dt), torch.zeros(128, dtype=dt), torch.zeros(128, dtype=dt))
                gx[:, self.real], dg[self.real], db[self.real] = gr
            else:
                gx, dg, db = (t.to(dt) for t in ln_bwd64(y, vv, self.gamma, self.real, stats(self.y)))
            sfx = "" if name == "gx" else "_in"
            out["gamma" + sfx], out["beta" + sfx] = dg, db
            out[name] = gx + self.res.to(dt) if name == "gx" else gx
        # GFV_IN_LNBWD: g3 -> (g3 W3) gelu'(z2) -> (. W2) gelu'(z1) -> . W1 + go     (W given transposed: out = in @ W)
        dgelu = (lambda z: CR._dgelu(z).to(dt))
        gz2 = (out["g3"] @ self.W3.to(dt)) * dgelu(self.z2)
        gz1 = (gz2 @ self.W2.to(dt)) * dgelu(self.z1)
        out["ge"] = gz1 @ self.W1.to(dt) + self.go.to(dt)
        return out


class Mlp(Problem):
    """3-layer MLP with a final LayerNorm (GFV_FIN_LN): y3 = gelu(gelu(x W1^T + b1) W2^T + b2) W3^T + b3, the row offset added to
    b3 on the real columns in units of s = the median float64 row std of y3 without it; one real output column of y3 is exactly
    zero (its W3 row and b3 entry are zero).  That column alone holds the rows' |mean| / std near h / sqrt(h - 1) however large
    the offset, so each case also exists without it (kind "mlp_dense"), where |mean| / std is the offset."""
    rows, sums, stats_of = ("y3", "out"), (), "y3"

    def __init__(self, h, layout, offset, zero=True):
        super().__init__("mlp" if zero else "mlp_dense", h, layout, offset)
        g = self.g
        self.x = (torch.randn(M, 128, generator=g) * self.real).float()
        self.W1, self.W2, self.W3 = (self.pad_w(_lin(g, 128, 128, 0.09 * (128 / h) ** 0.5)) for _ in range(3))
        self.b1, self.b2, self.b3 = (pad_vec(0.1 * torch.randn(128, generator=g), self.real) for _ in range(3))
        self.zero_col = int(torch.nonzero(self.real)[1])
        if zero:
            self.W3[self.zero_col, :] = 0
            self.b3[self.zero_col] = 0
        else:
            self.zero_col = None
        y3 = self._y3(torch.float64)
        self.s = float(y3[:, self.real].std(1, unbiased=False).median())
        shift = torch.full((128,), offset * self.s) * self.real
        if zero:
            shift[self.zero_col] = 0
        self.b3 = (self.b3.double() + shift.double()).float()

    def _y3(self, dt):
        z1 = F.linear(self.x.to(dt), self.W1.to(dt), self.b1.to(dt))
        z2 = F.linear(F.gelu(z1), self.W2.to(dt), self.b2.to(dt))
        return F.linear(F.gelu(z2), self.W3.to(dt), self.b3.to(dt))

    def evaluate(self, dt, stats):
        y3 = self._y3(dt)
        if stats is None:
            ln = torch.zeros_like(y3)
            ln[:, self.real] = F.layer_norm(y3[:, self.real], (self.h,), self.gamma.to(dt)[self.real], self.beta.to(dt)[self.real], EPS)
        else:
            ln = ln64(y3, self.gamma, self.beta, self.real, stats(y3)).to(dt)
        out = {"y3": y3, "out": ln + self.x.to(dt)}
        if stats is not None:
            m, r = stats(y3)
            out["stats"] = torch.cat((m, r), 1).to(dt)
        return out


class Trans(Problem):
    """The Transolver block's row-local chain (gfv_trans_mlp_fwd / _bwd): fx1 = x Wout^T + bout + res, z = LN(fx1) Wpre^T + bpre,
    out = gelu(z) Wpost^T + bpost + fx1; the LayerNorm input's offset is handed in through `res`.  Backward: g_z, g_fx1, g_out_x,
    dgamma, dbeta for the gradient g of `out`."""
    rows, sums, stats_of = ("fx1", "z", "out", "g_z", "g_fx1", "g_out_x"), ("gamma", "beta"), "fx1"

    def __init__(self, h, layout, offset):
        super().__init__("trans", h, layout, offset)
        g = self.g
        self.x = (torch.randn(M, 128, generator=g) * self.real).float()
        self.res = direct_rows(g, h, layout, offset)
        self.Wout = self.pad_w(_lin(g, 128, 128, 0.02))
        self.bout = torch.zeros(128)
        self.Wpre = _lin(g, 256, 128, 0.09) * self.real            # [256, 128]: dead input columns 0
        self.bpre = 0.1 * torch.randn(256, generator=g)
        self.Wpost = self.pad_w(_lin(g, 128, 256, 0.06), cols=False)
        self.bpost = pad_vec(0.1 * torch.randn(128, generator=g), self.real)
        self.gout = (torch.randn(M, 128, generator=g) * self.real).float()
        # a row of x W^T that vanishes keeps the exact zero of `res` in fx1: the zero rows of x
        self.x[::ZERO_EVERY] = 0.0

    def evaluate(self, dt, stats):
        t = lambda v: v.to(dt)
        fx1 = F.linear(t(self.x), t(self.Wout), t(self.bout)) + t(self.res)
        st = None if stats is None else stats(fx1)

        def ln_of(f):
            if st is None:
                o = torch.zeros_like(f)
                o[:, self.real] = F.layer_norm(f[:, self.real], (self.h,), t(self.gamma)[self.real], t(self.beta)[self.real], EPS)
                return o
            return ln64(f, self.gamma, self.beta, self.real, st).to(dt)
        ln = ln_of(fx1)
        z = F.linear(ln, t(self.Wpre), t(self.bpre))
        out = F.linear(F.gelu(z), t(self.Wpost), t(self.bpost)) + fx1
        g = t(self.gout)
        g_z = (g @ t(self.Wpost)) * CR._dgelu(z).to(dt)
        v = g_z @ t(self.Wpre)
        if st is None:
            fr = fx1[:, self.real].detach().clone().requires_grad_(True)
            gm, bt = t(self.gamma)[self.real].clone().requires_grad_(True), t(self.beta)[self.real].clone().requires_grad_(True)
            gr = torch.autograd.grad(F.layer_norm(fr, (self.h,), gm, bt, EPS), (fr, gm, bt), v[:, self.real])
            gx, dg, db = torch.zeros(M, 128, dtype=dt), torch.zeros(128, dtype=dt), torch.zeros(128, dtype=dt)
            gx[:, self.real], dg[self.real], db[self.real] = gr
        else:
            gx, dg, db = (u.to(dt) for u in ln_bwd64(fx1, v, self.gamma, self.real, st))
        g_fx1 = gx + g
        return {"fx1": fx1, "z": z, "out": out, "g_z": g_z, "g_fx1": g_fx1, "g_out_x": g_fx1 @ t(self.Wout), "gamma": dg, "beta": db}


KINDS = {"fwd": Fwd, "bwd": Bwd, "mlp": Mlp, "trans": Trans, "mlp_dense": lambda h, lay, off: Mlp(h, lay, off, zero=False)}
_PROBLEMS = {}


def problem(kind, h, layout, offset, m=M):
    """Problems are built once and shared (their references are never modified).  m: rows (kinds "fwd" and "bwd")."""
    key = (kind, h, layout, offset, m)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = KINDS[kind](h, layout, offset) if m == M else KINDS[kind](h, layout, offset, m)
    return _PROBLEMS[key]


# ---- CPU backends ------------------------------------------------------------------------------------------------------------------
class Torch32:
    """float32 eager torch (F.linear, F.gelu, F.layer_norm over the h real columns): the reference implementation's arithmetic."""
    name = "torch32"

    def run(self, p):
        return p.evaluate(torch.float32, None)


class Emu:
    """float64 arithmetic on the float32 inputs, with the LayerNorm statistics formed in float32 by the kernels' rule on the
    float32-rounded LayerNorm input.  old=True: the parent revision's rule (the subtraction)."""

    def __init__(self, old=False, rule=None):
        self.rule = rule or ("old" if old else "new")
        self.name = f"emu-{self.rule}"

    def run(self, p):
        return p.evaluate(torch.float64, lambda x: stats32(x.float(), p.h, p.layout, self.rule))


# ---- judging -----------------------------------------------------------------------------------------------------------------------
def e32(p):
    """Per output of the problem: the largest row error (rows) / the relative error (sums) of Torch32 against float64."""
    if getattr(p, "_e32", None) is None:
        got, ref = Torch32().run(p), p.ref()
        d = {n: float(CR.row_err(got[n], ref[n]).max()) for n in p.rows}
        d.update({n: CR.rel(got[n], ref[n]) for n in p.sums})
        p._e32 = d
    return p._e32


def limit(p, name):
    base = CR.TOL_SUM if name in p.sums else CR.TOL_ROW
    if p.offset == 0:
        return base
    return max(base, 4.0 * e32(p).get(name, 0.0))


def judge(p, got, names=None, ref=None, margin=1.0):
    """[(name, value, limit, ok)]: rows by chain_rows.row_err, sums and statistics by chain_rows.rel; the padded columns of the
    row tensors in `zero_pad` exactly zero is the caller's assertion (padding_is_zero)."""
    ref = p.ref() if ref is None else ref
    out = []
    for n in (names or [k for k in got if k in p.rows or k in p.sums]):
        if n in p.rows:      # (128-column tensors: on the real columns; what the padding must hold is asserted apart)
            a, b = (got[n][:, p.real.to(got[n].device)], ref[n][:, p.real]) if ref[n].shape[1] == 128 else (got[n], ref[n])
            v = float(CR.row_err(a, b).max())
        else:
            v = CR.rel(got[n][p.real] if got[n].numel() == 128 else got[n], ref[n][p.real] if ref[n].numel() == 128 else ref[n])
        lim = limit(p, n) * margin
        out.append((f"{p.tag}/{n}", v, lim, v <= lim))
    return out


def failed(checks):
    return [c for c in checks if not c[3]]


def report(checks):
    return "\n".join(f"{'ok  ' if c[3] else 'FAIL'} {c[1]:.3e} (limit {c[2]:.3e})  {c[0]}" for c in checks)


def padding_is_zero(t, real):
    return bool((t.detach().cpu()[:, ~real] == 0).all())


def lnw_line(site, p, checks):
    """`LNW site h layout offset e_max limit`: the record of one GPU run (the check that is closest to its limit)."""
    worst = max(checks, key=lambda c: c[1] / c[2])
    return f"LNW {site} {p.h} {p.layout} {p.offset} {worst[1]:.2e} {worst[2]:.2e}"


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
class Gpu:
    """One launch site of tests/test_ln_width_gpu.py: `run(p)` launches twice on the same device tensors and returns the first
    run's tensors (on the CPU); `.path` is gfv_rowtile_last_path() of the launch, `.bit_equal` whether the two runs agree bit for
    bit, `.status` the device status word, `.pad_zero` the names whose padded columns must be exactly zero.  The caller pins the
    family with the gfv_limits fixture; `family` is what the launch itself is given."""
    SITES = {  # site: (problem kind, family pinned in the launch?)
        "row_fin_ln": "mlp", "cfwd_fin_ln": "mlp", "row_in_ln": "fwd", "lin1s_in_ln": "fwd", "lin1_in_ln": "fwd",
        "row_in_lnbwd": "bwd", "cbwd_in_lnbwd": "bwd", "row_fin_lnbwd": "bwd", "lin1s_fin_lnbwd": "bwd", "lin1_fin_lnbwd": "bwd",
        "transmlp": "trans", "ctrans": "trans"}

    def __init__(self, site):
        assert site in self.SITES
        self.site, self.name = site, site
        self.path = self.bit_equal = self.status = self.ln_rows = None
        self.pad_zero = ()

    # -- helpers
    @staticmethod
    def _d(t):
        return t.float().cuda().contiguous()

    @staticmethod
    def _wi(ws):
        from gfv import ops
        wmax = torch.stack([w.abs().max() for w in ws]).max().reshape(1).cuda()
        wi = ops.WeightImages(torch.device("cuda"), wmax)
        wi.static = [(0, 1 << 62)]
        return wi

    @staticmethod
    def _nan(*s):
        return torch.full(s, float("nan"), device="cuda")

    def _family(self):
        from gfv import lib as L
        return L.CHAIN_ROW_OWNER if self.site.startswith("row_") else 0

    def run(self, p, **kw):
        from gfv import lib as L
        lib = L.load()
        launch = getattr(self, "_" + {"row_fin_ln": "fin_ln", "cfwd_fin_ln": "fin_ln", "row_in_ln": "in_ln", "lin1s_in_ln": "in_ln",
                                      "lin1_in_ln": "in_ln", "row_in_lnbwd": "in_lnbwd", "cbwd_in_lnbwd": "in_lnbwd",
                                      "row_fin_lnbwd": "fin_lnbwd", "lin1s_fin_lnbwd": "fin_lnbwd", "lin1_fin_lnbwd": "fin_lnbwd",
                                      "transmlp": "trans", "ctrans": "trans"}[self.site])
        L.check(lib.gfv_set_hidden_size(p.h), "gfv_set_hidden_size")
        try:
            once = launch(p, **kw)
            a = once()
            self.path = lib.gfv_rowtile_last_path()
            b = once()
            torch.cuda.synchronize()
        finally:
            lib.gfv_set_hidden_size(128)
        self.bit_equal = all(torch.equal(a[k], b[k]) for k in a)
        flags = L.C.c_int32(0)
        L.check(lib.gfv_status_flags(L.C.byref(flags)), "gfv_status_flags")
        self.status = flags.value
        return {k: v.cpu() for k, v in a.items()}

    # -- GFV_FIN_LN: the 3-layer MLP with the final LayerNorm (row-owner chain / cfwd.hip), fin_presave + fin_stats
    def _fin_ln(self, p):
        from gfv import lib as L, ops
        d = self._d
        Pd = {k: d(getattr(p, k)) for k in ("W1", "b1", "W2", "b2", "W3", "b3", "gamma", "beta")}
        wi, xd = self._wi([p.W1, p.W2, p.W3]), d(p.x)
        self.pad_zero = ("y3", "out")

        def once():
            z1, z2, y3, out, st = self._nan(M, 128), self._nan(M, 128), self._nan(M, 128), self._nan(M, 128), self._nan(M, 2)
            ops.rowtile_chain(M, [ops.Seg(xd)], [ops.LayerSpec(Pd["W1"], Pd["b1"], L.OP_BIAS_GELU, save=z1),
                                                 ops.LayerSpec(Pd["W2"], Pd["b2"], L.OP_BIAS_GELU, save=z2), ops.LayerSpec(Pd["W3"], Pd["b3"])],
                              [out], fin_op=L.FIN_LN, fin_gamma=Pd["gamma"], fin_beta=Pd["beta"], fin_presave=y3, fin_stats=st,
                              res=[xd], wimg=wi, family=self._family())
            return {"y3": y3, "out": out, "stats": st}
        return once

    # -- GFV_IN_LN: LayerNorm prologue of one Linear (row-owner chain / lin1s.hip / lin1.hip)
    def _in_ln(self, p):
        from gfv import lib as L, ops
        d = self._d
        Wd, bd, gd, btd, xd = d(p.W), d(p.b), d(p.gamma), d(p.beta), d(p.x)
        wi, M = self._wi([p.W]), p.M
        self.pad_zero = ("out",)

        def once():
            out = self._nan(M, 128)
            ops.rowtile_chain(M, [ops.Seg(xd)], [ops.LayerSpec(Wd, bd)], [out], in_op=L.IN_LN, in_gamma=gd, in_beta=btd, wimg=wi,
                              family=self._family())
            return {"out": out}
        return once

    # -- GFV_IN_LNBWD: LayerNorm backward prologue + three transposed layers (row-owner chain: statistics recomputed from in_aux;
    #    cbwd.hip: read from in_stats), in_save = g3, ln_partial, gscale
    def _in_lnbwd(self, p, stats=None):
        from gfv import lib as L, ops
        d = self._d
        W3t, W2t, W1t = (ops.transpose(d(w)) for w in (p.W3, p.W2, p.W1))
        wi = self._wi([p.W1, p.W2, p.W3])
        god, yd, z1d, z2d, gd = d(p.go), d(p.y), d(p.z1), d(p.z2), d(p.gamma)
        self.pad_zero = ("ge",)
        self.last = {}

        def once():
            g3, gz2, gz1, ge = (self._nan(M, 128) for _ in range(4))
            part = self._nan(ops.ln_rows(M), 2, 128)
            gs = torch.zeros(3, ops.gscale_ld(M), device="cuda")
            layers = [ops.LayerSpec(W3t, None, L.OP_MUL_DGELU, save=gz2, aux=z2d), ops.LayerSpec(W2t, None, L.OP_MUL_DGELU, save=gz1, aux=z1d),
                      ops.LayerSpec(W1t)]
            ops.rowtile_chain(M, [ops.Seg(god)], layers, [ge], in_op=L.IN_LNBWD, in_gamma=gd, in_aux=yd, in_stats=stats, in_save=g3,
                              ln_partial=part, res=[god], gscale=gs, wimg=wi, family=self._family())
            n = ops.last_ln_rows()
            tot = part[:n].double().sum(0)
            self.last = dict(g3=g3, gs=gs, ln_rows=n)
            return {"g3": g3, "ge": ge, "gamma_in": tot[0].float(), "beta_in": tot[1].float()}
        return once

    # -- GFV_FIN_LNBWD: one Linear (256 -> 128) + LayerNorm backward epilogue + residual (row-owner chain / lin1s.hip / lin1.hip)
    def _fin_lnbwd(self, p):
        from gfv import lib as L, ops
        d = self._d
        Wd, gzd, yd, gd, rd = d(p.Wt), d(p.gz), d(p.y), d(p.gamma), d(p.res)
        wi, M = self._wi([p.Wt]), p.M
        segs = [ops.Seg(gzd, width=128, ld=256), ops.Seg(gzd, width=128, ld=256, offset=128)]

        def once():
            out = self._nan(M, 128)
            part = torch.zeros(ops.rowtile_tiles(M), 2, 128, device="cuda")
            ops.rowtile_chain(M, segs, [ops.LayerSpec(Wd)], [out], fin_op=L.FIN_LNBWD, fin_gamma=gd, fin_aux=yd, ln_partial=part,
                              res=[rd], wimg=wi, family=self._family())
            tot = part.double().sum(0)
            return {"gx": out, "gamma": tot[0].float(), "beta": tot[1].float()}
        return once

    # -- gfv_trans_mlp_fwd / gfv_trans_mlp_bwd (transmlp.hip / ctrans.hip)
    def _trans(self, p):
        from gfv import lib as L, ops
        d = self._d
        Pd = {k: d(getattr(p, k)) for k in ("Wout", "bout", "gamma", "beta", "Wpre", "bpre", "Wpost", "bpost")}
        wi = self._wi([p.Wout, p.Wpre, p.Wpost])
        xd, rd, god = d(p.x), d(p.res), d(p.gout)
        gad = torch.zeros(M, 128, device="cuda")
        self.pad_zero = ("fx1", "out", "g_out_x")

        def once():
            prev = ops.set_weight_images(wi)
            try:
                f1, zz, oo = self._nan(M, 128), self._nan(M, 256), self._nan(M, 128)
                assert ops.trans_mlp_fwd(xd, rd, Pd["Wout"], Pd["bout"], Pd["gamma"], Pd["beta"], Pd["Wpre"], Pd["bpre"], Pd["Wpost"],
                                         Pd["bpost"], f1, zz, oo)
                Wpost_t, Wpre_t, Wout_t = ops.transpose(Pd["Wpost"]), ops.transpose(Pd["Wpre"]), ops.transpose(Pd["Wout"])
                gsum, gz, gfx1, gox = self._nan(M, 128), self._nan(M, 256), self._nan(M, 128), self._nan(M, 128)
                part = torch.zeros(ops.ln_rows(M), 2, 128, device="cuda")
                gs = torch.zeros(3, ops.gscale_ld(M), device="cuda")
                assert ops.trans_mlp_bwd(god, gad, gsum, zz, f1, Wpost_t, Wpre_t, Wout_t, Pd["gamma"], gz, gfx1, gox, part, gs[0])
                self.ln_rows = L.load().gfv_trans_mlp_ln_rows(M)
                tot = part.double().sum(0)
            finally:
                ops.set_weight_images(prev)
            return {"fx1": f1, "z": zz, "out": oo, "g_z": gz, "g_fx1": gfx1, "g_out_x": gox, "gamma": tot[0].float(), "beta": tot[1].float()}
        return once
