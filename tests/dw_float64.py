"""The weight-gradient launch of csrc/dw.hip stated in plain torch, and the checks that tests/test_dw_float64_cpu.py and
tests/test_dw_float64_gpu.py share:

    dW[n,k] = sum_m G[m,n] * act(A[idx[m],k] + in_add[idx[m],k]),    db[n] = sum_m G[m,n]

act = identity, exact GELU (erf) or LayerNorm (eps 1e-5) over the REAL columns of a model of hidden size h inside the kernels'
128 columns (node layout: columns [:h]; edge layout: halves at columns 0 and 64).  Every statement follows the dtype it is
handed, so the same lines are the float64 reference (`Ref64`: the kernel's float32 inputs, upcast), its float32 evaluation on
the CPU (`Torch32`: what a correct float32 implementation leaves of a limit) and - with the operands rounded where the kernel
rounds them - the model of the reduced-precision product forms (`Emu`: gfv_set_f16split(2) / (3), fp16 / bf16 hi x hi).  `Gpu`
runs the library: ops.linear_dw (gfv_linear_dw_gs) for one-G cases, lib.gfv_dw_multi with lib.DwTile for the rest.

Limits (none is taken from the kernel):
  sum      |got - ref| <= 2e-6 * mag per entry, mag = sum_m |G| |act| of that entry's own terms: the budget
           test_rowtile_and_dw_extreme_dynamic_range gives a float32 sum, the "sum" limit of tests/slice_float64.py.  Forms 0 / 1
           against the float64 product; forms 2 / 3 (a given activation) against `Emu` and the mag of the rounded operands: TIGHT
           of tests/test_bf16_form_gpu.py.
  chained  max|got - ref| <= 2e-3 * max|ref| per tile: forms 2 / 3 rounding an activation the kernel computed itself (CHAINED of
           tests/test_bf16_form_gpu.py).
  floor    unscaled activations in the split-fp16 form: the low part of an activation is an fp16 number, quantum 2^-24 below
           2^-14, so every activation entry may be off by half a quantum: + 2^-25 * sum_m |G[m,n]|.
A float32 torch evaluation must keep a quarter of each (LIMITS[kind][1]).

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import collections
import dataclasses
import math

import torch

EPS = 1e-5
LIMITS = {"sum": (2e-6, 5e-7), "chained": (2e-3, 5e-4)}
FLOOR_Q = 2.0 ** -25          # half the fp16 subnormal quantum
FORM_DISTANCE = 1e-4          # forms 2 / 3 on flat O(1) operands: at least this far from the unrounded product
SENTINEL = -7253.0            # fills the buffers the outputs are views of
SUB = 32                      # rows per staged sub-tile (csrc/dw.hip)


# ---- the slab rule ---------------------------------------------------------------------------------------------------------------
def dw_slabs(M, ntiles):
    """(rows_per_slab, slabs) of gfv_dw_slabs with the default environment: ~256 workgroups per launch (512 from 200 000 rows
    on), shared among the tiles; slabs of a multiple of 32 rows, at least 64."""
    ntiles = max(ntiles, 1)
    wgs = 256 if M < 40000 else (256 if M < 200000 else 512)
    target = max(wgs // ntiles, 1)
    rows = -(-M // target)
    rows = max(-(-rows // 32) * 32, 64)
    return rows, -(-M // rows)


# rows_per_slab, slabs, rows of the last slab - by hand
SLAB_TABLE = {
    (0, 1): (64, 0, 0), (1, 1): (64, 1, 1), (31, 1): (64, 1, 31), (32, 1): (64, 1, 32), (33, 1): (64, 1, 33), (63, 1): (64, 1, 63),
    (64, 1): (64, 1, 64), (65, 1): (64, 2, 1), (97, 1): (64, 2, 33), (129, 1): (64, 3, 1), (333, 1): (64, 6, 13),
    (1100, 1): (64, 18, 12), (3001, 1): (64, 47, 57),
    (20011, 1): (96, 209, 43),     # ceil(20011 / 256) = 79 -> 96; 208 * 96 = 19968
    (9645, 2): (96, 101, 45),      # ceil(9645 / 128) = 76 -> 96; 100 * 96 = 9600
    (6001, 3): (96, 63, 49),       # ceil(6001 / 85) = 71 -> 96; 62 * 96 = 5952
    (3019, 6): (96, 32, 43),       # ceil(3019 / 42) = 72 -> 96; 31 * 96 = 2976
    (97, 6): (64, 2, 33), (97, 2): (64, 2, 33), (97, 3): (64, 2, 33), (333, 2): (64, 6, 13), (333, 3): (64, 6, 13),
}


def real_cols(h, layout="node"):
    m = torch.zeros(128, dtype=torch.bool)
    if layout == "node":
        m[:h] = True
    else:
        m[:h // 2] = True
        m[64:64 + h // 2] = True
    return m


def pow2_scale(m):
    """gfv_pow2_scale (csrc/gfv_split.h) on a float32 tensor m >= 0: 2^(13 - floor(log2 m)), biased exponent in [1, 253]."""
    e = (m.float().contiguous().view(torch.int32) >> 23) & 255
    return ((267 - e).clamp(1, 253) << 23).view(torch.float32)


def group_scales(G, M):
    """The per-16-row scales a chain launch leaves for gradient rows G[:M] (gfv_rowtile_args_t.gscale), by that rule."""
    n16 = (M + 15) // 16
    pad = torch.zeros(n16 * 16, G.shape[1])
    pad[:M] = G[:M]
    return pow2_scale(pad.view(n16, -1).abs().max(1).values)


# ---- case description ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class Tile:
    G: torch.Tensor            # [>= M, ldg] float32
    n_out: int
    A: torch.Tensor            # [R, ld] float32: rows idx[m] (or m), columns col .. col + width
    width: int
    g_offset: int = 0          # first column of G
    col: int = 0               # first column of A
    idx: torch.Tensor = None   # [M] int32 or None
    in_add: torch.Tensor = None   # [R, ld]: columns 0 .. width are added (same rows as A)
    a_op: int = 0              # 0 none, 1 GELU, 2 LayerNorm(gamma, beta)
    gamma: torch.Tensor = None
    beta: torch.Tensor = None
    colscale: bool = False
    gscale: torch.Tensor = None
    out_off: int = 0           # where dW[0, 0] sits in the block, its row stride, and the bias gradient (or -1)
    ld_out: int = 0
    db_off: int = -1

    @property
    def ldg(self):
        return self.G.shape[1]

    @property
    def ld(self):
        return self.A.shape[1]


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    M: int
    tiles: list
    form: int = 0              # gfv_set_f16split: 0 fp32 MFMA, 1 split fp16 (3 products), 2 fp16 hi x hi, 3 bf16
    hidden: int = 128
    layout: str = "node"
    linear: bool = True        # one G, segments side by side, in_add on the first: ops.linear_dw takes it
    block_floats: int = 0
    exact: bool = False        # small integers: every backend must give the integer result bit for bit
    flat: bool = False         # flat O(1) operands: forms 2 / 3 must be FORM_DISTANCE from the unrounded product
    floor: bool = False        # unscaled small activations: the split form gets the format's floor
    o1_cols: torch.Tensor = None
    ln_offset: float = 0.0     # a_op 2: |mean| / std of the LayerNorm input rows (judge)

    @property
    def narrow(self):
        """dw_narrow_kernel takes it (gfv_dw_multi, default environment): plain fp32 FMAs whatever the form."""
        t = self.tiles[0]
        return len(self.tiles) == 1 and t.width <= 16 and t.n_out == 128 and t.idx is None and t.in_add is None and t.a_op == 0


def lay_out(tiles, linear):
    """Offsets of every tile's dW / db inside the block; returns block_floats."""
    if linear:
        K, n_out = sum(t.width for t in tiles), tiles[0].n_out
        off = 0
        for i, t in enumerate(tiles):
            t.out_off, t.ld_out, t.db_off = off, K, (n_out * K if i == 0 else -1)
            off += t.width
        return (n_out * K + n_out + 3) // 4 * 4
    off = 0
    for t in tiles:
        t.out_off, t.ld_out = off, t.width
        off = (off + t.n_out * t.width + 3) // 4 * 4
        if t.db_off != -1:
            t.db_off = off
            off = (off + t.n_out + 3) // 4 * 4
    return off


def rows_of(t, M):
    return torch.arange(M) if t.idx is None else t.idx[:M].long()


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def gelu(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))


def layer_norm(a, gamma, beta, real):
    x = a[:, real]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    out = torch.zeros_like(a)
    out[:, real] = (x - mean) * torch.rsqrt(var + EPS) * gamma[real].to(a.dtype) + beta[real].to(a.dtype)
    return out


def assembled(t, M, dtype):
    """The rows the kernel loads: A[idx[m], col : col + width] (+ in_add)."""
    r = rows_of(t, M)
    a = t.A[r, t.col:t.col + t.width].to(dtype)
    if t.in_add is not None:
        a = a + t.in_add[r, :t.width].to(dtype)
    return a


def activation(t, case, dtype):
    a = assembled(t, case.M, dtype)
    if t.a_op == 1:
        a = gelu(a)
    elif t.a_op == 2:
        a = layer_norm(a, t.gamma, t.beta, real_cols(case.hidden, case.layout))
    return a


def grad_rows(t, M, dtype):
    return t.G[:M, t.g_offset:t.g_offset + t.n_out].to(dtype)


Result = collections.namedtuple("Result", "dW db magW magb")


class Ref64:
    """The float64 product, with the sum of the absolute values of every entry's terms."""
    dtype = torch.float64

    def run(self, case):
        out = []
        for t in case.tiles:
            g, a = grad_rows(t, case.M, self.dtype), activation(t, case, self.dtype)
            out.append(Result(g.T @ a, g.sum(0), (g.abs().T @ a.abs()).double(), g.abs().sum(0).double()))
        return out


class Torch32(Ref64):
    """The same statements in float32 on the CPU."""
    dtype = torch.float32


class Emu:
    """Forms 2 / 3: float64 arithmetic on operands rounded as the kernel rounds them - G times its slab's power of two, then
    fp16 / bf16; the activation (a float32 value: a given one as it is, a computed one from float64) times its power of two
    per column and slab when the tile asks for column scales, else as it is, then fp16 / bf16.  The bias gradient is the
    float32 column sum of the unrounded rows.  dw_narrow_kernel cases are the plain float64 product in every form."""

    def __init__(self, form):
        assert form in (2, 3)
        self.to = torch.float16 if form == 2 else torch.bfloat16

    def rnd(self, x):
        return x.float().to(self.to).double()

    def run(self, case):
        if case.narrow:
            return Ref64().run(case)
        rows, slabs = dw_slabs(case.M, len(case.tiles))
        out = []
        for t in case.tiles:
            g = grad_rows(t, case.M, torch.float32)
            a = assembled(t, case.M, torch.float32) if t.a_op == 0 else activation(t, case, torch.float64).float()
            dW, mag = torch.zeros(t.n_out, t.width, dtype=torch.float64), torch.zeros(t.n_out, t.width, dtype=torch.float64)
            for s in range(slabs):
                b, e = s * rows, min(case.M, (s + 1) * rows)
                if t.gscale is not None:
                    sg = t.gscale[b >> 4:(e + 15) >> 4].min()
                else:
                    sg = pow2_scale(g[b:e].abs().max())
                gr = self.rnd(g[b:e] * sg) / sg.double()
                if t.colscale:
                    sa = pow2_scale(a[b:e].abs().amax(0))
                    ar = self.rnd(a[b:e] * sa) / sa.double()
                else:
                    ar = self.rnd(a[b:e])
                dW += gr.T @ ar
                mag += gr.abs().T @ ar.abs()
            out.append(Result(dW, g.double().sum(0), mag, g.double().abs().sum(0)))
        return out


class Gpu:
    """The library.  Outputs are views inside a buffer filled with SENTINEL, which must survive around them; the workspace of
    ops.linear_dw starts as NaN (every slot that is reduced must have been written), that of gfv_dw_multi as zeros (what the
    header asks of the caller)."""

    def __init__(self, dev):
        self.dev = dev

    def _d(self, t):
        return None if t is None else t.to(self.dev).contiguous()

    def upload(self, case):
        """Device copies of a case's tensors, made once (a tensor shared by several tiles is uploaded once)."""
        memo = {}

        def d(t):
            if t is None:
                return None
            if id(t) not in memo:
                memo[id(t)] = self._d(t)
            return memo[id(t)]
        return [dict(G=d(t.G), A=d(t.A), idx=d(t.idx), in_add=d(t.in_add), gamma=d(t.gamma), beta=d(t.beta), gscale=d(t.gscale))
                for t in case.tiles]

    def linear(self, case, up=None, accumulate=False, prior=None, nan_workspace=True):
        """ops.linear_dw -> the block [dW | db] as one CPU tensor."""
        from gfv import lib as L, ops
        assert case.linear
        up = up or self.upload(case)
        t0, n_out, K = case.tiles[0], case.tiles[0].n_out, sum(t.width for t in case.tiles)
        buf = torch.full((n_out * K + n_out + 48,), SENTINEL, device=self.dev)
        dW, db = buf[16:16 + n_out * K].view(n_out, K), buf[32 + n_out * K:32 + n_out * K + n_out]
        if prior is not None:
            dW.copy_(prior[:n_out * K].view(n_out, K))
            db.copy_(prior[n_out * K:n_out * K + n_out])
        segs = [ops.Seg(u["A"], idx=u["idx"], width=t.width, ld=t.ld, offset=t.col) for t, u in zip(case.tiles, up)]
        need = L.load().gfv_linear_dw_workspace_floats(case.M, n_out, K)
        ws = torch.full((max(need, 1),), float("nan") if nan_workspace else 0.0, device=self.dev)
        ops.linear_dw(up[0]["G"], n_out, segs, case.M, ldg=t0.ldg, in_add=up[0]["in_add"], a_op=t0.a_op, a_gamma=up[0]["gamma"],
                      a_beta=up[0]["beta"], dW=dW, db=db, accumulate=accumulate, workspace=ws, g_offset=t0.g_offset,
                      gscale=up[0]["gscale"], col_scale=t0.colscale)
        torch.cuda.synchronize()
        host = buf.cpu()
        around = torch.cat((host[:16], host[16 + n_out * K:32 + n_out * K], host[32 + n_out * K + n_out:]))
        assert bool((around == SENTINEL).all()), f"{case.name}: a write outside dW / db"
        return torch.cat((host[16:16 + n_out * K], host[32 + n_out * K:32 + n_out * K + n_out]))

    def tiles_c(self, case, up):
        from gfv import lib as L
        ct = (L.DwTile * 6)()
        for c, t, u in zip(ct, case.tiles, up):
            c.G, c.A = u["G"].data_ptr() + 4 * t.g_offset, u["A"].data_ptr() + 4 * t.col
            c.idx = None if u["idx"] is None else u["idx"].data_ptr()
            c.in_add = None if u["in_add"] is None else u["in_add"].data_ptr()
            c.a_gamma = None if u["gamma"] is None else u["gamma"].data_ptr()
            c.a_beta = None if u["beta"] is None else u["beta"].data_ptr()
            c.gscale = None if u["gscale"] is None else u["gscale"].data_ptr()
            c.ldg, c.n_out, c.width, c.ld = t.ldg, t.n_out, t.width, t.ld
            c.a_op = t.a_op | (L.DW_COLSCALE if t.colscale else 0)
            c.ld_out, c.out_off, c.db_off = t.ld_out, t.out_off, t.db_off
        return ct

    def multi(self, case, up=None, accumulate=False, prior=None, reduce=True, workspace_fill=0.0):
        """lib.gfv_dw_multi -> the gradient block (reduce=True; "2d": grad_block = NULL and the caller's reduction), or the slab
        workspace [slabs, block_floats] as grad_block = NULL leaves it (reduce=False)."""
        from gfv import lib as L
        lib = L.load()
        up = up or self.upload(case)
        ct = self.tiles_c(case, up)
        nt, bf = len(case.tiles), case.block_floats
        slabs = lib.gfv_dw_slabs(case.M, nt, None)
        assert lib.gfv_dw_multi_workspace_floats(case.M, nt, bf) == slabs * bf
        wbuf = torch.full((slabs * bf + 32,), SENTINEL, device=self.dev)
        ws = wbuf[16:16 + slabs * bf]
        ws.fill_(workspace_fill)
        buf = torch.full((bf + 32,), SENTINEL, device=self.dev)
        block = buf[16:16 + bf]
        block.copy_(prior) if prior is not None else block.zero_()
        L.check(lib.gfv_dw_multi(ct, nt, case.M, bf, ws.data_ptr(), block.data_ptr() if reduce is True else None,
                                 1 if accumulate else 0, L.stream_ptr()), "gfv_dw_multi")
        if reduce == "2d":
            # the caller's own reduction, as the engine does it: gfv_reduce_partials_2d piece by piece where its alignment rules
            # allow (cols % 4 == 0), a float64 sum over the slabs for the others
            host = ws.view(slabs, bf).double().sum(0).float()
            for t in case.tiles:
                pieces = [(t.out_off, t.n_out, t.width)] + ([(t.db_off, 1, t.n_out)] if t.db_off >= 0 else [])
                for off, r, c in pieces:
                    if c % 4 == 0 and slabs > 0:
                        L.check(lib.gfv_reduce_partials_2d(ws.data_ptr() + 4 * off, slabs, bf, r, c, c, block.data_ptr() + 4 * off,
                                                           L.stream_ptr()), "gfv_reduce_partials_2d")
                    else:
                        block[off:off + r * c] = host[off:off + r * c]
        torch.cuda.synchronize()
        hw, hb = wbuf.cpu(), buf.cpu()
        for h in (hw, hb):
            assert bool((h[:16] == SENTINEL).all() and (h[-16:] == SENTINEL).all()), f"{case.name}: a write outside its buffers"
        return hb[16:16 + bf] if reduce else hw[16:16 + slabs * bf].view(slabs, bf)   # (True / "2d": the block)

    def run(self, case, **kw):
        block = self.linear(case, **kw) if case.linear else self.multi(case, **kw)
        return split_block(case, block)


def split_block(case, block):
    out = []
    for t in case.tiles:
        dW = block.as_strided((t.n_out, t.width), (t.ld_out, 1), block.storage_offset() + t.out_off)
        out.append(Result(dW, None if t.db_off < 0 else block[t.db_off:t.db_off + t.n_out], None, None))
    return out


def expected_block(case, results, prior=None):
    """The block a set of per-tile results makes (float64), on top of `prior` or zeros."""
    block = torch.zeros(case.block_floats, dtype=torch.float64) if prior is None else prior.double().clone()
    for t, r in zip(case.tiles, results):
        for n in range(t.n_out):
            block[t.out_off + n * t.ld_out:t.out_off + n * t.ld_out + t.width] += r.dW[n].double()
        if t.db_off >= 0:
            block[t.db_off:t.db_off + t.n_out] += r.db.double()
    return block


# ---- checks ----------------------------------------------------------------------------------------------------------------------
Check = collections.namedtuple("Check", "name kind value ok")


class Checks(list):
    def summed(self, name, got, ref, mag, floor=None, widen=1.0):
        """(the recorded value is divided by `widen` >= 1: judge(), cases with a LayerNorm row offset)
        |got - ref| <= 2e-6 * mag (+ floor) on every entry - an entry without terms must be zero -, and ref must not vanish
        next to mag on at least half of the entries that have terms (an all-zero output cannot pass; the dead columns of a
        LayerNorm over fewer than 128 real columns, or a zero column, have none)."""
        got, ref = got.double(), ref.double()
        err = (got - ref).abs()
        if floor is not None:
            err = (err - floor).clamp(min=0)
        v = float(torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).double()).max()) / widen
        self.append(Check(name, "sum", v, v < LIMITS["sum"][0]))
        frac = float(((ref.abs() >= 1e-3 * mag) & (mag > 0)).double().sum() / max(int((mag > 0).sum()), 1)) if mag.numel() else 1.0
        self.append(Check(name + ": entries with |ref| >= 1e-3 sum|terms|", "atleast", frac, frac >= 0.5))

    def chained(self, name, got, ref):
        v = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
        self.append(Check(name, "chained", v, v < LIMITS["chained"][0]))

    def equal(self, name, got, ref):
        """bit for bit (ref holds integers a float32 represents)"""
        bad = int((got.double() != ref.double()).sum())
        self.append(Check(name, "equal", bad, bad == 0 and bool(torch.isfinite(got).all())))

    def cond(self, name, value, ok):
        self.append(Check(name, "cond", float(value), bool(ok)))

    def failed(self, margin=False):
        """The checks that miss their limit (margin: the quarter limit a float32 torch evaluation must keep)."""
        return [c for c in self if not (c.ok and (not margin or c.kind not in LIMITS or c.value <= LIMITS[c.kind][1]))]

    def worst(self, kind):
        return max((c.value for c in self if c.kind == kind), default=0.0)

    def report(self):
        return "\n".join(f"{'ok  ' if c.ok else 'FAIL'} {c.kind:7s} {c.value:.3e}  {c.name}" for c in self)


_REF = {}


def reference(case):
    """The float64 reference of a case, computed once (cases are rebuilt from their seed: keyed by name and size)."""
    key = (case.name, case.M)
    if key not in _REF:
        _REF[key] = Ref64().run(case)
    return _REF[key]


_E32 = {}


def torch32_figure(case):
    """The largest |float32 torch - float64| / sum|terms| over the entries of a case's dW and db (computed once)."""
    key = (case.name, case.M)
    if key not in _E32:
        v = 0.0
        for g, r in zip(Torch32().run(case), reference(case)):
            for a, b, m in ((g.dW, r.dW, r.magW), (g.db, r.db, r.magb)):
                if a is not None and bool((m > 0).any()):
                    v = max(v, float(((a.double() - b.double()).abs()[m > 0] / m[m > 0]).max()))
        _E32[key] = v
    return _E32[key]


def judge(case, got, ck=None):
    """The checks of one case on a backend's results `got` ([Result] per tile).  A case whose LayerNorm input rows carry an offset
    (ln_offset: their mean is that many standard deviations from zero) is held to max(2e-6, 4 e32) of sum|terms|, e32 the figure of
    the float32 torch evaluation of the same case - tests/ln_width.py's rule: the reference's arithmetic keeps a quarter."""
    ck = Checks() if ck is None else ck
    ref = reference(case)
    widen = max(1.0, 4.0 * torch32_figure(case) / LIMITS["sum"][0]) if case.ln_offset else 1.0
    emu = Emu(case.form).run(case) if case.form in (2, 3) and not case.exact else None
    for i, (t, g, r) in enumerate(zip(case.tiles, got, ref)):
        tag = f"{case.name} M {case.M} form {case.form} tile {i}"
        if case.exact:
            ck.equal(tag + " dW", g.dW, r.dW)
            if g.db is not None:
                ck.equal(tag + " db", g.db, r.db)
            continue
        if g.db is not None:
            ck.summed(tag + " db", g.db, r.db, r.magb, widen=widen)
        if not case.floor and not t.colscale and case.M > 0:
            # (reference only) the fp16 floor of unscaled activations stays below a quarter of the limit where it is not granted
            has = r.magW > 0
            ratio = float((FLOOR_Q * r.magb[:, None].expand_as(r.magW)[has] / r.magW[has]).max()) if bool(has.any()) else 0.0
            ck.cond(tag + ": fp16 floor of the activations / sum|terms|", ratio, ratio <= LIMITS["sum"][1])
        if emu is None or case.narrow:
            floor = FLOOR_Q * r.magb[:, None].expand_as(r.dW) if (case.floor and case.form == 1 and not t.colscale) else None
            ck.summed(tag + " dW", g.dW, r.dW, r.magW, floor=floor, widen=widen)
            if floor is not None:    # (informative) how far the small columns are from the float64 product, and how much of the bound is used
                err = (g.dW.double() - r.dW).abs()
                ck.append(Check(tag + " dW / sum|terms| with no floor granted", "raw", float((err / r.magW).max()), True))
                ck.append(Check(tag + " dW / (2e-6 sum|terms| + floor)", "used", float((err / (LIMITS["sum"][0] * r.magW + floor)).max()), True))
        elif t.a_op == 0:
            ck.summed(tag + " dW (rounded operands)", g.dW, emu[i].dW, emu[i].magW)
            if case.flat:
                d = float(((g.dW.double() - r.dW).abs() / r.magW).max())
                ck.cond(tag + " distance to the unrounded product", d, d > FORM_DISTANCE)
        else:
            ck.chained(tag + " dW (rounded computed activation)", g.dW, emu[i].dW)
    return ck


def floor_conditions(case, ck=None):
    """On the O(1) columns of a small-activation case the floor must not excuse anything: below 1e-6 of mag (reference only)."""
    ck = Checks() if ck is None else ck
    for i, r in enumerate(reference(case)):
        ratio = float((FLOOR_Q * r.magb[:, None] / r.magW)[:, case.o1_cols].max())
        ck.cond(f"{case.name} tile {i}: floor / mag on the O(1) columns", ratio, ratio < 1e-6)
        small = float((FLOOR_Q * r.magb[:, None] / r.magW)[:, ~case.o1_cols].max())
        ck.cond(f"{case.name} tile {i}: floor / mag on the small columns (the floor is what is being tested)", small, small > 2e-6)
    return ck


# ---- the cases -------------------------------------------------------------------------------------------------------------------
ROW_MS = [1, 31, 32, 33, 63, 64, 65, 97, 129]
ROW_MS_LONG = [(20011, 1), (9645, 2), (6001, 3)]      # rows_per_slab 96, last slab = a full sub-tile + a tail that is no multiple of 4
GN = [(128, 128, 0), (64, 64, 0), (3, 3, 0), (3, 4, 0), (35, 35, 0), (128, 256, 128)]                  # n_out, ldg, g_offset
WL = [(128, 128, 0), (128, 256, 128), (64, 64, 0), (35, 35, 0), (17, 20, 0), (16, 16, 0), (15, 16, 0), (15, 15, 0), (12, 12, 0),
      (7, 7, 0), (1, 1, 0)]                                                                             # width, ld, column offset
UNNAMED = 977.0      # what source rows that no index names hold


def _seed(name, M):
    s = 17
    for ch in f"{name}/{M}":
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


A_MIN = 2.0 ** -4     # random activations keep this distance from zero: FLOOR_Q / A_MIN = 2^-21 < a quarter of the sum limit


def _values(g, shape, exact, lim, away=False):
    """Small integers (exact) or N(0, 1); away: pushed to |v| >= A_MIN, so that an entry whose few terms all have a tiny
    activation - which the split form, splitting activations unscaled, holds only to the fp16 floor - is left to the
    small-activation cases, where that floor is part of the bound."""
    if exact:
        return torch.randint(-lim, lim + 1, shape, generator=g).float()
    v = torch.randn(*shape, generator=g)
    return torch.where(v.abs() < A_MIN, torch.where(v < 0, -A_MIN, A_MIN), v) if away else v


def _index(g, M, R, A):
    """Indices with repeats, out of order, into R source rows; rows that none names hold UNNAMED."""
    idx = torch.randint(0, R, (M,), generator=g, dtype=torch.int32)
    named = torch.zeros(R, dtype=torch.bool)
    named[idx.long()] = True
    A[~named] = UNNAMED
    return idx


def linear_case(name, M, form=0, n_out=128, ldg=128, g_offset=0, segs=((128, 128, 0),), idx=None, in_add=False, a_op=0,
                hidden=128, layout="node", colscale=False, exact=False, flat=False, g_rows=None, a_cols=None, a_rows=None, zero_col=None,
                ln_offset=0.0):
    """One G, one to three segments (width, ld, column offset).  idx: None, "more" (a source of M + 37 rows) or "fewer"
    (of about M / 2).  g_rows / a_cols / a_rows: factors per row of G / per column / per source row of the first segment.
    ln_offset (a_op 2): added to the real columns of the LayerNorm input rows - their |mean| / std (tests/ln_width.py) - with an
    exact zero in the first real column of every 7th source row."""
    g = _seed(name, M)
    G = _values(g, (max(M, 1), ldg), exact, 2)
    if g_rows is not None:
        G = G * g_rows[:, None]
    real = real_cols(hidden, layout)
    tiles = []
    for i, (width, ld, col) in enumerate(segs):
        R = max(M, 1) if idx is None else (M + 37 if idx == "more" else max(M // 2, 1))
        A = _values(g, (R, ld), exact, 3, away=True)
        add = None
        if in_add and i == 0:
            add = _values(g, (R, ld), exact, 1)
        if a_op == 1:
            A = A.clamp(-3, 3)
            if add is not None:
                add = add.clamp(-3, 3)        # |z| <= 6
        if a_op == 2:
            A[:, col:col + width][:, ~real] = 0.0
            if add is not None:
                add[:, :width][:, ~real] = 0.0
            if ln_offset:
                A[:, col:col + width][:, real] += ln_offset
                A[::7, col] = 0.0
                if add is not None:
                    add[::7, 0] = 0.0
        if a_cols is not None and i == 0:
            A[:, col:col + width] *= a_cols
        if a_rows is not None and i == 0:
            A *= a_rows(R)[:, None]
        if zero_col is not None and i == 0:
            A[:, col + zero_col] = 0.0
        ix = None if idx is None else _index(g, M, R, A)
        t = Tile(G, n_out, A, width, g_offset=g_offset, col=col, idx=ix, in_add=add, a_op=a_op, colscale=colscale)
        if a_op == 2:
            t.gamma = torch.where(real, 1 + 0.2 * torch.randn(128, generator=g), torch.zeros(128))
            t.beta = torch.where(real, 0.2 * torch.randn(128, generator=g), torch.zeros(128))
        tiles.append(t)
    c = Case(name, M, tiles, form=form, hidden=hidden, layout=layout, exact=exact, flat=flat, ln_offset=ln_offset)
    c.block_floats = lay_out(tiles, True)
    return c


ROW_SEGS = {1: ((128, 128, 0),), 2: ((64, 64, 0), (128, 128, 0)), 3: ((128, 128, 0), (128, 128, 0), (15, 16, 0))}


def row_cases(form, exact):
    for M, nseg in [(M, 1) for M in ROW_MS] + ROW_MS_LONG:
        for idx in (None, "more", "fewer"):
            yield linear_case(f"rows{'-exact' if exact else ''} nseg {nseg} idx {idx}", M, form, segs=ROW_SEGS[nseg], idx=idx,
                              exact=exact, flat=not exact and idx is None and M in (33, 129))


def width_cases(form, exact, M):
    tag = "width-exact" if exact else "width"
    for n_out, ldg, goff in GN:
        for seg in WL:
            yield linear_case(f"{tag} G {n_out}/{ldg}+{goff} A {seg}", M, form, n_out, ldg, goff, segs=(seg,), exact=exact)
    for n_out, ldg, goff in ((128, 128, 0), (35, 35, 0)):
        for segs in (((64, 64, 0), (128, 128, 0)), ((128, 128, 0), (128, 256, 128), (15, 16, 0)), ((128, 128, 0), (7, 7, 0)),
                     ((15, 15, 0), (12, 12, 0), (1, 1, 0))):
            yield linear_case(f"{tag} G {n_out}/{ldg} segments {segs}", M, form, n_out, ldg, goff, segs=segs, exact=exact)
    # widths <= 16 where dw_narrow_kernel must NOT take them (the single plain segment above is where it does)
    for seg in ((16, 16, 0), (15, 16, 0), (15, 15, 0), (12, 12, 0), (7, 7, 0), (1, 1, 0)):
        yield linear_case(f"{tag} narrow {seg} + in_add", M, form, segs=(seg,), in_add=True, exact=exact)
        yield linear_case(f"{tag} narrow {seg} + idx", M, form, segs=(seg,), idx="more", exact=exact)


def onload_cases(form, M):
    yield linear_case("in_add", M, form, in_add=True)
    yield linear_case("in_add + idx + GELU", M, form, in_add=True, idx="more", a_op=1)
    yield linear_case("GELU, n_out 35", M, form, n_out=35, ldg=35, a_op=1)
    yield linear_case("LayerNorm h 128", M, form, a_op=2)
    yield linear_case("LayerNorm h 128 + in_add + idx", M, form, a_op=2, in_add=True, idx="fewer")
    yield linear_case("LayerNorm h 64 node, n_out 64", M, form, n_out=64, ldg=64, a_op=2, hidden=64)
    yield linear_case("LayerNorm h 64 node", M, form, a_op=2, hidden=64)
    yield linear_case("LayerNorm h 32 edge", M, form, a_op=2, hidden=32, layout="edge")


LN_OFFSETS = (8, 32)      # tests/ln_width.py OFFSETS; 0: onload_cases, and below for the widths those do not hold


def ln_offset_cases(form, M):
    """LayerNorm on load of rows whose mean is 8 / 32 standard deviations from zero, at every width and in both layouts, exact
    zeros inside real columns: a rule that subtracts (128 - h) mean^2 from a sum over all 128 columns loses
    (mean / std)^2 (128 - h) / h ulps of the variance here (csrc/gfv_common.h gfv_lnq_*)."""
    # (h = 16: a row of 16 samples can have a standard deviation below the 0.5 that onload_cases promise)
    yield linear_case("LayerNorm h 16 node offset 0", M, form, a_op=2, hidden=16)
    yield linear_case("LayerNorm h 16 edge offset 0", M, form, a_op=2, hidden=16, layout="edge")
    yield linear_case("LayerNorm h 112 edge offset 0", M, form, a_op=2, hidden=112, layout="edge")
    for off in LN_OFFSETS:
        for h, lay in ((16, "node"), (16, "edge"), (32, "edge"), (64, "node"), (112, "edge"), (128, "node")):
            yield linear_case(f"LayerNorm h {h} {lay} offset {off}", M, form, a_op=2, hidden=h, layout=lay, ln_offset=float(off))
        yield linear_case(f"LayerNorm h 32 node offset {off} + in_add + idx", M, form, a_op=2, hidden=32, in_add=True, idx="fewer",
                          ln_offset=float(off))


def decades(M):
    """gradient rows in blocks of decades (test_chain_group_scales_feed_the_weight_gradient)"""
    return 10.0 ** (torch.arange(max(M, 1)).float() // max(M // 6, 1) * 3 - 9)


def small_case(form, M, colscale):
    """Half the columns O(1), half at 1e-3 / 1e-4 / 1e-6, unscaled (the engine's 128-wide latent segments) or column-scaled."""
    o1 = torch.arange(128) % 2 == 0
    f = torch.ones(128)
    f[~o1] = torch.tensor([1e-3, 1e-4, 1e-6]).repeat(22)[:64]
    c = linear_case(f"small activations{' colscale' if colscale else ''}", M, form, a_cols=f, colscale=colscale)
    c.floor, c.o1_cols = not colscale, o1
    return c


def scale_cases(form):
    for M in (97, 129):
        r = torch.ones(M)
        r[64:128] = 0.0
        yield linear_case("zero slab of G", M, form, g_rows=r)
        yield linear_case("zero slab of G, colscale", M, form, g_rows=r, colscale=True)
    for M in (97, 333):
        yield linear_case("zero column of A, colscale", M, form, colscale=True, zero_col=5)
        yield linear_case("zero column of A, colscale, 15 / 16 + idx", M, form, segs=((15, 16, 0),), idx="more", colscale=True,
                          zero_col=5)
    for M in (33, 97, 129, 20011):
        yield linear_case("colscale, columns 1e-6 .. 1e+6", M, form, colscale=True, a_cols=10.0 ** torch.linspace(-6, 6, 128))
    for M in (33, 97, 129):
        yield linear_case("colscale, rows 1e-6 .. 1e+6 inside every column", M, form, colscale=True,
                          a_rows=lambda R: 10.0 ** ((torch.arange(R).double() * 0.6180339887 % 1) * 12 - 6).float())
    for M in (97, 1100, 20011):
        yield small_case(form, M, False)
        yield small_case(form, M, True)


def gscale_case(form, M, handed):
    c = linear_case("gscale", M, form, g_rows=decades(M))
    if handed:
        c.tiles[0].gscale = group_scales(c.tiles[0].G, M)
    return c


def multi_case(form, M, exact=False):
    """Six tiles on three gradient tensors, as the engine states the weight gradients of one MLP: own G per layer, some tiles
    without a bias gradient."""
    g = _seed("multi" + ("-exact" if exact else ""), M)
    G0, G1, G2 = (_values(g, (M, ld), exact, 2) for ld in (128, 256, 35))
    R = M + 37
    mk = lambda rows, ld: _values(g, (rows, ld), exact, 3, away=True)
    tiles = [Tile(G0, 128, mk(M, 128), 128, db_off=0),
             Tile(G0, 128, mk(M, 64), 64),
             Tile(G1, 128, mk(R, 128), 128, g_offset=128, db_off=0),
             Tile(G1, 128, mk(M, 256), 128, g_offset=128, col=128, in_add=_values(g, (M, 256), exact, 1)),
             Tile(G2, 35, mk(M, 20), 17, db_off=0),
             Tile(G2, 35, mk(M, 128), 128)]
    if not exact:
        tiles[2].a_op = 1
        tiles[2].A.clamp_(-6, 6)
        tiles[5].a_op, tiles[5].gamma, tiles[5].beta = 2, 1 + 0.2 * torch.randn(128, generator=g), 0.2 * torch.randn(128, generator=g)
    tiles[2].idx = _index(g, M, R, tiles[2].A)
    c = Case("multi" + ("-exact" if exact else ""), M, tiles, form=form, linear=False, exact=exact)
    c.block_floats = lay_out(tiles, False)
    return c


def empty_cases():
    yield linear_case("M = 0", 0, 0)
    yield linear_case("M = 0, three segments", 0, 0, n_out=35, ldg=35, segs=ROW_SEGS[3])
