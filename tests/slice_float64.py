"""The Transolver block's physics attention (GraphTransolver.py:64-92) stated step by step in plain torch, and the checks of
csrc/slice.hip / gfv_reduce_partials_seg that tests/test_slice_gpu.py, tests/test_slice_float64_cpu.py and
tests/slice_scalar_worker.py share.

Every step takes the tensors it is handed and follows their dtype, so the same lines serve as the float64 reference (a kernel's
actual float32 inputs, upcast) and - evaluated in float32 on the CPU (`Torch32`) - as the measure of what a correct float32
implementation leaves of the limits below.  The adjoints come from autograd; a softmax whose OUTPUT a kernel was handed (w,
attn: saved by the forward, not recomputed by the backward) takes that output as given (`softmax(z, given=y)`).

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import collections
import contextlib

import torch

H, D, G = 8, 16, 32
EPS = 1e-5                       # GraphTransolver.py:74
NODE_SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 130, 513]   # >= 3 graphs in one 32-node workgroup, boundaries on and off
#                                  multiples of 32, chunk lengths 1, 15, 16, 17, 63 and a full 64 followed by a 1-node chunk
ATTN_CHUNKS = [1, 7, 8, 9, 17, 0]   # chunks per graph: below, at and above the 8-wide walk, two rounds + tail, an empty graph
SEG_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 0, 129]   # gfv_reduce_partials_seg: tail only, one stride of 16, the 4x body + tail

# kind -> (limit, limit a float32 torch evaluation of the same statements must keep: a quarter of it)
#   elem: max|got - ref| / max|ref| (the project's TOL of test_kernels_gpu.py / test_slice_gpu.py)
#   sum:  max over the elements of |got - ref| / (float64 sum of the absolute values of that element's own terms): the budget
#         test_rowtile_and_dw_extreme_dynamic_range gives a float32 sum
LIMITS = {"elem": (1e-5, 2.5e-6), "sum": (2e-6, 5e-7)}

Check = collections.namedtuple("Check", "name kind value ok")


class Checks(list):
    def elem(self, name, got, ref):
        v = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
        self.append(Check(name, "elem", v, v < LIMITS["elem"][0]))

    def summed(self, name, got, ref, mag):
        """got against ref, every element judged against mag = sum |terms| of that element; and ref must not vanish next to
        mag (a zero output cannot pass)."""
        v = float(((got.double() - ref).abs() / mag).max())
        self.append(Check(name, "sum", v, v < LIMITS["sum"][0]))
        nz = float(ref.abs().max() / mag.max())
        self.append(Check(name + " |ref| / sum|terms|", "atleast", nz, nz >= 1e-3))

    def cond(self, name, value, ok):
        self.append(Check(name, "cond", float(value), bool(ok)))

    def failed(self, margin=False):
        """The checks that miss their limit (margin: the quarter limit a float32 torch evaluation must keep)."""
        bad = []
        for c in self:
            ok = c.ok and (not margin or c.kind not in LIMITS or c.value <= LIMITS[c.kind][1])
            if not ok:
                bad.append(c)
        return bad

    def report(self):
        return "\n".join(f"{'ok  ' if c.ok else 'FAIL'} {c.kind:7s} {c.value:.3e}  {c.name}" for c in self)


# ---- the block, step by step ---------------------------------------------------------------------------------------------------
class _SoftmaxGiven(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y):
        ctx.save_for_backward(y)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return y * (g - (y * g).sum(-1, keepdim=True)), None


def softmax(z, given=None):
    """softmax over the last axis; `given`: its output as a kernel was handed it - returned as is, the adjoint taken at it."""
    return torch.softmax(z, -1) if given is None else _SoftmaxGiven.apply(z, given)


def slice_logits(xmid, Ws, bs, temp):
    """in_project_slice(x_mid) and z = logits / graph_temperature (:61-63): [N, 8, 32] each."""
    logits = torch.einsum("nhc,gc->nhg", xmid.view(-1, H, D), Ws) + bs
    return logits, logits / temp.view(1, H, 1)


def chunk_tokens(w, a, cb, ce):
    """Per-chunk sums [n_chunks, 256, 17] of (:64-73): slots 0..15 sum_n w[n,h,g] a[n,h,c], slot 16 sum_n w[n,h,g]."""
    w, a = w.view(-1, H, G), a.view(-1, H, D)
    out = w.new_zeros(len(cb), H, G, D + 1)
    for k, (b, e) in enumerate(zip(cb, ce)):
        out[k, :, :, :D] = torch.einsum("nhg,nhc->hgc", w[b:e], a[b:e])
        out[k, :, :, D] = w[b:e].sum(0)
    return out.view(len(cb), H * G, D + 1)


def segment_sum(rows, ptr):
    """out[b] = sum of rows[ptr[b] : ptr[b + 1]] (an empty segment: zeros)."""
    out = rows.new_zeros((len(ptr) - 1,) + tuple(rows.shape[1:]))
    for b in range(len(ptr) - 1):
        out[b] = rows[ptr[b]:ptr[b + 1]].sum(0)
    return out


def _attention_from_token(tok, W, scale, attn=None):
    """(:77-83) q / k / v, softmax(q k^T scale) - or the attn handed -, out_token."""
    r = dict(token=tok)
    r["q"], r["k"], r["v"] = tok @ W[0].T, tok @ W[1].T, tok @ W[2].T
    r["dots"] = r["q"] @ r["k"].transpose(-1, -2) * scale
    r["attn"] = softmax(r["dots"], given=attn)
    r["out_token"] = r["attn"] @ r["v"]
    return r


def attention(sums, Wq, Wk, Wv, scale):
    """(:74-83) from the per-graph sums [B, 256, 17]: token = raw / (norm + 1e-5), then the attention among the 32 tokens."""
    B = sums.shape[0]
    raw, norm = sums[:, :, :D].reshape(B, H, G, D), sums[:, :, D].reshape(B, H, G)
    return dict(_attention_from_token(raw / (norm.unsqueeze(-1) + EPS), (Wq, Wk, Wv), scale), raw=raw, norm=norm)


def deslice(w, T, batch):
    """(:86-91) out[n,h,c] = sum_g w[n,h,g] T[b(n),h,g,c] -> [N, 128]."""
    return torch.einsum("nhg,nhgc->nhc", w.view(-1, H, G), T[batch]).reshape(-1, H * D)


def slice_gw(a, T, batch, add=None):
    """The adjoint of the de-slice / token sums wrt w: sum_c a[n,h,c] T[b(n),h,g,c] (+ add[b(n),h,g]) -> [N, 256]."""
    r = torch.einsum("nhc,nhgc->nhg", a.view(-1, H, D), T[batch])
    return (r if add is None else r + add[batch]).reshape(-1, H * G)


def slice_softmax_adjoint(xmid, Ws, bs, temp, w, gw):
    """The adjoint of w = softmax((x_mid Ws^T + bs) / T) at the w handed, for the cotangent gw: g_x_mid and the parameter
    gradients, each with the sum of the absolute values of its terms (from the retained gradients of logits and z)."""
    x, Ws, bs, temp = (t.detach().clone().requires_grad_(True) for t in (xmid, Ws, bs, temp))
    logits, z = slice_logits(x, Ws, bs, temp)
    logits.retain_grad()
    z.retain_grad()
    softmax(z, given=w.view(-1, H, G)).backward(gw.view(-1, H, G))
    gl, xa = logits.grad.abs(), x.detach().view(-1, H, D).abs()
    return dict(gx=x.grad, dWs=Ws.grad, dbs=bs.grad, dT=temp.grad, dWs_mag=torch.einsum("nhg,nhc->gc", gl, xa), dbs_mag=gl.sum((0, 1)),
                dT_mag=((z.grad * z.detach()).abs() / temp.detach().view(1, H, 1)).sum((0, 2)))


def attention_adjoint(token, norm, attn, g_out, Wq, Wk, Wv, scale):
    """The adjoint of `attention` at the saved token / norm / attn for the cotangent g_out of out_token: g_raw, g_norm, dWq / dWk /
    dWv [3, 16, 16] and the sums of the absolute values of their terms (from the retained gradients of q, k, v)."""
    tok = token.detach().clone().requires_grad_(True)
    W = [t.detach().clone().requires_grad_(True) for t in (Wq, Wk, Wv)]
    r = _attention_from_token(tok, W, scale, attn)
    for n in "qkv":
        r[n].retain_grad()
    r["out_token"].backward(g_out)
    # token = raw / (norm + eps) at the raw that gives the saved token
    raw = (token * (norm.unsqueeze(-1) + EPS)).detach().requires_grad_(True)
    nrm = norm.detach().clone().requires_grad_(True)
    (raw / (nrm.unsqueeze(-1) + EPS)).backward(tok.grad)
    ta = token.abs()
    return dict(g_raw=raw.grad, g_norm=nrm.grad, dW=torch.stack([t.grad for t in W]),
                dW_mag=torch.stack([torch.einsum("bhgj,bhgc->jc", r[n].grad.abs(), ta) for n in "qkv"]))


# ---- inputs that make the non-trivial terms large -------------------------------------------------------------------------------
# name -> (graph sizes, seed, scale of Ws, whether max w > 0.99 is a precondition).  Seeds and scales are the first at which the
# float32 torch evaluation keeps the quarter limits of LIMITS with room (tests/test_slice_float64_cpu.py asserts it).  The
# two smallest batches run below Ws ~ N(0, 1): with 8 or 256 (node, head) rows the parameter gradients are sums of few terms, a
# sharp row's gz = w (gw - <w, gw>) is all cancellation, and the sum of |terms| - taken behind that cancellation - does not
# cover it: float32 torch itself left 5e-7 .. 1.3e-6 on [5, 7, 9, 11] and 9e-7 .. 3e-2 on [1] at full scale (no seed of 40
# within 5e-7 on [1]), hence 0.5 there and 0.25 on [1], where w > 0.99 no longer occurs.
NODE_CASES = {"thirteen_graphs": (NODE_SIZES, 15, 1.0, True), "four_graphs_one_workgroup": ([5, 7, 9, 11], 13, 0.5, True),
              "one_node": ([1], 18, 0.25, False), "one_graph_96": ([96], 15, 1.0, True)}
ATTN_SEED, SEG_SEED = 25, 31


def node_case(sizes, seed, ws_scale=1.0, sharp=True):
    """Sharp slice weights: Ws ~ ws_scale N(0, 1), bs ~ 0.3 N, temperatures in [0.3, 1.5].  Chunks of 64 nodes inside each
    graph (gfv/plan.py)."""
    g = torch.Generator().manual_seed(seed)
    N, B = sum(sizes), len(sizes)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    cb, ce, start = [], [], 0
    for n in sizes:
        for s0 in range(start, start + n, 64):
            cb.append(s0)
            ce.append(min(s0 + 64, start + n))
        start += n
    return dict(sizes=list(sizes), N=N, B=B, batch=torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)), cb=cb, ce=ce,
                sharp=sharp, xmid=r(N, 128), fxm=r(N, 128), gox=r(N, 128), Ws=r(G, D, scale=ws_scale), bs=r(G, scale=0.3),
                temp=0.3 + 1.2 * torch.rand(H, generator=g), T1=r(B, H, G, D), T2=r(B, H, G, D, scale=0.2),
                gn=r(B, H, G, scale=0.1), base=r(N, 128))


def attention_case(seed, hidden):
    """Per-chunk partials of ATTN_CHUNKS graphs - the float64 token sums of sharp slice weights over chunks of 1 .. 64 nodes,
    rounded to float32 - and Wq, Wk ~ 0.6 N (at the scale 0.25 of hidden 128; the same dots at another hidden size), Wv ~ 0.3 N."""
    g = torch.Generator().manual_seed(seed)
    nch = sum(ATTN_CHUNKS)
    lens = torch.randint(1, 65, (nch,), generator=g).tolist()
    lens[:8] = [1 + n % 4 for n in lens[:8]]   # the first two graphs: 1 .. 4 nodes a chunk, many of their slice norms far below eps
    ce = torch.tensor(lens).cumsum(0).tolist()
    cb = [0] + ce[:-1]
    N = ce[-1]
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * scale
    temp = 0.3 + 1.2 * torch.rand(H, generator=g, dtype=torch.float64)
    w = softmax(slice_logits(r(N, 128), r(G, D), r(G, scale=0.3), temp)[1])
    scale = (hidden / 8) ** -0.5
    qk = 0.6 * (0.25 / scale) ** 0.5
    ptr = [0]
    for n in ATTN_CHUNKS:
        ptr.append(ptr[-1] + n)
    return dict(hidden=hidden, scale=scale, ptr=ptr, B=len(ATTN_CHUNKS), partial=chunk_tokens(w, r(N, 128), cb, ce).float(),
                gpartial=chunk_tokens(w, r(N, 128), cb, ce).float(), Wq=r(D, D, scale=qk).float(), Wk=r(D, D, scale=qk).float(),
                Wv=r(D, D, scale=0.3).float())


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def node_checks(c, impl):
    """The node kernels of csrc/slice.hip on one batch: each against float64 of the tensors it was handed."""
    ck = Checks()
    d = lambda t: t.double()
    batch, cb, ce, single = c["batch"], c["cb"], c["ce"], c["B"] == 1
    wref = softmax(slice_logits(d(c["xmid"]), d(c["Ws"]), d(c["bs"]), d(c["temp"]))[1]).reshape(-1, H * G)
    if c["sharp"]:
        ck.cond("precondition: max w > 0.99", wref.max(), wref.max() > 0.99)
    if len(c["sizes"]) > 4:
        nrm = segment_sum(wref, [0] + torch.tensor(c["sizes"]).cumsum(0).tolist())
        small = float((nrm < 1e-5).double().mean())
        ck.cond("precondition: >= 1 % of the slice norms < 1e-5", small, small >= 0.01)
        ck.cond("precondition: a slice norm > 1", nrm.max(), nrm.max() > 1)
    w_fwd = impl.softmax_fwd(c)
    w, part = impl.softmax_token(c, c["fxm"])
    ck.elem("softmax_fwd w", w_fwd, wref)
    ck.elem("softmax_token w", w, wref)
    ck.elem("softmax_fwd w against softmax_token w", w_fwd, w)
    # from here on w is the forward's own
    for name, got, a in (("softmax_token", part, c["fxm"]), ("token_partial", impl.token_partial(c, w, c["gox"]), c["gox"])):
        ref = chunk_tokens(d(w), d(a), cb, ce)
        err = (d(got) - ref).abs()
        ck.append(_per_chunk(name + " tokens, every chunk by its own max", err[:, :, :D], ref[:, :, :D]))
        ck.append(_per_chunk(name + " norms, every chunk by its own max", err[:, :, D:], ref[:, :, D:]))
    ref = deslice(d(w), d(c["T1"]), batch)
    for acc in (0, 1) + ((4,) if single else ()):
        ck.elem(f"deslice accumulate={acc}", impl.deslice(c, w, c["T1"], acc, c["base"]), ref + d(c["base"]) if acc == 1 else ref)
    # the four launches behind the attention: gw, de-slice of g_raw, gw on top of it, the slice-softmax adjoint at that gw
    gw1 = impl.slice_gw(c, c["gox"], c["T1"], None, None)
    ck.elem("slice_gw", gw1, slice_gw(d(c["gox"]), d(c["T1"]), batch))
    gw2 = impl.slice_gw(c, c["fxm"], c["T2"], c["gn"], gw1)
    ck.elem("slice_gw accumulate=1 + g_norm", gw2, d(gw1) + slice_gw(d(c["fxm"]), d(c["T2"]), batch, d(c["gn"])))
    gfx_ref = deslice(d(w), d(c["T2"]), batch)
    ck.elem("deslice of g_raw", impl.deslice(c, w, c["T2"], 0, c["base"]), gfx_ref)
    _adjoint_checks(ck, "softmax_bwd", impl.softmax_bwd(c, w, gw2), c, w, d(gw2))
    # ... and the one pass
    got = impl.post_bwd(c, w)
    gw = slice_gw(d(c["gox"]), d(c["T1"]), batch) + slice_gw(d(c["fxm"]), d(c["T2"]), batch, d(c["gn"]))
    ck.elem("post_bwd g_fx_mid", got["gfx"], gfx_ref)
    _adjoint_checks(ck, "post_bwd", got, c, w, gw)
    return ck


def _per_chunk(name, err, ref):
    v = float((err.flatten(1).max(1).values / ref.abs().flatten(1).max(1).values).max())
    return Check(name, "elem", v, v < LIMITS["elem"][0])


def _adjoint_checks(ck, name, got, c, w, gw):
    d = lambda t: t.double()
    ref = slice_softmax_adjoint(d(c["xmid"]), d(c["Ws"]), d(c["bs"]), d(c["temp"]), d(w), gw)
    ck.elem(name + " g_x_mid", got["gx"], ref["gx"].reshape(-1, H * D))
    for n in ("dWs", "dbs", "dT"):
        ck.summed(f"{name} {n}", got[n], ref[n], ref[n + "_mag"])


def attention_checks(c, impl):
    """gfv_slice_attention_fwd / _bwd walking the chunks of each graph themselves, then fed the per-graph sums with a unit
    pointer (the engine's call); the forward-only launch; the empty graph."""
    ck = Checks()
    d = lambda t: t.double()
    W = (c["Wq"], c["Wk"], c["Wv"])
    W64 = tuple(d(t) for t in W)
    B, ptr, empty = c["B"], c["ptr"], ATTN_CHUNKS.index(0)
    sums64, gsums64 = segment_sum(d(c["partial"]), ptr), segment_sum(d(c["gpartial"]), ptr)
    r = attention(sums64, *W64, c["scale"])
    nonempty = [b for b in range(B) if b != empty]
    small = float((r["norm"][nonempty] < 1e-5).double().mean())
    ck.cond("precondition: >= 1 % of the slice norms of the graphs with nodes < 1e-5", small, small >= 0.01)
    ck.cond("precondition: a slice norm > 1", r["norm"].max(), r["norm"].max() > 1)
    ck.cond("precondition: max attn > 0.9", r["attn"].max(), r["attn"].max() > 0.9)
    ck.cond("precondition: max |dots| <= 20", r["dots"].abs().max(), r["dots"].abs().max() <= 20)
    unit = list(range(B + 1))
    for how, part, gpart, p in (("chunk walk", c["partial"], c["gpartial"], ptr), ("unit pointer", sums64.float(), gsums64.float(), unit)):
        ref = attention(segment_sum(d(part), p), *W64, c["scale"])
        got = impl.attention_fwd(part, p, W, c["hidden"], keep=True)
        for n in ("token", "norm", "attn", "out_token"):
            ck.elem(f"attention_fwd {how} {n}", got[n], ref[n])
        z = max(float(got[n][empty].abs().max()) for n in ("token", "norm", "out_token"))
        ck.cond(f"attention_fwd {how}: the empty graph gives zeros", z, z == 0.0)
        fo = impl.attention_fwd(part, p, W, c["hidden"], keep=False)["out_token"]
        ck.cond(f"attention_fwd {how}: forward-only out_token bit-equal", (fo != got["out_token"]).sum(), torch.equal(fo, got["out_token"]))
        # the backward reads what the forward saved
        g_out = segment_sum(d(gpart), p)[:, :, :D].reshape(B, H, G, D)
        ref = attention_adjoint(d(got["token"]), d(got["norm"]), d(got["attn"]), g_out, *W64, c["scale"])
        bw = impl.attention_bwd(gpart, p, W, c["hidden"], got["token"], got["norm"], got["attn"])
        ck.elem(f"attention_bwd {how} g_raw", bw["g_raw"], ref["g_raw"])
        ck.elem(f"attention_bwd {how} g_norm", bw["g_norm"], ref["g_norm"])
        for i, n in enumerate(("dWq", "dWk", "dWv")):
            ck.summed(f"attention_bwd {how} {n}", bw["dW"][i], ref["dW"][i], ref["dW_mag"][i])
        z = max(float(bw[n][empty].abs().max()) for n in ("g_raw", "g_norm"))
        ck.cond(f"attention_bwd {how}: the empty graph gives zeros", z, z == 0.0)
    return ck


def seg_case(seed):
    g = torch.Generator().manual_seed(seed)
    ptr = [0]
    for n in SEG_LENGTHS:
        ptr.append(ptr[-1] + n)
    return dict(ptr=ptr, rows=torch.randn(ptr[-1], 256 * 17, generator=g))


def seg_checks(c, impl):
    ck = Checks()
    rows = c["rows"].double()
    ref, mag = segment_sum(rows, c["ptr"]), segment_sum(rows.abs(), c["ptr"])
    got = impl.reduce_seg(c["rows"], c["ptr"])
    empty = SEG_LENGTHS.index(0)
    ck.cond("reduce_partials_seg: the empty segment is written as zeros", got[empty].abs().max(), bool((got[empty] == 0).all()))
    ck.elem("reduce_partials_seg", got, ref)
    mag[empty] = 1.0
    v = float(((got.double() - ref).abs() / mag).max())
    ck.append(Check("reduce_partials_seg, every element by its own sum |terms|", "sum", v, v < LIMITS["sum"][0]))
    return ck


# ---- the two implementations the checks run on ---------------------------------------------------------------------------------
class Torch32:
    """The statements above in float32 torch on the CPU."""

    def softmax_fwd(self, c):
        return softmax(slice_logits(c["xmid"], c["Ws"], c["bs"], c["temp"])[1]).reshape(-1, H * G)

    def softmax_token(self, c, a):
        w = self.softmax_fwd(c)
        return w, self.token_partial(c, w, a)

    def token_partial(self, c, w, a):
        return chunk_tokens(w, a, c["cb"], c["ce"])

    def deslice(self, c, w, T, accumulate, base):
        r = deslice(w, T, c["batch"])
        return r + base if accumulate == 1 else r

    def slice_gw(self, c, a, T, add, base):
        r = slice_gw(a, T, c["batch"], add)
        return r if base is None else base + r

    def softmax_bwd(self, c, w, gw):
        return slice_softmax_adjoint(c["xmid"], c["Ws"], c["bs"], c["temp"], w, gw)

    def post_bwd(self, c, w):
        gw = slice_gw(c["gox"], c["T1"], c["batch"]) + slice_gw(c["fxm"], c["T2"], c["batch"], c["gn"])
        return dict(self.softmax_bwd(c, w, gw), gfx=deslice(w, c["T2"], c["batch"]))

    def reduce_seg(self, rows, ptr):
        return segment_sum(rows, ptr)

    def attention_fwd(self, partial, ptr, W, hidden, keep):
        return attention(segment_sum(partial, ptr), *W, (hidden / 8) ** -0.5)

    def attention_bwd(self, gpartial, ptr, W, hidden, token, norm, attn):
        g_out = segment_sum(gpartial, ptr)[:, :, :D].reshape(-1, H, G, D)
        return attention_adjoint(token, norm, attn, g_out, *W, (hidden / 8) ** -0.5)


class Gpu:
    """The C ABI of include/gfv.h on the current device: CPU tensors in, CPU tensors out; every output buffer starts as NaN;
    the per-block partials of the parameter gradients are summed in float64."""

    def __init__(self):
        from gfv import lib as L
        self.L, self.lib, self.st = L, L.load(), L.stream_ptr()

    @staticmethod
    def _up(*ts):
        return [None if t is None else t.cuda().contiguous() for t in ts]

    @staticmethod
    def _nan(*shape):
        return torch.full(shape, float("nan"), device="cuda")

    @staticmethod
    def _i32(v):
        return (v if torch.is_tensor(v) else torch.tensor(v)).int().cuda()

    def _done(self, rc, what, *outs):
        self.L.check(rc, what)
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]

    @contextlib.contextmanager
    def _hidden(self, h):
        self.L.check(self.lib.gfv_set_hidden_size(h), "gfv_set_hidden_size")
        try:
            yield
        finally:
            self.lib.gfv_set_hidden_size(128)

    @staticmethod
    def _partials(sp):
        s = sp.double().sum(0)
        return dict(dWs=s[:512].view(G, D), dbs=s[512:544], dT=s[544:552])

    def softmax_fwd(self, c):
        x, Ws, bs, t = self._up(c["xmid"], c["Ws"], c["bs"], c["temp"])
        w = self._nan(c["N"], H * G)
        return self._done(self.lib.gfv_slice_softmax_fwd(x.data_ptr(), Ws.data_ptr(), bs.data_ptr(), t.data_ptr(), w.data_ptr(), c["N"],
                                                         self.st), "slice_softmax_fwd", w)[0]

    def softmax_token(self, c, a):
        x, Ws, bs, t, a = self._up(c["xmid"], c["Ws"], c["bs"], c["temp"], a)
        cb, ce, nch = self._i32(c["cb"]), self._i32(c["ce"]), len(c["cb"])
        w, part = self._nan(c["N"], H * G), self._nan(nch, H * G, D + 1)
        return self._done(self.lib.gfv_slice_softmax_token(x.data_ptr(), Ws.data_ptr(), bs.data_ptr(), t.data_ptr(), a.data_ptr(),
                                                           cb.data_ptr(), ce.data_ptr(), nch, w.data_ptr(), part.data_ptr(), self.st),
                          "slice_softmax_token", w, part)

    def token_partial(self, c, w, a):
        w, a = self._up(w, a)
        cb, ce, nch = self._i32(c["cb"]), self._i32(c["ce"]), len(c["cb"])
        part = self._nan(nch, H * G, D + 1)
        return self._done(self.lib.gfv_slice_token_partial(w.data_ptr(), a.data_ptr(), cb.data_ptr(), ce.data_ptr(), nch, part.data_ptr(),
                                                           self.st), "slice_token_partial", part)[0]

    def deslice(self, c, w, T, accumulate, base):
        assert accumulate in (0, 1) or (accumulate == 4 and c["B"] == 1)   # bit 2: the caller vouches for a one-graph batch
        w, T = self._up(w, T)
        out = base.cuda().contiguous() if accumulate == 1 else self._nan(c["N"], H * D)
        return self._done(self.lib.gfv_deslice(w.data_ptr(), T.data_ptr(), self._i32(c["batch"]).data_ptr(), out.data_ptr(), c["N"],
                                               accumulate, self.st), "deslice", out)[0]

    def slice_gw(self, c, a, T, add, base):
        a, T, add = self._up(a, T, add)
        gw = self._nan(c["N"], H * G) if base is None else base.cuda().contiguous()
        return self._done(self.lib.gfv_slice_gw(a.data_ptr(), T.data_ptr(), self.L.ptr(add), self._i32(c["batch"]).data_ptr(),
                                                gw.data_ptr(), c["N"], 0 if base is None else 1, self.st), "slice_gw", gw)[0]

    def softmax_bwd(self, c, w, gw):
        x, Ws, bs, t, w, gw = self._up(c["xmid"], c["Ws"], c["bs"], c["temp"], w, gw)
        gx, sp = self._nan(c["N"], H * D), self._nan(self.lib.gfv_slice_softmax_bwd_blocks(c["N"]), 552)
        gx, sp = self._done(self.lib.gfv_slice_softmax_bwd(x.data_ptr(), Ws.data_ptr(), bs.data_ptr(), t.data_ptr(), w.data_ptr(),
                                                           gw.data_ptr(), gx.data_ptr(), sp.data_ptr(), c["N"], self.st),
                            "slice_softmax_bwd", gx, sp)
        return dict(self._partials(sp), gx=gx)

    def post_bwd(self, c, w):
        x, Ws, bs, t, w, gox, T1, fxm, T2, gn = self._up(c["xmid"], c["Ws"], c["bs"], c["temp"], w, c["gox"], c["T1"], c["fxm"], c["T2"],
                                                         c["gn"])
        gx, gfx = self._nan(c["N"], H * D), self._nan(c["N"], H * D)
        sp = self._nan(self.lib.gfv_slice_softmax_bwd_blocks(c["N"]), 552)
        gx, gfx, sp = self._done(self.lib.gfv_slice_post_bwd(x.data_ptr(), Ws.data_ptr(), bs.data_ptr(), t.data_ptr(), w.data_ptr(),
                                                             gox.data_ptr(), T1.data_ptr(), fxm.data_ptr(), T2.data_ptr(), gn.data_ptr(),
                                                             self._i32(c["batch"]).data_ptr(), gx.data_ptr(), gfx.data_ptr(), sp.data_ptr(),
                                                             c["N"], c["B"], self.st), "slice_post_bwd", gx, gfx, sp)
        return dict(self._partials(sp), gx=gx, gfx=gfx)

    def reduce_seg(self, rows, ptr):
        assert ptr[-1] == rows.shape[0]
        rows, = self._up(rows)
        out = self._nan(len(ptr) - 1, rows.shape[1])
        return self._done(self.lib.gfv_reduce_partials_seg(rows.data_ptr(), self._i32(ptr).data_ptr(), len(ptr) - 1, rows.shape[1],
                                                           out.data_ptr(), self.st), "reduce_partials_seg", out)[0]

    def attention_fwd(self, partial, ptr, W, hidden, keep):
        assert ptr[-1] <= partial.shape[0] and tuple(partial.shape[1:]) == (H * G, D + 1)
        B = len(ptr) - 1
        partial, Wq, Wk, Wv = self._up(partial, *W)
        token, norm, attn = (self._nan(B, H, G, D), self._nan(B, H, G), self._nan(B, H, G, G)) if keep else (None, None, None)
        out = self._nan(B, H, G, D)
        with self._hidden(hidden):
            res = self._done(self.lib.gfv_slice_attention_fwd(partial.data_ptr(), self._i32(ptr).data_ptr(), B, Wq.data_ptr(), Wk.data_ptr(),
                                                              Wv.data_ptr(), self.L.ptr(token), self.L.ptr(norm), self.L.ptr(attn),
                                                              out.data_ptr(), self.st), "slice_attention_fwd",
                             *((token, norm, attn, out) if keep else (out,)))
        return dict(zip(("token", "norm", "attn", "out_token") if keep else ("out_token",), res))

    def attention_bwd(self, gpartial, ptr, W, hidden, token, norm, attn):
        assert ptr[-1] <= gpartial.shape[0] and tuple(gpartial.shape[1:]) == (H * G, D + 1)
        B = len(ptr) - 1
        gpartial, Wq, Wk, Wv, token, norm, attn = self._up(gpartial, *W, token, norm, attn)
        g_raw, g_norm, dwp = self._nan(B, H, G, D), self._nan(B, H, G), self._nan(B * H, 3, D, D)
        with self._hidden(hidden):
            g_raw, g_norm, dwp = self._done(
                self.lib.gfv_slice_attention_bwd(gpartial.data_ptr(), self._i32(ptr).data_ptr(), B, Wq.data_ptr(), Wk.data_ptr(),
                                                 Wv.data_ptr(), token.data_ptr(), norm.data_ptr(), attn.data_ptr(), g_raw.data_ptr(),
                                                 g_norm.data_ptr(), dwp.data_ptr(), self.st), "slice_attention_bwd", g_raw, g_norm, dwp)
        return dict(g_raw=g_raw, g_norm=g_norm, dW=dwp.double().sum(0))
