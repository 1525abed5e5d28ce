"""The finite-volume section (csrc/fvm.hip) stage by stage in plain torch: from the decoder output `dec` through
10 tanh(dec / 10), the Dirichlet overwrite and the integrator's uv_hat to the WLSQ gradients, the face and cell values, the four
per-cell residual columns, their per-graph sums, the four losses and the two output fields - every tensor a kernel of that file
writes, in the kernel's own layout (phi [N,8], grad [N,16], Ff [E,16], phic [C,8], cres [C,4], gradc [C,16], sums / losses [B,4]).

The arithmetic is the oracle's (oracle/fvgn_oracle.py: integrator_conserved / integrator_non_conserved, which follow the dtype
of what they are handed); restated here is only what the oracle does not return: the per-cell outlet term lp2, the packing of Ff
with the face boundary-condition overwrite, cres, gradc, sums and the node field for the four values of `smooth`.  Evaluated in
float64 (`graph_tensors(graphs)`) it is the reference; evaluated in float32 (`graph_tensors(graphs, torch.float32)`) it is the
yardstick - what a correct float32 implementation leaves - from which the GPU tests take their tolerances (`tolerance`).  The
moments A, B1, Bx and every other mesh tensor enter as the kernels see them: rounded to float32, then cast.

`distinct_coefficients` gives every per-graph PDE coefficient its own value, so that a kernel reading a neighbouring entry of
theta_PDE / sigma / uvp_dim / dt_graph computes something else; `MISWIRED` are such mistakes made to the reference on purpose
(tests/test_fvm_float64_cpu.py holds each of them to be visible at 100 x the tolerance).

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import torch

from oracle import fvgn_oracle as O

MODES = ("explicit", "implicit", "imex")          # gfv_phi_fwd mode 0 / 1 / 2
FLOOR = 2.0 ** -22                                # tolerance floor: 4 float32 roundings of the column maximum
FACTOR = 4.0                                      # kernel tolerance = FACTOR x the float32 oracle's own error
ROW_STAGES = (("phi", "node_batch"), ("grad", "node_batch"), ("Ff", "edge_batch"), ("phic", "cell_batch"),
              ("cres", "cell_batch"), ("gradc", "cell_batch"), ("uvp_node", "node_batch"), ("uvp_cell", "cell_batch"),
              ("node_raw", "node_batch"), ("cell_raw", "cell_batch"), ("node_nosmooth", "node_batch"),
              ("node_nosmooth_raw", "node_batch"))
GRAPH_STAGES = ("sums", "losses")


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def distinct_coefficients(graphs, seed):
    """Clones of the five graph objects with every per-graph coefficient distinct: theta_PDE[:, 0:5] times factors in [0.5, 2]
    (per graph and per column), a non-zero source theta_PDE[:, 5], every entry of sigma and of uvp_dim distinct and non-zero,
    dt_graph distinct per graph.

    The source is +-20 times such a factor: with `draw_dec`'s fields on these meshes the momentum residual per unit area has a
    median of 20 ... 70 (tests/test_fvm_float64_cpu.py asserts the range), so `- src` is a visible part of it and not all of it."""
    out = tuple(g.clone() for g in graphs)
    gi = out[4]
    B = int(gi.theta_PDE.shape[0])
    g = torch.Generator().manual_seed(seed)

    def factors(rows, cols):
        # distinct by construction: a geometric ladder strictly inside (0.5, 2) - no rung is 1 - handed out in random order
        n = rows * cols
        lad = 0.5 * 4.0 ** ((torch.arange(n, dtype=torch.float64) + 0.25) / n)
        return lad[torch.randperm(n, generator=g)].reshape(rows, cols).to(torch.float32)

    theta = gi.theta_PDE.clone()
    theta[:, 0:5] = theta[:, 0:5] * factors(B, 5)
    sign = torch.tensor([1.0, -1.0]).repeat(B)[:B]
    theta[:, 5] = sign * 20.0 * factors(B, 1).reshape(-1)
    gi.theta_PDE = theta
    gi.sigma = factors(B, 3)
    gi.uvp_dim = gi.uvp_dim * factors(B, 3)
    gi.dt_graph = gi.dt_graph * factors(B, 1)
    return out


def draw_dec(N, seed):
    """Decoder output [N,3] float32: about 3 randn - tanh(dec / 10) neither linear nor saturated - with a few rows at +-60
    (saturated: 1 - tanh^2 = 2.5e-5) and at 0."""
    g = torch.Generator().manual_seed(seed)
    dec = 3.0 * torch.randn(N, 3, generator=g)
    rows = torch.randperm(N, generator=g)[:12]
    dec[rows[0:4]] = 60.0
    dec[rows[4:8]] = -60.0
    dec[rows[8:12]] = 0.0
    return dec


def uv_old_of(graphs):
    """The previous velocity as importer.py:168-170 forms it, in float32."""
    gn, gi = graphs[0], graphs[4]
    return (gn.x[:, 0:2] / gi.uvp_dim[gn.batch.reshape(-1), 0:2]).to(torch.float32).contiguous()


def graph_tensors(graphs, dtype=torch.float64):
    """oracle.graph_tensors with every floating tensor rounded to float32 (what the plan hands the kernels), then cast."""
    G = O.graph_tensors(*graphs)
    for k, v in G.items():
        if torch.is_tensor(v):
            G[k] = v.to(torch.float32).to(dtype) if v.is_floating_point() else v.reshape(-1) if k.endswith("_batch") else v
    G["node_type"] = G["node_type"].reshape(-1)
    G["face_type"] = G["face_type"].reshape(-1)
    G["y"] = G["y"][:, 0:2]
    return G


def has_outflow(G):
    """[B] bool: the graph has an OUTFLOW face, i.e. its pressure-outlet loss depends on the fields at all."""
    out = torch.zeros(G["num_graphs"], dtype=torch.bool)
    out[G["edge_batch"][G["face_type"] == O.OUTFLOW]] = True
    return out


# ---- wiring mistakes, made to the reference's coefficients on purpose --------------------------------------------------------------
def _swap(t, i, j):
    t = t.clone()
    t[:, [i, j]] = t[:, [j, i]]
    return t


def _copy_col(t, dst, src):
    t = t.clone()
    t[:, dst] = t[:, src]
    return t


def _zero_col(t, j):
    t = t.clone()
    t[:, j] = 0
    return t


MISWIRED = {
    "th2<->th3": lambda G: dict(G, theta_PDE=_swap(G["theta_PDE"], 2, 3)),
    "sigma[0]<->sigma[1]": lambda G: dict(G, sigma=_swap(G["sigma"], 0, 1)),
    "theta[1]->theta[0]": lambda G: dict(G, theta_PDE=_copy_col(G["theta_PDE"], 1, 0)),
    "source dropped": lambda G: dict(G, theta_PDE=_zero_col(G["theta_PDE"], 5)),
    "dt of graph 0 for all": lambda G: dict(G, dt_graph=G["dt_graph"][0:1].expand_as(G["dt_graph"]).clone()),
    "uvp_dim columns swapped": lambda G: dict(G, uvp_dim=_swap(G["uvp_dim"], 0, 2)),
}


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def phi_stage(dec, y, node_type, uv_old, integrator):
    """importer.py:187-201 -> phi [N,8] = (uvp_new, uv_hat, uv_old, 0)."""
    uvp = O.enforce_boundary_condition(torch.tanh(dec / 10) * 10, node_type, y)
    if integrator == "explicit":
        uv_hat = uv_old
    elif integrator == "implicit":
        uv_hat = uvp[:, 0:2]
    else:
        uv_hat = (uv_old + uvp[:, 0:2]) / 2.0
    return torch.cat((uvp, uv_hat, uv_old, torch.zeros_like(uvp[:, 0:1])), dim=1)


def _pad(t, width):
    return torch.cat((t, t.new_zeros(t.shape[0], width - t.shape[1])), dim=1)


def stages(dec, uv_old, G, conserved=True, integrator="imex", order="2nd"):
    """Every tensor of the section, in the dtype of `dec` / `G` (differentiable with respect to `dec`)."""
    nb, cb = G["node_batch"], G["cell_batch"]
    B, C = G["num_graphs"], G["centroid"].shape[0]
    phi = phi_stage(dec, G["y"], G["node_type"], uv_old, integrator)
    uvp, uv_hat = phi[:, 0:3], phi[:, 3:5]
    integ = O.integrator_conserved if conserved else O.integrator_non_conserved
    res, inter = integ(uvp, uv_hat, uv_old, G, dict(order=order, ncn_smooth=True), return_intermediates=True)
    lc, lmx, lmy, lp, smoothed, _ = res
    grad, phi_cell = inter["grad"], inter["phi_cell"]                                    # [N,7,2], [C,7]
    ei, ftype = G["edge_index"], G["face_type"]
    phi_face = inter["phi_face"] if conserved else O.node_to_face_2nd_order(phi[:, 0:5], grad[:, 0:5], ei, G["pos"], G["face_pos"])
    grad_face = inter["grad_face"] if conserved else O.node_to_face_2nd_order(grad[:, 0:5], None, ei, G["pos"], G["face_pos"])
    # Ff = [phi_f[0:5] | grad_f at 5 + 2c + a | 0], the velocities with the face boundary condition (FVscheme.py:32-48)
    y_face = (G["y"][ei[0]] + G["y"][ei[1]]) / 2.0
    Ff = torch.cat((O.fix_face_flux_bc(phi_face[:, 0:2], ftype, y_face), phi_face[:, 2:3],
                    O.fix_face_flux_bc(phi_face[:, 3:5], ftype, y_face), grad_face.reshape(-1, 10),
                    torch.zeros_like(phi_face[:, 0:1])), dim=1)
    # the pressure-outlet term per cell (FVscheme.py:145-167 sums it per graph at once)
    cf, ci = G["cells_face"], G["cells_index"]
    Svec = G["cells_face_unv"].view(-1, 2) * G["face_area"].view(-1, 1)[cf]
    diff_c = G["theta_PDE"][cb][:, 4:5]
    visc = diff_c[ci] * torch.matmul(grad_face[cf, 0:2], Svec.unsqueeze(2)).squeeze(2)
    lvec = (visc - phi_face[cf, 2:3] * Svec) * (ftype[cf] == O.OUTFLOW).unsqueeze(1).to(Svec.dtype)
    lp2 = O.scatter_add((lvec ** 2).sum(-1), ci, C)
    cres = torch.cat((inter["div"].view(-1, 1), inter["mom"], lp2.view(-1, 1)), dim=1)
    sums = O.scatter_add(torch.cat((cres[:, 0:3] ** 2, cres[:, 3:4]), dim=1), cb, B)
    st = dict(phi=phi, grad=_pad(grad.reshape(-1, 14), 16), Ff=Ff, phic=_pad(phi_cell, 8), cres=cres, sums=sums,
              losses=torch.cat((lc, lmx, lmy, lp), dim=1))
    if not conserved:
        st["gradc"] = _pad(inter["grad_cell"].reshape(-1, 10), 16)
    # the two fields: smooth bit 0 = cell -> node smoothing, bit 1 = raw (no Dirichlet overwrite, not re-dimensionalised)
    dim_n, dim_c = G["uvp_dim"][nb] * G["sigma"][nb], G["uvp_dim"][cb] * G["sigma"][cb]
    finish = lambda f: O.enforce_boundary_condition(f, G["node_type"], G["y"]) * dim_n           # importer.py:223-231
    st["uvp_node"], st["node_raw"] = finish(smoothed), smoothed
    st["node_nosmooth"], st["node_nosmooth_raw"] = finish(uvp), uvp
    st["uvp_cell"], st["cell_raw"] = phi_cell[:, 0:3] * dim_c, phi_cell[:, 0:3]
    return st


def detached(st):
    return {k: v.detach() for k, v in st.items()}


def one_hot_gradients(dec, uv_old, G, conserved=True, integrator="imex", order="2nd"):
    """{(b, l): d losses[b, l] / d dec [N,3]} by autograd, each loss of each graph on its own; the pairs whose loss does not
    depend on dec - the pressure-outlet loss of a graph without an OUTFLOW face - are left out."""
    dec = dec.detach().clone().requires_grad_(True)
    losses = stages(dec, uv_old, G, conserved, integrator, order)["losses"]
    outflow = has_outflow(G)
    grads = {}
    for b in range(G["num_graphs"]):
        for l in range(4):
            if l == 3 and not bool(outflow[b]):
                continue
            grads[(b, l)] = torch.autograd.grad(losses[b, l], dec, retain_graph=True)[0]
    return grads


# ---- comparison: per column, per graph ---------------------------------------------------------------------------------------
def col_err(got, ref):
    """max |got - ref| / max |ref| per column; a column whose reference is all zero must be exactly zero (else inf)."""
    d = (got.double() - ref.double()).abs().amax(0)
    s = ref.double().abs().amax(0)
    return torch.where(s > 0, d / s.clamp(min=1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))


def column_errors(got, ref, G, names=None):
    """{stage: [B, columns]} - every column of every stage normalised by that column's reference maximum over the rows of one
    graph; `sums` and `losses` element by element."""
    out = {}
    for name, rows in ROW_STAGES:
        if name not in got or name not in ref or (names is not None and name not in names):
            continue
        assert got[name].shape == ref[name].shape, (name, got[name].shape, ref[name].shape)
        out[name] = torch.stack([col_err(got[name][G[rows] == b], ref[name][G[rows] == b]) for b in range(G["num_graphs"])])
    for name in GRAPH_STAGES:
        if name in got and name in ref and (names is None or name in names):
            out[name] = torch.stack([col_err(got[name][b:b + 1], ref[name][b:b + 1]) for b in range(G["num_graphs"])])
    return out


def gradient_errors(got, ref, G):
    """{(b, l): [3]} - a one-hot gradient per channel over the rows of graph b; rows of the other graphs must be exactly 0."""
    out = {}
    for (b, l), r in ref.items():
        m = G["node_batch"] == b
        e = col_err(got[(b, l)][m], r[m])
        if bool((got[(b, l)][~m] != 0).any()):
            e = torch.full_like(e, float("inf"))
        out[(b, l)] = e
    return out


def tolerance(yard):
    """The kernels' tolerance from the float32 oracle's own error: FACTOR x that, at least FLOOR."""
    return {k: (FACTOR * v).clamp(min=FLOOR) for k, v in yard.items()}


def failures(err, tol):
    """[(stage, graph, column, error, tolerance)] of the columns over their tolerance."""
    bad = []
    for k, e in err.items():
        t = tol[k]
        for idx in torch.nonzero(~(e <= t)).tolist():
            bad.append((k, *idx, float(e[tuple(idx)]), float(t[tuple(idx)])))
    return bad


def family_max(err):
    """{stage: largest finite column error} for the docstrings."""
    return {str(k): float(v[torch.isfinite(v)].max()) if bool(torch.isfinite(v).any()) else 0.0 for k, v in err.items()}


# ---- per-graph norms, exactly ----------------------------------------------------------------------------------------------------
def graph_norms(cres, gcell_ptr, theta, sigma):
    """float64 sums [B,4] and losses [B,4] of float32 cres [C,4] (FVscheme.py:158-164,184-188,243-250)."""
    c = cres.double()
    sq = torch.cat((c[:, 0:3] ** 2, c[:, 3:4]), dim=1)
    B = gcell_ptr.numel() - 1
    sums = torch.stack([sq[int(gcell_ptr[b]):int(gcell_ptr[b + 1])].sum(0) for b in range(B)])
    coef = torch.stack((theta.double()[:, 1], sigma.double()[:, 0], sigma.double()[:, 1], torch.ones(B, dtype=torch.float64)), dim=1)
    return sums, sums.sqrt() * coef
