"""Device-resident state pool.

The reference keeps its meshes and current fields in a CPU ``Data_Pool`` and, every training step, batches five PyG views on
the host and copies them to the device (Load_mesh/Graph_loader.py:131-152,405-480,830-1006; pre_train_Adam.py:150-156),
then copies the prediction back (``payback``, Graph_loader.py:370-396).  Here every mesh lives in HBM together with its
own ``MeshPlan`` (CSR tables, permuted WLSQ moments: built ONCE per mesh); a batch of any meshes of the pool is assembled
on the device by ONE launch of ``gfv_concat_offsets`` - a batch is block diagonal, so every batched plan tensor is the
concatenation of the per-mesh tensors with the node / face / cell / incidence offset of the mesh added to its indices
(the ``__inc__`` rules of ``CustomGraphData``) - and predictions are written back in place.  The assembled plan is
tensor-for-tensor equal to ``build_plan(build_batch(meshes))`` (tests/test_pool_gpu.py).

For training over the pool with a new batch every step there is ``DevicePool.arena`` -> ``BatchArena``: the same batch, assembled
into FIXED memory by one launch of ``gfv_pool_assemble`` with no per-step allocation or host-built table (what
``gfv.pool_trainer.PoolTrainStep`` replays recorded steps over), and ``DevicePool.add_variant``: entries that share a topology.
``DevicePool.renew`` re-draws the boundary conditions of many entries by one launch (``gfv_pool_renew``; the reference's renewal
schedule around it: ``gfv.renew.PoolRenewal``); ``reset_env`` is the same for one entry with torch ops.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from .graph import Data, build_batch
from .plan import MeshPlan, SLICE_CHUNK, build_plan

# attribute -> (offset kind); offsets: n node, e face, e2 2*face, c cell, k incidence, s stencil entry, - none
_INT_ATTRS = dict(es="n", er="n", n_col_node="n", x_out="n", xo_in="n", knode="n", s_col="e", r_col="e", kface="e",
                  n_col_edge2="e2", kcell="c", ncell="c", fk="k", node_type="-", ftype="-")
# rowptr attribute -> (row count kind, nnz offset kind)
_ROWPTRS = dict(n_rowptr=("n", "e2"), s_rowptr=("n", "e"), r_rowptr=("n", "e"), x_rowptr=("n", "s"),
                xo_rowptr=("n", "s"), crow=("c", "k"), frow=("e", "k"), nrow=("n", "k"))
_FLOAT_ATTRS = ("inv_deg", "y", "pos", "x_B", "xo_B", "sumB", "rn", "An", "fpos", "kS", "centroid", "area", "theta", "sigma",
                "uvp_dim", "dt")
_FILL = dict(batch="n", cbatch="c")   # graph id per node / cell

_DESC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("kind", "<i4"), ("add", "<i4")])

_VARIANT_OWNED = ("y", "theta", "dt", "uvp_dim")      # (+ x and the bc record): what reset_env writes
_SIZE_KEYS = ("n", "e", "c", "k", "s", "nchunk")      # the head columns of the source table (include/gfv.h gfv_pool_args_t)
_KIND_ID = {"-": 0, "n": 1, "e": 2, "e2": 3, "c": 4, "k": 5, "s": 6}
# rows of every copied attribute in units of a size ("g": one row per graph); checked against every entry when an arena is built
_ROWS_OF = dict(es="e", er="e", n_col_node="e2", x_out="s", xo_in="s", knode="k", s_col="e", r_col="e", kface="k", n_col_edge2="e2",
                kcell="k", ncell="k", fk="k", node_type="n", ftype="e", inv_deg="n", y="n", pos="n", x_B="s", xo_B="s", sumB="n",
                rn="n", An="n", fpos="e", kS="k", centroid="c", area="c", theta="g", sigma="g", uvp_dim="g", dt="g", x="n", x_raw="n")


def entry_signature(size):
    """(nodes, faces, cells, incidences, stencil entries, slice chunks) of one pool entry."""
    return tuple(int(size[k]) for k in _SIZE_KEYS)


def batch_signature(sizes, indices):
    """The ordered size signature of a batch: two batches with the same signature are assembled into the same memory with the
    same shapes, so the launches of a step over one are the launches of a step over the other."""
    return tuple(entry_signature(sizes[int(i)]) for i in indices)


def batch_totals(sizes, indices):
    return {k: sum(int(sizes[int(i)][k]) for i in indices) for k in _SIZE_KEYS}


def default_capacity(sizes, max_graphs):
    """Totals no batch of up to `max_graphs` entries exceeds: per size, the sum of its `max_graphs` largest values."""
    if int(max_graphs) < 1:
        raise ValueError("max_graphs must be at least 1")
    return {k: sum(sorted((int(s[k]) for s in sizes), reverse=True)[:int(max_graphs)]) for k in _SIZE_KEYS}


def check_fits(totals, B, capacity, max_graphs):
    """ValueError when a batch of B entries with these totals does not fit an arena of this capacity."""
    if B < 1:
        raise ValueError("a batch needs at least one entry")
    if B > max_graphs:
        raise ValueError(f"a batch of {B} entries exceeds the arena's capacity of {max_graphs} graphs")
    for k in _SIZE_KEYS:
        if totals[k] > capacity[k]:
            raise ValueError(f"the batch needs {totals[k]} of '{k}', the arena holds {capacity[k]}: build it with larger max_sizes")


def _rows(size, kind, B=1):
    return B if kind == "g" else (2 * size["e"] if kind == "e2" else size[kind])


class BatchArena:
    """Fixed memory every batch of a DevicePool is assembled into (include/gfv.h gfv_pool_assemble: ONE launch, the entry indices
    by value, offsets formed on the device).  `load(indices)` returns views of that memory: for batches of equal size signature
    every tensor has the same `data_ptr()` and shape as last time - a recorded launch list of a step over one such batch is valid
    for every other (gfv/pool_trainer.py).  A later load overwrites what an earlier one returned."""

    VIEW_CACHE = 256

    def __init__(self, pool, max_graphs, max_sizes=None):
        self.pool = pool
        self.max_graphs = int(max_graphs)
        if not 1 <= self.max_graphs <= L.POOL_MAX_GRAPHS:
            raise ValueError(f"max_graphs must be in [1, {L.POOL_MAX_GRAPHS}]")
        cap = default_capacity(pool.sizes, self.max_graphs) if max_sizes is None else {k: int(max_sizes[k]) for k in _SIZE_KEYS}
        self.capacity = cap
        dev = pool.device
        B = self.max_graphs
        # attributes of the launch, in table order: (name, mode, offset kind, rows kind, words per row, dtype)
        attrs = []
        for a, k in _INT_ATTRS.items():
            attrs.append((a, L.POOL_COPY if k == "-" else L.POOL_ADD, k))
        for a, (_, nnz) in _ROWPTRS.items():
            attrs.append((a, L.POOL_ROWPTR, nnz))
        for a in _FLOAT_ATTRS + ("x", "x_raw"):
            attrs.append((a, L.POOL_COPY, "-"))
        for a, k in _FILL.items():
            attrs.append((a, L.POOL_FILL, "-"))
        self.attrs = attrs
        self.names = [a[0] for a in attrs]
        A = len(attrs)
        assert A <= L.POOL_MAX_ATTRS
        self._buf, self._row_shape = {}, {}
        args = L.PoolArgs()
        for j, (a, mode, k) in enumerate(attrs):
            if mode == L.POOL_FILL:
                rows, row_shape, dtype = cap[_FILL[a]], (), torch.int32
            elif mode == L.POOL_ROWPTR:
                rows, row_shape, dtype = cap[_ROWPTRS[a][0]] + 1, (), torch.int32
            else:
                _, _, row_shape, dtype = pool._src["x" if a == "x_raw" else a]
                rows = _rows(cap, _ROWS_OF[a], B)
            roww = int(np.prod(row_shape)) if row_shape else 1
            words = rows * roww
            buf = torch.zeros(max(words, 4), dtype=dtype, device=dev)
            assert buf.data_ptr() % 16 == 0
            self._buf[a], self._row_shape[a] = buf, tuple(row_shape)
            args.attr_info[j] = mode | (_KIND_ID[k] << 4)
            args.dst[j] = buf.data_ptr()
            args.dst_cap_words[j] = words
        small = dict(gnode_ptr=B + 1, gcell_ptr=B + 1, gchunk_ptr=B + 1, gunit_ptr=B + 1, chunk_beg=cap["nchunk"], chunk_end=cap["nchunk"])
        for j, (a, words) in enumerate(small.items()):
            self._buf[a] = torch.zeros(max(words, 1), dtype=torch.int32, device=dev)
            args.small[j] = self._buf[a].data_ptr()
        args.n_attrs, args.max_graphs, args.slice_chunk, args.max_chunks = A, B, SLICE_CHUNK, cap["nchunk"]
        self._args = args
        self.x_attr = self.names.index("x")
        self._views = {}
        self._n_tab = -1
        self._last = None
        self._build_table()

    # the source table: one row per entry, on the host (argument checks, grid sizes) and on the device (the kernels) -----------------
    def _build_table(self):
        pool, A = self.pool, len(self.attrs)
        tab = np.zeros((pool.n, L.POOL_ROW_HEAD + 2 * A), dtype=np.int64)
        for c, k in enumerate(_SIZE_KEYS):
            tab[:, c] = [s[k] for s in pool.sizes]
        for j, (a, mode, k) in enumerate(self.attrs):
            if mode == L.POOL_FILL:
                tab[:, L.POOL_ROW_HEAD + A + j] = [s[_FILL[a]] for s in pool.sizes]
                continue
            ptrs, words, row_shape, _ = pool._src["x" if a == "x_raw" else a]
            tab[:, L.POOL_ROW_HEAD + j] = ptrs.astype(np.int64)
            tab[:, L.POOL_ROW_HEAD + A + j] = words
            roww = int(np.prod(row_shape)) if row_shape else 1
            want = [(_rows(s, _ROWPTRS[a][0]) + 1) if mode == L.POOL_ROWPTR else _rows(s, _ROWS_OF[a]) * roww for s in pool.sizes]
            if list(words) != want:
                raise ValueError(f"pool attribute '{a}' does not have the rows its size kind says")
        self._tab = np.ascontiguousarray(tab)
        info = (C.c_int32 * A)(*[self._args.attr_info[j] for j in range(A)])
        rc = L.load(raw=True).gfv_pool_table_check(self._tab.ctypes.data, pool.n, A, C.addressof(info))
        if rc != 0:
            raise ValueError("the pool's source table is not valid (gfv_pool_table_check)")
        self._tab_dev = torch.from_numpy(self._tab).to(pool.device)
        self._args.table_host, self._args.table_dev = self._tab.ctypes.data, self._tab_dev.data_ptr()
        self._args.n_entries = pool.n
        self._entry_sig = [entry_signature(s) for s in pool.sizes]
        self._n_tab = pool.n

    def signature(self, indices):
        return batch_signature(self.pool.sizes, indices)

    def _make_views(self, idx):
        pool, B = self.pool, len(idx)
        tot = batch_totals(pool.sizes, idx)
        check_fits(tot, B, self.capacity, self.max_graphs)
        p = MeshPlan()
        out = {}
        for a, mode, k in self.attrs:
            if mode == L.POOL_FILL:
                words = tot[_FILL[a]]
            elif mode == L.POOL_ROWPTR:
                words = tot[_ROWPTRS[a][0]] + 1
            else:
                rs = self._row_shape[a]
                words = _rows(tot, _ROWS_OF[a], B) * (int(np.prod(rs)) if rs else 1)
            t = self._buf[a][:words]
            rs = self._row_shape[a]
            out[a] = t.view((-1,) + rs) if rs else t
            if a not in ("x", "x_raw"):
                setattr(p, a, out[a])
        for a, words in (("gnode_ptr", B + 1), ("gcell_ptr", B + 1), ("gchunk_ptr", B + 1), ("gunit_ptr", B + 1),
                         ("chunk_beg", tot["nchunk"]), ("chunk_end", tot["nchunk"])):
            setattr(p, a, self._buf[a][:words])
        p.N, p.E, p.C, p.B = tot["n"], tot["e"], tot["c"], B
        p.S, p.Sg, p.n_chunks, p.device = tot["s"], tot["k"], tot["nchunk"], pool.device
        p.M = pool.plans[idx[0]].M
        graph_node = Data(x=out["x"], batch=p.batch, pos=p.pos, num_graphs=B, norm_uvp=True, norm_global=True)
        graph_node._gfv_pool_plan = p
        graph_node._gfv_x_raw = out["x_raw"]       # the un-normalised rows (what TrainStep clones into its backup, kept by the arena)
        graphs = (graph_node, Data(num_graphs=B), Data(num_graphs=B), Data(num_graphs=B),
                  Data(theta_PDE=p.theta, sigma=p.sigma, uvp_dim=p.uvp_dim, dt_graph=p.dt.view(-1, 1), num_graphs=B))
        return graphs, p

    def load(self, indices):
        """-> (graphs, plan) of the batch `indices`, assembled into the arena by one launch on the current stream."""
        idx = [int(i) for i in indices]
        pool = self.pool
        if pool.n != self._n_tab:
            self._build_table()                    # (entries were added: add_variant)
        for i in idx:
            if not 0 <= i < pool.n:
                raise ValueError(f"pool entry {i} does not exist (the pool holds {pool.n})")
        sig = tuple(self._entry_sig[i] for i in idx)
        hit = self._views.get(sig)
        if hit is None:
            hit = self._make_views(idx)            # (raises ValueError for a batch beyond the capacity)
            if len(self._views) >= BatchArena.VIEW_CACHE:
                self._views.pop(next(iter(self._views)))
            self._views[sig] = hit
        args = self._args
        args.B = len(idx)
        for b, i in enumerate(idx):
            args.idx[b] = i
        rc = L.load().gfv_pool_assemble(C.byref(args), L.stream_ptr())
        if rc == -1:
            raise ValueError("gfv_pool_assemble refused the batch (it does not fit the arena, or an index is outside the pool)")
        L.check(rc, "gfv_pool_assemble")
        self._last = (idx, sig)
        return hit

    def x_raw(self, graphs):
        return graphs[0]._gfv_x_raw

    def payback(self, indices, uvp_node, advance=False):
        """Write the batch's predicted (u, v, p) [N, 3] back into the pool entries' own `x` (DevicePool.payback as ONE launch; an
        entry that appears twice takes its later occurrence); advance: also into the arena's un-normalised state, which the next
        inner step over the same batch then starts from (TrainStep.advance_time)."""
        idx = [int(i) for i in indices]
        if self.pool.n != self._n_tab:
            self._build_table()
        assert uvp_node.dtype == torch.float32 and uvp_node.is_contiguous() and uvp_node.shape[1] == 3
        ia = (C.c_int32 * len(idx))(*idx)
        raw = self._buf["x_raw"].data_ptr() if advance else None
        rc = L.load().gfv_pool_payback(self._tab.ctypes.data, self._tab_dev.data_ptr(), self.pool.n, len(self.attrs), self.x_attr,
                                       C.addressof(ia), len(idx), uvp_node.data_ptr(), int(uvp_node.shape[0]), raw, L.stream_ptr())
        if rc == -1:
            raise ValueError("gfv_pool_payback refused the batch (index outside the pool, or uvp_node is not the batch's node field)")
        L.check(rc, "gfv_pool_payback")


class DevicePool:
    def __init__(self, meshes, fields=None, device="cuda"):
        self.device = torch.device(device)
        self.n = len(meshes)
        self.plans, self.x, self.sizes = [], [], []
        self.bc = [dict(m["bc"]) if "bc" in m else None for m in meshes]       # sampled PDE parameters per mesh
        self.pos64 = [torch.from_numpy(np.ascontiguousarray(m["node|pos"])).to(self.device) for m in meshes]
        for i, m in enumerate(meshes):
            g = build_batch([m], None if fields is None else [fields[i]], device=self.device)
            p = build_plan(*g)
            self.plans.append(p)
            self.x.append(g[0].x.contiguous())          # [N, 3 + 9]: (u, v, p) state + theta_PDE (datapreprocessing)
            self.sizes.append(dict(n=p.N, e=p.E, e2=2 * p.E, c=p.C, k=p.Sg, s=p.S, nchunk=p.n_chunks))
        self._src = {}   # attr -> (ptr per mesh, words per mesh, words per row)
        for a in list(_INT_ATTRS) + list(_ROWPTRS) + list(_FLOAT_ATTRS):
            ts = [getattr(p, a) for p in self.plans]
            assert all(t.is_contiguous() and t.element_size() == 4 for t in ts), a
            self._src[a] = (np.array([t.data_ptr() for t in ts], dtype=np.uint64),
                            np.array([t.numel() for t in ts], dtype=np.int64), tuple(ts[0].shape[1:]), ts[0].dtype)
        self._src["x"] = (np.array([t.data_ptr() for t in self.x], dtype=np.uint64),
                          np.array([t.numel() for t in self.x], dtype=np.int64), tuple(self.x[0].shape[1:]), torch.float32)
        # renew: min / max of pos[:, 1] over all nodes and over the inlet nodes, one row per topology (a variant shares the
        # positions of its parent, and with them the row), reduced on the first renewal that touches the topology
        self._yrange = torch.empty((max(self.n, 1), 4), dtype=torch.float64, device=self.device)
        self._yrange_row = {}

    # ------------------------------------------------------------------------------------------------------------
    def batch(self, indices):
        """-> (graphs, plan): the five graph objects (carrying what the HIP model reads: ``graph_node.x`` and the plan)
        for the meshes `indices` of the pool, assembled on the device."""
        idx = [int(i) for i in indices]
        B = len(idx)
        sz = [self.sizes[i] for i in idx]
        off = {k: np.concatenate(([0], np.cumsum([s[k] for s in sz]))).astype(np.int64) for k in ("n", "e", "e2", "c", "k", "s")}
        off["-"] = np.zeros(B + 1, dtype=np.int64)
        dev = self.device
        descs = []
        out = {}

        def alloc(a, words, dtype, row_shape):
            t = torch.empty((words,), dtype=dtype, device=dev)
            out[a] = t.view((-1,) + row_shape) if row_shape else t
            return t.data_ptr()

        def add_pieces(a, kind, adds, extra_last=0):
            ptrs, words, row_shape, dtype = self._src[a]
            w = words[idx].copy()
            if extra_last:                     # rowptr: n_i entries per mesh, n_last + 1 for the last one
                w -= 1
                w[-1] += 1
            base = alloc(a, int(w.sum()), dtype, row_shape)
            starts = np.concatenate(([0], np.cumsum(w)[:-1]))
            d = np.zeros(B, dtype=_DESC)
            d["src"], d["dst"], d["n"], d["kind"], d["add"] = ptrs[idx], base + 4 * starts.astype(np.uint64), w, kind, adds
            descs.append(d)

        for a, k in _INT_ATTRS.items():
            add_pieces(a, 0 if k == "-" else 1, off[k][:B])
        for a, (_, nnz) in _ROWPTRS.items():
            add_pieces(a, 1, off[nnz][:B], extra_last=1)
        for a in _FLOAT_ATTRS:
            add_pieces(a, 0, 0)
        add_pieces("x", 0, 0)
        for a, k in _FILL.items():
            counts = np.array([s[k] for s in sz], dtype=np.int64)
            base = alloc(a, int(counts.sum()), torch.int32, ())
            d = np.zeros(B, dtype=_DESC)
            d["dst"], d["n"], d["kind"], d["add"] = base + 4 * off[k][:B].astype(np.uint64), counts, 2, np.arange(B)
            descs.append(d)
        # small per-graph pointer arrays and the slice-token chunks: computed on the host, one upload
        chunk_beg, chunk_end, gcp = [], [], [0]
        for b in range(B):
            n0, n1 = int(off["n"][b]), int(off["n"][b + 1])
            st = np.arange(n0, n1, SLICE_CHUNK)
            chunk_beg.append(st)
            chunk_end.append(np.minimum(st + SLICE_CHUNK, n1))
            gcp.append(gcp[-1] + len(st))
        small = dict(gnode_ptr=off["n"], gcell_ptr=off["c"], gchunk_ptr=np.array(gcp), gunit_ptr=np.arange(B + 1),
                     chunk_beg=np.concatenate(chunk_beg), chunk_end=np.concatenate(chunk_end))
        blob = np.concatenate([np.concatenate(descs).view(np.int32)] + [v.astype(np.int32) for v in small.values()])
        dblob = torch.from_numpy(blob).to(dev, non_blocking=True)
        ndesc = sum(len(d) for d in descs)
        L.check(L.load().gfv_concat_offsets(dblob.data_ptr(), ndesc, 48, L.stream_ptr()), "gfv_concat_offsets")

        p = MeshPlan()
        for a, t in out.items():
            if a != "x":
                setattr(p, a, t)
        pos = ndesc * (_DESC.itemsize // 4)
        for a, v in small.items():
            setattr(p, a, dblob[pos:pos + len(v)])
            pos += len(v)
        p.N, p.E, p.C, p.B = int(off["n"][B]), int(off["e"][B]), int(off["c"][B]), B
        p.S, p.Sg, p.n_chunks, p.device = int(off["s"][B]), int(off["k"][B]), gcp[-1], dev
        p.M = self.plans[idx[0]].M                         # WLSQ Taylor terms (all meshes of a pool share the order)
        p._keep = dblob                                    # the small arrays are views of the upload buffer
        graph_node = Data(x=out["x"], batch=p.batch, pos=p.pos, num_graphs=B, norm_uvp=True, norm_global=True)
        graph_node._gfv_pool_plan = p
        graphs = (graph_node, Data(num_graphs=B), Data(num_graphs=B), Data(num_graphs=B),
                  Data(theta_PDE=p.theta, sigma=p.sigma, uvp_dim=p.uvp_dim, dt_graph=p.dt.view(-1, 1), num_graphs=B))
        self._last = (idx, off["n"])
        return graphs, p

    # ------------------------------------------------------------------------------------------------------------
    def reset_env(self, i, **sampled):
        """Re-select the boundary condition of mesh `i` and restart its field, in place on the device
        (Data_Pool.reset_env -> CFDdatasetBase.transform_mesh, Graph_loader.py:154-229, Load_mesh.py:82-130,134-246,
        524-565).  `sampled`: any of U, rho, mu, source, aoa, dt, L - the values the reference draws from the ranges of
        BC.json (select_PDE_coef; the draw itself stays with the caller).  Geometry, stencil and moment matrices do not
        depend on them and stay as they are (the reference rebuilds identical copies); what changes is theta_PDE, dt, the
        dimensional scales, the Dirichlet targets and the initial field: 31 scalars from the host, the per-node part
        (inlet velocity profile -> target, initial state) with torch ops on the device."""
        from . import meshgen
        if self.bc[i] is None:
            raise ValueError("the mesh was given without its 'bc' record (gfv.meshgen.finish_mesh keeps it)")
        bc = self.bc[i]
        bc.update({k: float(v) for k, v in sampled.items()})
        theta, dt_graph, uvp_dim = meshgen.pde_coefficients(bc)
        p, dev = self.plans[i], self.device
        small = torch.from_numpy(np.concatenate((theta.reshape(-1), dt_graph.reshape(-1), uvp_dim.reshape(-1)))).to(dev)
        p.theta.copy_(small[0:9].view(1, 9))
        p.dt.copy_(small[9:10])
        p.uvp_dim.copy_(small[10:13].view(1, 3))
        U = float(bc["U"])
        pos, nt = self.pos64[i], p.node_type
        inlet = (nt == meshgen.INFLOW) | (nt == meshgen.IN_WALL) | (nt == meshgen.PRESS_POINT)

        def profile(pp):   # gfv.meshgen.velocity_profile in float64
            u = torch.zeros(pp.shape[0], dtype=torch.float64, device=dev)
            if pp.shape[0] == 0:
                return u
            if bc["inlet_type"] == "parabolic":
                yy = pp[:, 1] - pp[:, 1].min()
                ymax, ymin = yy.max(), yy.min()
                u = 6 * U * yy * (((ymax - ymin) - yy) / (ymax - ymin) ** 2)
            elif bc["inlet_type"] == "uniform":
                u = u + U
            else:
                raise ValueError(bc["inlet_type"])
            return u

        u = profile(pos).to(torch.float32)
        u[inlet] = profile(pos[inlet]).to(torch.float32)
        u = torch.where(nt == meshgen.WALL, torch.zeros_like(u), u)
        u = torch.where(nt == meshgen.IN_WALL, u / 2.0, u)
        x = self.x[i]
        x[:, 0] = u
        x[:, 1:3] = 0.0
        x[:, 3:12] = p.theta
        p.y[:, 0] = u / np.float32(U)
        p.y[:, 1] = 0.0

    # ------------------------------------------------------------------------------------------------------------
    def _yrange_ptr(self, i):
        """Device address of entry i's row of the y-range table [min, max of pos[:, 1] over all nodes | over the inlet nodes];
        the row is reduced when its topology is first asked for (reductions that do not synchronise; no inlet node: +inf, -inf)."""
        from . import meshgen
        key = self.pos64[i].data_ptr()
        r = self._yrange_row.get(key)
        if r is None:
            r = len(self._yrange_row)
            y, nt = self.pos64[i][:, 1], self.plans[i].node_type
            other = ~((nt == meshgen.INFLOW) | (nt == meshgen.IN_WALL) | (nt == meshgen.PRESS_POINT))
            self._yrange[r].copy_(torch.stack((y.amin(), y.amax(), y.masked_fill(other, float("inf")).amin(),
                                               y.masked_fill(other, float("-inf")).amax())))
            self._yrange_row[key] = r
        return self._yrange.data_ptr() + 32 * r

    @staticmethod
    def _renew_kind(v, what):
        if v is not None and not isinstance(v, str):
            raise ValueError(f"{what}: the list-valued form ([u, v, p]) is not implemented (nor is it by the reference's velocity_profile)")
        if v not in L.RENEW_KINDS:
            if v.lower().endswith((".vtu", ".h5")):
                raise ValueError(f"{what}: the file-valued form ('{v}') is not implemented (nor is it by the reference's velocity_profile)")
            raise ValueError(f"{what}: unknown profile kind '{v}' (known: {[k for k in L.RENEW_KINDS if k]} and None)")
        return L.RENEW_KINDS[v]

    def renew(self, indices, sampled):
        """`reset_env` for many entries at once: ONE launch of gfv_pool_renew per POOL_MAX_GRAPHS entries, no host synchronisation,
        nothing uploaded (the records - pointers, the 13 coefficients, U, the angle - travel in the launch's arguments).
        sampled: one dict per index with the keys of `reset_env` (U, rho, mu, source, aoa, dt, L) and optionally `inlet_type` /
        `init_field_type`: a profile kind of the reference's velocity_profile (Set_BC.py:33-64: "parabolic", "uniform",
        "uniform_aoa", "Taylor_Green", None).  The initial field follows `init_field_type` (absent: the inlet kind), the Dirichlet
        targets `inlet_type` (Load_mesh.py:86-118); the host-side `bc` records are updated as `reset_env` updates them.  ValueError
        - nothing changed - for an entry without a `bc` record, an unknown kind, a repeated index, or U = 0."""
        from . import meshgen
        idx = [int(i) for i in indices]
        sampled = list(sampled)
        if len(sampled) != len(idx):
            raise ValueError(f"{len(idx)} entries but {len(sampled)} sets of sampled values")
        if len(set(idx)) != len(idx):
            raise ValueError("an entry is given twice in one renewal")
        new_bc, recs = [], (L.RenewRec * max(len(idx), 1))()
        for k, (i, s) in enumerate(zip(idx, sampled)):
            if not 0 <= i < self.n:
                raise ValueError(f"pool entry {i} does not exist (the pool holds {self.n})")
            if self.bc[i] is None:
                raise ValueError("the mesh was given without its 'bc' record (gfv.meshgen.finish_mesh keeps it)")
            bc = dict(self.bc[i])
            for key, v in s.items():
                bc[key] = v if key in ("inlet_type", "init_field_type") else float(v)
            inlet_kind = self._renew_kind(bc["inlet_type"], "inlet_type")
            init_kind = self._renew_kind(bc.get("init_field_type", bc["inlet_type"]), "init_field_type")
            U = float(bc["U"])
            if U == 0.0 or not math.isfinite(U):
                raise ValueError("the inlet velocity U must be finite and non-zero (everything is made dimensionless by it)")
            theta, dt_graph, uvp_dim = meshgen.pde_coefficients(bc)
            p, r = self.plans[i], recs[k]
            r.x, r.y, r.theta, r.dt, r.uvp_dim = (t.data_ptr() for t in (self.x[i], p.y, p.theta, p.dt, p.uvp_dim))
            r.node_type, r.pos, r.N = p.node_type.data_ptr(), self.pos64[i].data_ptr(), int(self.x[i].shape[0])
            aoa = math.radians(float(np.float32(bc["aoa"])))    # (init_env reads the angle from the mesh's fp32 tensor)
            r.U, r.cos_aoa, r.sin_aoa = U, math.cos(aoa), math.sin(aoa)
            r.coef[:] = np.concatenate((theta.reshape(-1), dt_graph.reshape(-1), uvp_dim.reshape(-1))).tolist()
            r.inlet_kind, r.init_kind = inlet_kind, init_kind
            new_bc.append(bc)
        for k, i in enumerate(idx):
            recs[k].yrange = self._yrange_ptr(i)
        lib, stream = L.load(), L.stream_ptr()
        for k0 in range(0, len(idx), L.POOL_MAX_GRAPHS):
            K = min(L.POOL_MAX_GRAPHS, len(idx) - k0)
            rc = lib.gfv_pool_renew(C.addressof(recs) + k0 * C.sizeof(L.RenewRec), K, stream)
            if rc == -1:
                raise ValueError("gfv_pool_renew refused the records")
            L.check(rc, "gfv_pool_renew")
        for i, bc in zip(idx, new_bc):
            self.bc[i].update(bc)

    # ------------------------------------------------------------------------------------------------------------
    def add_variant(self, i, fields=None, **sampled):
        """A new entry over the topology of entry `i` -> its index.  The reference fills its pool by walking the same few mesh
        files again and again with freshly drawn PDE coefficients (Graph_loader.py:98-114: `transform_mesh` of a mesh that is
        already loaded); here such an entry SHARES every structural tensor of entry `i` (same storage, no copy) and owns only what
        `reset_env` changes: the node state `x`, the Dirichlet targets `y`, `theta`, `dt`, `uvp_dim` and the `bc` record.
        `sampled`: as for `reset_env` (applied to the new entry, which restarts its field); `fields` [N, 3]: the (u, v, p) state
        the entry starts from instead."""
        i = int(i)
        src = self.plans[i]
        p = MeshPlan()
        p.__dict__.update({k: v for k, v in vars(src).items() if not k.startswith("_")})
        for a in _VARIANT_OWNED:
            setattr(p, a, getattr(src, a).clone())
        v = self.n
        self.plans.append(p)
        self.x.append(self.x[i].clone())
        self.sizes.append(dict(self.sizes[i]))
        self.bc.append(None if self.bc[i] is None else dict(self.bc[i]))
        self.pos64.append(self.pos64[i])
        for a, (ptrs, words, row_shape, dtype) in self._src.items():
            t = self.x[v] if a == "x" else getattr(p, a)
            self._src[a] = (np.append(ptrs, np.uint64(t.data_ptr())), np.append(words, np.int64(t.numel())), row_shape, dtype)
        self.n = v + 1
        if sampled:
            self.reset_env(v, **sampled)
        if fields is not None:
            f = torch.as_tensor(fields, dtype=torch.float32).to(self.device)
            self.x[v][:, 0:3].copy_(f.reshape(-1, 3))
        return v

    def arena(self, max_graphs, max_sizes=None):
        """Fixed-capacity device memory for batches of up to `max_graphs` entries -> BatchArena.  max_sizes: totals of a batch
        (keys n, e, c, k, s, nchunk: nodes, faces, cells, incidences, stencil entries, slice chunks); default: the `max_graphs`
        largest entries of the pool, size by size."""
        return BatchArena(self, max_graphs, max_sizes)

    # ------------------------------------------------------------------------------------------------------------
    def payback(self, indices, uvp_node):
        """Write the batch's predicted (u, v, p) back into the pool (Data_Pool.payback, Graph_loader.py:370-396)."""
        idx = [int(i) for i in indices]
        o = 0
        for i in idx:
            n = self.sizes[i]["n"]
            self.x[i][:, 0:3].copy_(uvp_node[o:o + n, 0:3])
            o += n
