"""Pool training measurement: the changing-batch loop of pre_train_Adam.py:112-198 (a different batch of the pool every step).

Per configuration, three runs each, medians (and the spread of the three runs of (a)):
  (a) parent path        : pool.batch + TrainStep(use_graph=False).set_batch + step  (set_batch drops any recorded list: eager)
  (b) PoolTrainStep eager: arena.load + step, max_list_bytes=0
  (c) PoolTrainStep list : arena.load + replay of the list of the batch's size signature
  (d) fixed batch, list  : TrainStep(use_graph="list") over ONE batch of the same size (what a changing batch is measured against)
and the assembly alone: arena.load (one launch) against pool.batch.
Configurations: B = 1 at 50 k cells, 16 entries over 2 meshes; 8 entries of ~15 k cells per batch, 16 entries over 2 meshes, every
batch four variants of the first mesh followed by four of the second (ONE ordered size signature: a pool trained this way draws
its batches topology by topology); B = 1 on the 5 k-cell cavity, 8 variants.
`--assemble-only`: just 50 assemblies of the 50 k-cell configuration, for a kernel trace.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gen-fvgn-steady_amd"))
import torch  # noqa: E402

from FVMmodel.importer import NNmodel  # noqa: E402
from gfv import meshgen  # noqa: E402
from gfv.params import default_params  # noqa: E402
from gfv.pool import DevicePool  # noqa: E402
from gfv.pool_trainer import PoolTrainStep  # noqa: E402
from gfv.trainer import TrainStep  # noqa: E402

STEPS, WARM, RUNS = 150, 12, 3
STREAM_TBS = 5.24     # profiles/r03_stream_run.txt: reads 1 writes 1, plain stores, 1024 B runs


def make_pool(kind, cells, n_meshes, n_entries):
    ms, fs = [], []
    for i in range(n_meshes):
        if kind == "cavity":
            raw = meshgen.raw_quad_cavity(n=max(2, int(round(cells ** 0.5))), jitter=0.0, seed=1234 + i)
        else:
            nx, ny = meshgen.cylinder_grid_for_cells(cells)
            raw = meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234 + i)
        m = meshgen.finish_mesh(raw, device="cuda")
        ms.append(m)
        fs.append(meshgen.random_fields(m, seed=1 + i))
    pool = DevicePool(ms, fs)
    j = 0
    while pool.n < n_entries:
        parent = j % n_meshes
        pool.add_variant(parent, fields=meshgen.random_fields(ms[parent], seed=100 + j), U=0.1 + 0.01 * j, mu=1e-3 * (1 + j % 5))
        j += 1
    return pool, n_meshes


def batches(pool, n_meshes, B):
    """step k -> indices.  B = 1: entry k; B > 1: B / n_meshes entries of every mesh, mesh by mesh, other variants every step."""
    per = pool.n // n_meshes      # entry i belongs to mesh i % n_meshes
    if B == 1:
        return lambda k: [k % pool.n]
    q = B // n_meshes
    return lambda k: [m + n_meshes * ((k * q + r) % per) for m in range(n_meshes) for r in range(q)]


def model():
    torch.manual_seed(0)
    return NNmodel(default_params(dataset_size=1)).cuda()


def timed(one, steps=STEPS, warm=WARM):
    for k in range(warm):
        one(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(warm, warm + steps):
        one(k)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def measure(name, kind, cells, n_meshes, n_entries, B):
    pool, nm = make_pool(kind, cells, n_meshes, n_entries)
    pick = batches(pool, nm, B)
    out = {"entries": pool.n, "meshes": nm, "B": B, "cells_per_entry": int(pool.sizes[0]["c"])}
    runs = {k: [] for k in "abcd"}
    # (a)
    ts_a = TrainStep(model(), pool.batch(pick(0))[0], use_graph=False)

    def one_a(k):
        ts_a.set_batch(pool.batch(pick(k))[0])
        ts_a.step()
    ts_b = PoolTrainStep(model(), pool, max_graphs=B, max_list_bytes=0)
    ts_c = PoolTrainStep(model(), pool, max_graphs=B, max_list_bytes=64 << 30)
    ts_d = TrainStep(model(), pool.batch(pick(0))[0], use_graph="list")
    for _ in range(RUNS):
        runs["a"].append(timed(one_a))
        runs["b"].append(timed(lambda k: ts_b.step(pick(k))))
        runs["c"].append(timed(lambda k: ts_c.step(pick(k))))
        runs["d"].append(timed(lambda k: ts_d.step()))
    med = {k: statistics.median(v) for k, v in runs.items()}
    out.update({"ms_a_parent_path": round(med["a"], 4), "ms_b_pool_eager": round(med["b"], 4), "ms_c_pool_list": round(med["c"], 4),
                "ms_d_fixed_batch_list": round(med["d"], 4), "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                "spread_a": round((max(runs["a"]) - min(runs["a"])) / med["a"], 4),
                "c_over_a": round(med["c"] / med["a"], 4), "c_over_d": round(med["c"] / med["d"], 4), "stats_c": ts_c.stats()})
    arena = pool.arena(B)
    asm = [timed(lambda k: arena.load(pick(k)), steps=64, warm=8) for _ in range(RUNS)]
    old = [timed(lambda k: pool.batch(pick(k)), steps=64, warm=8) for _ in range(RUNS)]
    out.update({"ms_assemble_launch": round(statistics.median(asm), 4), "ms_pool_batch": round(statistics.median(old), 4),
                "assemble_bytes": assemble_bytes(arena, pick(0))})
    return name, out


def assemble_bytes(arena, idx):
    """Bytes the assembly launch moves for this batch: 4 read + 4 written per copied word, 4 written per filled word."""
    from gfv import lib as L
    A = len(arena.attrs)
    words = arena._tab[idx][:, L.POOL_ROW_HEAD + A:].sum(0)
    return int(sum((4 if mode == L.POOL_FILL else 8) * int(w) for (a, mode, k), w in zip(arena.attrs, words)))


def main():
    if "--assemble-only" in sys.argv:
        pool, nm = make_pool("cyl", 50000, 2, 4)
        arena = pool.arena(1)
        pick = batches(pool, nm, 1)
        for k in range(50):
            arena.load(pick(k))
        torch.cuda.synchronize()
        print(json.dumps({"assemble_only": True, "launches": 50, "assemble_bytes": assemble_bytes(arena, pick(0)),
                          "stream_rate_TBs": STREAM_TBS}))
        return
    res = {"what": "changing-batch training step, ms per step, medians of 3 runs of %d steps" % STEPS, "stream_rate_TBs": STREAM_TBS}
    for cfg in (("cyl50k_B1", "cyl", 50000, 2, 16, 1), ("cyl15k_B8", "cyl", 15000, 2, 16, 8), ("cavity5k_B1", "cavity", 5041, 1, 8, 1)):
        if "--only" in sys.argv and cfg[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        name, out = measure(*cfg)
        res[name] = out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
