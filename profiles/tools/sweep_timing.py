#!/usr/bin/env python3
"""Wall time of running a trained model over a six-variant pool (one ~5 k-cell cylinder mesh + five variants with other U, mu, dt
and fields) at equal `max_steps`, two ways:

  sweep    gfv.sweep.Sweep(model, pool, max_graphs=2, tol=-1, max_steps=S).run() - construction included
  rollout  one gfv.rollout.Rollout per batch of two (pool.batch + Rollout + run(steps=S) + pool.payback) - construction included

    python profiles/tools/sweep_timing.py [--cells 5000] [--steps 200] [--runs 3] [--out FILE]

prints ONE JSON line (and writes it to --out).  `tol=-1`: nothing converges, so both legs take exactly S steps per entry and the
comparison is of the machinery, not of a convergence rate.  Both legs run once untimed with 3 steps first (library load, kernel
code objects, allocator); the timed runs alternate.  Host clock around a leg, ending in a device synchronise.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from FVMmodel.importer import NNmodel
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.params import default_params
    from gfv.pool import DevicePool
    from gfv.rollout import Rollout
    from gfv.sweep import Sweep
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    nx, ny = meshgen.cylinder_grid_for_cells(args.cells)
    mesh = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234), U=0.15)

    def make_pool():
        pool = DevicePool([mesh], [meshgen.random_fields(mesh, seed=5)])
        for j in range(5):
            pool.add_variant(0, fields=meshgen.random_fields(mesh, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
        return pool

    def make_model():
        model = NNmodel(default_params(dataset_size=1))      # a trained model: the Normalizer no longer accumulates
        sd = model.state_dict()
        for k, v in O.init_parameters(0).items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        return model.cuda()

    stats = {}

    def sweep_leg(model, pool, steps):
        sw = Sweep(model, pool, max_graphs=2, tol=-1, max_steps=steps)
        sw.run()
        stats.update(sw.stats())

    def rollout_leg(model, pool, steps):
        for pair in ([0, 1], [2, 3], [4, 5]):
            graphs, _ = pool.batch(pair)
            r = Rollout(model, graphs, max_steps=steps)
            for _ in range(steps):
                r.step()
            pool.payback(pair, r.x_backup[:, 0:3])

    legs = {"sweep": sweep_leg, "rollout": rollout_leg}
    models = {name: make_model() for name in legs}           # (one engine per leg: neither rebuilds the other's weight images)
    for name, leg in legs.items():
        leg(models[name], make_pool(), 3)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(args.runs):
        for name, leg in legs.items():
            pool = make_pool()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg(models[name], pool, args.steps)
            torch.cuda.synchronize()
            times[name].append(round(time.perf_counter() - t0, 4))
    out = {"cells": int(make_pool().sizes[0]["c"]), "entries": 6, "slots": 2,
           "max_steps": args.steps, "wall_s": times, "wall_s_median": {k: statistics.median(v) for k, v in times.items()},
           "sweep_stats": stats}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
