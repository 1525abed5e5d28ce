#!/usr/bin/env python3
"""What re-drawing the boundary conditions of pool entries costs, two ways, on a pool of eight entries over one
~15 k-cell channel mesh (seven `add_variant` entries: own state, shared topology):

  renew       DevicePool.renew(indices, sampled): one launch of gfv_pool_renew for all K entries, no synchronisation
  reset_env   K calls of DevicePool.reset_env: per entry ~25 torch launches, two boolean-mask indexings (a synchronising
              `nonzero` each) and a blocking upload of 13 scalars

(a) the call alone, K = 1 and K = 8: `--reps` repetitions per way and K, the ways ALTERNATING repetition by repetition, every
    repetition fenced by one torch.cuda.synchronize() (after one in front of the clock): host wall time until the device is idle;
(b) a PoolTrainStep loop of `--steps` replayed steps (max_graphs = 1, list mode, recorded in the warm-up) with ONE K = 8 renewal
    in the middle, both ways, `--loops` loops per way, alternating, one synchronisation at the end of a loop.

Reported per figure: the median and the spread (min, max) over the repetitions.  No threshold: the figures are what they are.

    python profiles/tools/renew_timing.py [--cells 15000] [--reps 30] [--loops 7] [--steps 40] [--warmup 5] [--out FILE]

prints ONE JSON line and (--out, default profiles/renew_timing.json) writes it there."""
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

N_ENTRIES = 8
WAYS = ("renew", "reset_env")


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=15000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loops", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "renew_timing.json"))
    args = ap.parse_args()
    import torch
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.params import default_params
    from gfv.pool import DevicePool
    from gfv.pool_trainer import PoolTrainStep
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    nx, ny = meshgen.cylinder_grid_for_cells(args.cells)
    mesh = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234), U=0.15, device=dev)

    def make_pool():
        pool = DevicePool([mesh], [meshgen.random_fields(mesh, seed=1)], device=dev)
        for j in range(N_ENTRIES - 1):
            pool.add_variant(0, fields=meshgen.random_fields(mesh, seed=2 + j), U=0.10 + 0.01 * j, mu=1e-3 * (1 + 0.1 * j))
        return pool

    count = [0]

    def draws(K):
        count[0] += 1
        return [dict(U=0.1 + 0.001 * ((count[0] + 7 * k) % 97), mu=1e-3 * (1 + 0.01 * (count[0] % 13)), dt=0.02) for k in range(K)]

    def redraw(pool, way, idx, sampled):
        if way == "renew":
            pool.renew(idx, sampled)
        else:
            for i, s in zip(idx, sampled):
                pool.reset_env(i, **s)

    # both ways write the same bits (tests/test_pool_renew_gpu.py holds them to that; checked here at the size that is timed)
    pa, pb = make_pool(), make_pool()
    s = draws(N_ENTRIES)
    redraw(pa, "renew", list(range(N_ENTRIES)), s)
    redraw(pb, "reset_env", list(range(N_ENTRIES)), s)
    torch.cuda.synchronize()
    for i in range(N_ENTRIES):
        assert torch.equal(pa.x[i], pb.x[i]) and torch.equal(pa.plans[i].y, pb.plans[i].y), i
        assert torch.equal(pa.plans[i].theta, pb.plans[i].theta), i
    del pb
    pool = pa
    out = {"entries": N_ENTRIES, "cells_per_entry": int(pool.sizes[0]["c"]), "nodes_per_entry": int(pool.sizes[0]["n"]),
           "reps": args.reps, "call_ms": {}, "loop": {}}

    # (a) the call alone
    for K in (1, N_ENTRIES):
        idx = list(range(K))
        for way in WAYS:
            for _ in range(args.warmup):
                redraw(pool, way, idx, draws(K))
        torch.cuda.synchronize()
        ms = {way: [] for way in WAYS}
        for _ in range(args.reps):
            for way in WAYS:
                sampled = draws(K)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                redraw(pool, way, idx, sampled)
                torch.cuda.synchronize()
                ms[way].append(1e3 * (time.perf_counter() - t0))
        out["call_ms"][f"K={K}"] = {way: summary(ms[way]) for way in WAYS}
        out["call_ms"][f"K={K}"]["reset_env_over_renew"] = round(statistics.median(ms["reset_env"]) / statistics.median(ms["renew"]), 2)

    # (b) inside a training loop of replayed steps
    model = NNmodel(default_params(dataset_size=1))
    sd = model.state_dict()
    for k, v in O.init_parameters(0).items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    ts = PoolTrainStep(model.to(dev), pool, max_graphs=1, lr=1e-4, use_graph="list")
    everyone = list(range(N_ENTRIES))

    def loop(way):
        for k in range(args.steps):
            if k == args.steps // 2:
                redraw(pool, way, everyone, draws(N_ENTRIES))
            ts.step([k % N_ENTRIES])
        torch.cuda.synchronize()

    for way in WAYS:
        loop(way)                                  # (the first: two eager steps and the recording)
    before = dict(ts.stats())
    ms = {way: [] for way in WAYS}
    for _ in range(args.loops):
        for way in WAYS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(way)
            ms[way].append(1e3 * (time.perf_counter() - t0))
    after = ts.stats()
    assert after["recorded"] == before["recorded"] and after["replayed"] - before["replayed"] == 2 * args.loops * args.steps, (before, after)
    out["loop"] = {"steps": args.steps, "loops": args.loops, "renewal": f"K={N_ENTRIES} after step {args.steps // 2}",
                   "ms_per_loop": {way: summary(ms[way]) for way in WAYS}}
    out["loop"]["reset_env_minus_renew_ms"] = round(statistics.median(ms["reset_env"]) - statistics.median(ms["renew"]), 4)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
