#!/usr/bin/env python3
"""What the observation term costs a training step: ms per step of `TrainStep(observations=...)` with EVERY node and
channel observed against `TrainStep` without observations (the parent commit's step: with observations=None no launch of the term
is issued and nothing is allocated), both in list mode on bench.py's workloads, the two launches on their own, and the number of
recorded commands of both lists.

    python profiles/tools/observe_timing.py --workload cavity --cells 5041 | --workload cylinder --cells 50000
                                            [--blocks 7] [--steps 200] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/observe_timing.json) under "<workload>_<cells>".
A run: fresh models from one seed, 10 warm-up steps per leg (the lists are recorded there), then blocks of `--steps` steps, the
two legs ALTERNATING block by block; ms_per_step = host wall time of a block (ending in a synchronisation) over its steps; median,
min and max over the blocks.  The launches alone: 200 back-to-back `gfv_obs_fwd` (and `gfv_obs_bwd`) on the step's own tensors
between two device events, us per launch."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LAUNCH_BLOCK = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cavity", choices=("cavity", "cylinder"))
    ap.add_argument("--cells", type=int, default=5041)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observe_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    from FVMmodel.importer import NNmodel
    from gfv.observe import Observations
    from gfv.params import default_params
    from gfv.trainer import TrainStep
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    cpu_graphs, sz = bench.build_workload(args.workload, args.cells, 1, 0, "cuda")

    def graphs():
        return tuple(g.clone().to("cuda") for g in cpu_graphs)

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    g_obs = graphs()
    target = g_obs[0].x[:, 0:3].clone()                     # every node and channel observed: the initial state, weight 1
    obs = Observations(target, torch.ones_like(target), weight=1e6)
    legs = {"observed": TrainStep(model(), g_obs, lr=5e-5, use_graph="list", observations=obs),
            "plain": TrainStep(model(), graphs(), lr=5e-5, use_graph="list")}
    for ts in legs.values():
        for _ in range(10):
            ts.step()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, ts in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts.step()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    rec = obs.read()
    assert float(rec[0, 1]) == 3.0 * sz["N"] and float(rec[0, 0]) > 0, rec
    out = {"workload": args.workload, "cells": sz["C"], "nodes": sz["N"], "steps_per_block": args.steps, "blocks": args.blocks,
           "ms_per_step": {}, "recorded_commands": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["recorded_commands"][name] = sorted(len(e.cl) for e in legs[name]._lists.values())
    out["observed_minus_plain_us"] = round(1e3 * (out["ms_per_step"]["observed"]["median"]
                                                  - out["ms_per_step"]["plain"]["median"]), 2)

    # ---- the launches alone, on the tensors of the observed leg's last step ---------------------------------------------------
    ts = legs["observed"]
    ts.use_graph = False
    ts.step()                                               # (an eager step: its saved tensors are not a list's)
    pl, dev = ts.plan, ts.dev
    phi = torch.rand((pl.N, 8), dtype=torch.float32, device=dev)
    dec = torch.rand((pl.N, 3), dtype=torch.float32, device=dev)
    g_dec = torch.zeros((pl.N, 3), dtype=torch.float32, device=dev)
    loss, gloss = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros((pl.B, 4), dtype=torch.float32, device=dev)
    calls = {"gfv_obs_fwd": lambda: obs.fwd(phi, pl, ts.losses, ts.hyper, loss, gloss),
             "gfv_obs_bwd": lambda: obs.bwd(dec, phi, pl, g_dec)}
    out["launch_us"] = {}
    for name, launch in calls.items():
        for _ in range(20):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            launch()
        e1.record()
        torch.cuda.synchronize()
        out["launch_us"][name] = round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)
    print(json.dumps(out))
    if args.out:
        key = f"{args.workload}_{args.cells}"
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[key] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
