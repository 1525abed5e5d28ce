#!/usr/bin/env python3
"""What gradient accumulation buys on a heterogeneous pool: 16 meshes of 16 DISTINCT sizes around `--cells`, one
optimiser step over 8 of them drawn at random, three ways,

  a  PoolTrainStep(max_graphs=8)                     one step over the batch of 8 (up to 16^8 ordered signatures: eager for good)
  b  PoolTrainStep(max_graphs=1, accum_steps=8)      eight micro-steps of 1 (16 signatures: every list recorded and replayed)
  c  PoolTrainStep(max_graphs=2, accum_steps=4)      four micro-steps of 2 (up to 240 ordered signatures)

over the SAME draws, and on one repeated signature the cost per micro-step of

  pair   PoolTrainStep(max_graphs=1, accum_steps=2)  three launches at the end of the step (two of them near-empty on a hold)
  plain  PoolTrainStep(max_graphs=1)                 the one Adam launch

    python profiles/tools/accum_timing.py --cells 5000|15000 [--legs a,b,c,pair,plain] [--root TREE] [--label NAME]

prints ONE JSON line and (--out, default profiles/accum_timing.json) merges it into that file under `--label` (default
"<cells>").  `--root`: measure the package of ANOTHER checkout of this repository (the parent commit: legs a and plain exist there)
with this one tool, so that both sides of a comparison are timed by the same code; run the two alternately.
A run: fresh models from one seed, `--warmup` optimiser steps per leg, then `--opt-steps` timed ones in blocks of 10, the legs
ALTERNATING block by block; ms_per_opt_step = host wall time of a leg's blocks (each ending in a device synchronise) over its
optimiser steps.  pair / plain: blocks of 40 micro-steps of entry 0, alternating, ms per micro-step."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BLOCK, MICRO_BLOCK = 10, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=5000)
    ap.add_argument("--legs", default="a,b,c,pair,plain")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--opt-steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--micro-steps", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_timing.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (root, os.path.join(root, "gen-fvgn-steady_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from FVMmodel.importer import NNmodel
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.params import default_params
    from gfv.pool import DevicePool, batch_signature
    from gfv.pool_trainer import PoolTrainStep
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    legs = [x for x in args.legs.split(",") if x]
    assert set(legs) <= {"a", "b", "c", "pair", "plain"}, legs

    # 16 meshes, 16 sizes: the channel grid grows by one column per mesh around the grid of `--cells`
    nx0, ny0 = meshgen.cylinder_grid_for_cells(args.cells)
    ms, fs = [], []
    for i in range(16):
        m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx0 - 8 + i, ny=ny0, jitter=0.2, seed=1234 + i), device="cuda")
        ms.append(m)
        fs.append(meshgen.random_fields(m, seed=1 + i))

    def make_pool():
        return DevicePool(ms, fs)
    probe = make_pool()
    cells = [int(s["c"]) for s in probe.sizes]
    assert len({batch_signature(probe.sizes, [i]) for i in range(16)}) == 16, "the 16 meshes must have 16 distinct signatures"
    del probe

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    rng = np.random.default_rng(7)
    draws = [rng.choice(16, size=8, replace=False).tolist() for _ in range(args.warmup + args.opt_steps + BLOCK)]
    CONF = {"a": dict(max_graphs=8), "b": dict(max_graphs=1, accum_steps=8), "c": dict(max_graphs=2, accum_steps=4)}

    def opt_step(leg, ts, d):
        if leg == "a":
            ts.step(d)
        elif leg == "b":
            for i in d:
                ts.step([i])
        else:
            for j in range(0, 8, 2):
                ts.step(d[j:j + 2])

    out = {"cells_target": args.cells, "cells": cells, "root_is_this_tree": root == ROOT, "opt_steps_per_leg": args.opt_steps,
           "legs": {leg: {"runs": []} for leg in legs}}
    for _ in range(args.runs):
        G = {}
        for leg in legs:
            if leg in CONF:
                ts = PoolTrainStep(model(), make_pool(), want_outputs=False, **CONF[leg])
                for k in range(args.warmup):
                    opt_step(leg, ts, draws[k])
            else:
                ts = PoolTrainStep(model(), make_pool(), max_graphs=1, want_outputs=False, **(dict(accum_steps=2) if leg == "pair" else {}))
                for k in range(12):
                    ts.step([0])
            torch.cuda.synchronize()
            G[leg] = dict(ts=ts, wall=0.0, steps=0)
        goal = {leg: (args.opt_steps if leg in CONF else args.micro_steps) for leg in legs}
        while any(G[leg]["steps"] < goal[leg] for leg in legs):
            for leg in legs:
                g = G[leg]
                if g["steps"] >= goal[leg]:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg in CONF:
                    for k in range(BLOCK):
                        opt_step(leg, g["ts"], draws[args.warmup + g["steps"] + k])
                    n = BLOCK
                else:
                    for k in range(MICRO_BLOCK):
                        g["ts"].step([0])
                    n = MICRO_BLOCK
                torch.cuda.synchronize()
                g["wall"] += time.perf_counter() - t0
                g["steps"] += n
        for leg in legs:
            g = G[leg]
            key = "ms_per_opt_step" if leg in CONF else "ms_per_micro_step"
            out["legs"][leg]["runs"].append({key: round(1e3 * g["wall"] / g["steps"], 4), "stats": g["ts"].stats()})
        del G
        torch.cuda.empty_cache()
    for leg in legs:
        key = "ms_per_opt_step" if leg in CONF else "ms_per_micro_step"
        vals = [x[key] for x in out["legs"][leg]["runs"]]
        out["legs"][leg][key + "_median"] = round(statistics.median(vals), 4)
        out["legs"][leg][key + "_spread"] = round(max(vals) - min(vals), 4)
    med = {leg: next(v for k, v in out["legs"][leg].items() if k.endswith("_median")) for leg in legs}
    for x in ("b", "c"):
        if x in med and "a" in med:
            out[x + "_over_a"] = round(med[x] / med["a"], 4)
    if "pair" in med and "plain" in med:
        out["pair_minus_plain_us_per_micro_step"] = round(1e3 * (med["pair"] - med["plain"]), 2)
    print(json.dumps(out))
    if args.out:
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[args.label or str(args.cells)] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
