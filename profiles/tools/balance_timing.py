#!/usr/bin/env python3
"""What the balancer's launch costs a training step: ms per step of `TrainStep(balance=Inverse())` against
`TrainStep` without a balancer (the parent commit's step: with balance=None no launch of the balancer's is issued and nothing is
allocated), both in list mode on bench.py's workloads, and the launch on its own.

    python profiles/tools/balance_timing.py --workload cavity --cells 5041 | --workload cylinder --cells 50000
                                            [--blocks 7] [--steps 200] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/balance_timing.json) under "<workload>_<cells>".
A run: fresh models from one seed, 10 warm-up steps per leg (the lists are recorded there), then blocks of `--steps` steps, the
two legs ALTERNATING block by block; ms_per_step = host wall time of a block (ending in a synchronisation) over its steps; median,
min and max over the blocks.  The launch alone: 200 back-to-back `gfv_loss_balance` between two device events, us per launch,
for B = 1 and B = 200 graphs, publishing on every launch."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "balance_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    from FVMmodel.importer import NNmodel
    from gfv import lib as L
    from gfv.balance import Inverse
    from gfv.params import default_params
    from gfv.trainer import TrainStep
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    cpu_graphs, sz = bench.build_workload(args.workload, args.cells, 1, 0, "cuda")

    def graphs():
        return tuple(g.clone().to("cuda") for g in cpu_graphs)

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    legs = {"balanced": TrainStep(model(), graphs(), lr=5e-5, use_graph="list", balance=Inverse()),
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
    st = legs["balanced"].balance.stats()
    assert st["n"] + st["n_skipped"] == 10 + args.blocks * args.steps and st["n_updates"] == st["n"] - 10, st
    out = {"workload": args.workload, "cells": sz["C"], "nodes": sz["N"], "steps_per_block": args.steps, "blocks": args.blocks,
           "observations": st["n"], "rejected": st["n_skipped"], "ms_per_step": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["balanced_minus_plain_us"] = round(1e3 * (out["ms_per_step"]["balanced"]["median"]
                                                  - out["ms_per_step"]["plain"]["median"]), 2)

    # ---- the launch alone ----------------------------------------------------------------------------------------------------
    dev, lib = legs["plain"].dev, L.load()
    hyper = torch.zeros(8, dtype=torch.float32, device=dev)
    out["launch_us"] = {}
    for B in (1, 200):
        one = Inverse(warmup=0)
        one.set_base((6e4, 5e4, 1.0))
        rec = one.pack().to(dev)
        terms = torch.rand((B, 4), dtype=torch.float32, device=dev) + 0.5

        def launch():
            L.check(lib.gfv_loss_balance(terms.data_ptr(), B, rec.data_ptr(), hyper.data_ptr(), None, L.stream_ptr()),
                    "gfv_loss_balance")
        for _ in range(20):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            launch()
        e1.record()
        torch.cuda.synchronize()
        assert int(rec.cpu().view(torch.int32)[5]) == LAUNCH_BLOCK + 20          # every launch published
        out["launch_us"][f"B={B}"] = round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)
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
