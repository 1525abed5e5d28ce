#!/usr/bin/env python3
"""What Anderson acceleration of the rollout costs per step and what it buys in steps.  No pass / fail.

  cost     ms per step of gfv.rollout.Rollout in command-list mode with anderson = 0 and anderson = 5 on the 5 041-cell cavity and
           on the 50 k-cell cylinder mesh (initial weights: the cost of a step does not depend on them, as long as the steps ARE
           accelerated - the mean depth used over the timed steps is reported beside the time).  Per leg `--warmup` steps (warm-up,
           recording, first replays); then blocks that ALTERNATE between the legs: reset(), 8 untimed steps (the ring fills), a
           synchronise, `--block` timed steps, a synchronise.  Reported: median and min / max over the blocks of a leg.
           Expected from DESIGN.md 9: two kernel boundaries (1.6 - 2.6 us each) plus about (2 m + 4) * 12 bytes per node.
  benefit  the cavity model trained with gfv.trainer.TrainStep for `--train-steps` steps; then, for m in {0, 3, 5, 8}, a Rollout
           from the initial field: steps and wall time until every graph's || G(x) - x || / || G(x) || is below `--tol`
           (checked every `--check-every` steps; `--max-steps` at most), and the restarts.

    python profiles/tools/anderson_timing.py [--parts cost,benefit] [--blocks 7] [--block 20] [--train-steps 2000]

prints ONE JSON line and (--out, default profiles/anderson_timing.json) writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FILL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cost,benefit")
    ap.add_argument("--workloads", default="cavity,50k")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anderson_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import bench                                   # the tree's own workload builder
    from gfv import host as gfv_host
    from gfv.params import default_params
    from gfv.rollout import Rollout
    from gfv.trainer import TrainStep
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    parts = tuple(x for x in args.parts.split(",") if x)
    WORKLOADS = {"cavity": ("cavity", 5041), "50k": ("cylinder", 50000)}

    def new_model():
        model = NNmodel(default_params(dataset_size=1))      # a trained model: the Normalizer no longer accumulates
        sd = model.state_dict()
        for k, v in O.init_parameters(0).items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        return model.to(dev)

    def fresh(graphs):
        hg = tuple(g.clone().to(dev) for g in graphs)
        hg[0].norm_uvp, hg[0].norm_global = True, True
        return hg

    out = {"depth": args.depth, "block_steps": args.block, "blocks_per_leg": args.blocks}
    if "cost" in parts:
        out["cost"] = {}
        for name in (w for w in args.workloads.split(",") if w):
            graphs, sizes = bench.build_workload(*WORKLOADS[name], 1, 0, dev)
            model = new_model()
            room = args.warmup + FILL + args.block + 8
            legs = {m: Rollout(model, fresh(graphs), max_steps=room, anderson=m) for m in (0, args.depth)}
            for r in legs.values():
                for _ in range(args.warmup):
                    r.step()
            torch.cuda.synchronize()
            ms = {m: [] for m in legs}
            used = []
            for _ in range(args.blocks):
                for m, r in legs.items():
                    r.reset()
                    for _ in range(FILL):
                        r.step()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.block):
                        r.step()
                    torch.cuda.synchronize()
                    ms[m].append(1e3 * (time.perf_counter() - t0) / args.block)
                    if m:
                        used.append(float(r.anderson_history()[FILL:, :, 2].mean()))
            res = {"sizes": sizes, "nodes": int(legs[0].plan.N)}
            for m in legs:
                res[f"anderson_{m}"] = {"ms_per_step_median": round(statistics.median(ms[m]), 5),
                                        "ms_per_step_min": round(min(ms[m]), 5), "ms_per_step_max": round(max(ms[m]), 5)}
            res["on_minus_off_us"] = round(1e3 * (statistics.median(ms[args.depth]) - statistics.median(ms[0])), 2)
            res["mean_depth_used_in_timed_steps"] = round(statistics.mean(used), 3)
            res["expected_extra_bytes_per_step"] = (2 * args.depth + 4) * 12 * res["nodes"]
            out["cost"][name] = res
            del legs, model
            torch.cuda.empty_cache()
    if "benefit" in parts:
        graphs, sizes = bench.build_workload("cavity", 5041, 1, 0, dev)
        model = new_model()
        ts = TrainStep(model, fresh(graphs), use_graph="list", want_outputs=False)
        first = None
        for i in range(args.train_steps):
            ts.step()
            if i == 0:
                first = float(ts.loss)
        torch.cuda.synchronize()
        ben = {"sizes": sizes, "train_steps": args.train_steps, "train_loss_first": first, "train_loss_last": float(ts.loss),
               "tol": args.tol, "max_steps": args.max_steps, "check_every": args.check_every, "runs": {}}
        del ts
        for m in (0, 3, 5, 8):
            r = Rollout(model, fresh(graphs), max_steps=args.max_steps, anderson=m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = r.run(steps=args.max_steps, tol=args.tol, check_every=args.check_every)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if m:
                tab = r.anderson_history()
                ratio = (tab[:, :, 0] / tab[:, :, 1]).max(dim=1).values
                extra = {"restarts": r.anderson_stats()["restarts"],
                         "flag_counts": {n: int((tab[:, :, 3] == f).sum()) for f, n in ((1, "nonfinite"), (2, "growth"), (4, "singular"))}}
            else:
                ratio = (hist[:, :, 4] / hist[:, :, 5]).max(dim=1).values
                extra = {}
            ben["runs"][f"anderson_{m}"] = dict(steps=int(r.steps_done), converged=bool(ratio[-1] < args.tol), wall_s=round(wall, 4),
                                               last_ratio=float(ratio[-1]), best_ratio=float(ratio[torch.isfinite(ratio)].min())
                                               if bool(torch.isfinite(ratio).any()) else None, **extra)
        out["benefit"] = ben
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
