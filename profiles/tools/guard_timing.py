#!/usr/bin/env python3
"""What the training guard costs: gfv.trainer.TrainStep in command-list mode on one batch, two ways,

  off  TrainStep(...)                                           one Adam launch at the end of the step
  on   TrainStep(..., max_grad_norm=<above every norm>, skip_nonfinite=True)
       the norm + decision launch, then the guarded Adam: the same arithmetic (coefficient 1.0), so the two legs train alike

and the norm launch by itself on the step's own flat gradient.

    python profiles/tools/guard_timing.py --workload cavity|50k [--runs 3] [--steps 200] [--warmup 10]

prints ONE JSON line and (--out, default profiles/guard_timing.json) merges it into that file under the workload's name.
A run: a fresh model and TrainStep per leg from the same weights, `--warmup` steps each (warm-up, recording, first replays), then
`--steps` timed steps per leg in blocks of 20, the legs ALTERNATING block by block; ms_per_step = host wall time of a leg's blocks
(each ending in a device synchronise) over its steps.  `spread_off`: max - min of leg off over the runs.
guard_launch_us: device time between two events around `--launches` norm launches issued back to back, over their number (the
gradient is then L2 / Infinity-Cache warm, as it is behind the backward that has just written it)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKLOADS = {"cavity": ("cavity", 5041), "50k": ("cylinder", 50000)}
BLOCK = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cavity")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import bench                                   # the tree's own workload builder
    from gfv import host as gfv_host
    from gfv import lib as L
    from gfv.params import default_params
    from gfv.trainer import TrainStep
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    wl, cells = WORKLOADS[args.workload]
    graphs, sizes = bench.build_workload(wl, cells, 1, 0, dev)
    params = default_params(dataset_size=1)
    weights = O.init_parameters(0)

    def make_leg(leg):
        model = NNmodel(params)
        sd = model.state_dict()
        for k, v in weights.items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        model = model.to(dev)
        hg = tuple(g.clone().to(dev) for g in graphs)
        kw = dict(max_grad_norm=1e30, skip_nonfinite=True) if leg == "on" else {}
        ts = TrainStep(model, hg, use_graph="list", want_outputs=False, **kw)
        for _ in range(args.warmup):
            ts.step()
        torch.cuda.synchronize()
        return dict(ts=ts, wall=0.0, steps=0)

    legs = ("off", "on")
    out = {"workload": args.workload, "sizes": sizes, "timed_steps_per_leg": args.steps, "legs": {leg: {"runs": []} for leg in legs},
           "guard_launch_us": []}
    for _ in range(args.runs):
        G = {leg: make_leg(leg) for leg in legs}
        while any(g["steps"] < args.steps for g in G.values()):
            for leg in legs:
                g = G[leg]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(BLOCK):
                    g["ts"].step()
                torch.cuda.synchronize()
                g["wall"] += time.perf_counter() - t0
                g["steps"] += BLOCK
        for leg in legs:
            g = G[leg]
            out["legs"][leg]["runs"].append({"ms_per_step": round(1e3 * g["wall"] / g["steps"], 4), "final_loss": float(g["ts"].loss)})
        # the norm launch alone, on the gradient the last step left
        ts = G["on"]["ts"]
        gd, lib = ts._guard, L.load()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(2):
            e0.record()
            for _ in range(args.launches):
                L.check(lib.gfv_grad_guard_dev(ts.flat_g.data_ptr(), gd.segs.data_ptr(), gd.n_seg, gd.n_elems, ts.hyper.data_ptr(),
                                               gd.guard.data_ptr(), gd.ws.data_ptr(), L.stream_ptr()), "grad_guard")
            e1.record()
            torch.cuda.synchronize()
        out["guard_launch_us"].append(round(1e3 * e0.elapsed_time(e1) / args.launches, 3))
        out["guard_segments"], out["guard_elements"] = gd.n_seg, gd.n_elems
        out["guard_stats"] = ts.guard_stats()
        del G, ts
        torch.cuda.empty_cache()
    for leg in legs:
        vals = [x["ms_per_step"] for x in out["legs"][leg]["runs"]]
        out["legs"][leg]["ms_per_step_median"] = round(statistics.median(vals), 4)
        out["legs"][leg]["ms_per_step_spread"] = round(max(vals) - min(vals), 4)
    out["spread_off"] = out["legs"]["off"]["ms_per_step_spread"]
    out["on_minus_off_us"] = round(1e3 * (out["legs"]["on"]["ms_per_step_median"] - out["legs"]["off"]["ms_per_step_median"]), 2)
    out["guard_launch_us_median"] = round(statistics.median(out["guard_launch_us"]), 3)
    print(json.dumps(out))
    if args.out:
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[args.workload] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
