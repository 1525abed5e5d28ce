#!/usr/bin/env python3
"""What the averaged weights cost, in two parts.

  launch  the Adam launch alone on the flat buffers of the model (n = its parameter count, alignment padding included):
            off  gfv_adam_step_dev        28 bytes per element
            on   gfv_adam_step_ema_dev    36 bytes per element (guard == NULL, accum == NULL)
          device time between two events around `--launches` launches issued back to back, over their number, in blocks that
          ALTERNATE between the two (the buffers are then L2 / Infinity-Cache warm, as they are behind a backward that has just
          written the gradient).
  step    gfv.trainer.TrainStep in command-list mode on the 5 k-cell cavity:
            off  TrainStep(...)                    ema_decay=None
            on   TrainStep(..., ema_decay=0.999)
          `--warmup` steps each (warm-up, recording, first replays), then `--steps` timed steps per leg in blocks of 20, the legs
          ALTERNATING block by block; ms_per_step = host wall time of a leg's blocks (each ending in a device synchronise) over
          its steps.

    python profiles/tools/ema_timing.py [--legs off,on] [--root TREE] [--label NAME] [--runs 3] [--steps 200] [--warmup 10]

prints ONE JSON line and (--out, default profiles/ema_timing.json) merges it into that file under `--label` (default "this").
`--root`: measure the package of ANOTHER checkout of this repository (the parent commit: only the off legs exist there, so
`--legs off --label parent`) with this one tool, so that both sides of a comparison are timed by the same code; run the two
alternately."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BLOCK = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--launch-blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_timing.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (root, os.path.join(root, "gen-fvgn-steady_amd"), os.path.join(root, "tests", "golden")):
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
    legs = tuple(x for x in args.legs.split(",") if x)
    assert legs and set(legs) <= {"off", "on"}, legs
    dev = torch.device("cuda:0")
    graphs, sizes = bench.build_workload("cavity", 5041, 1, 0, dev)
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
        ts = TrainStep(model, hg, use_graph="list", want_outputs=False, **(dict(ema_decay=0.999) if leg == "on" else {}))
        for _ in range(args.warmup):
            ts.step()
        torch.cuda.synchronize()
        return dict(ts=ts, wall=0.0, steps=0)

    out = {"sizes": sizes, "root_is_this_tree": root == ROOT, "timed_steps_per_leg": args.steps,
           "step": {leg: {"runs": []} for leg in legs}, "launch": {leg: {"us": []} for leg in legs}}
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
            out["step"][leg]["runs"].append({"ms_per_step": round(1e3 * g["wall"] / g["steps"], 4), "final_loss": float(g["ts"].loss)})
        # the Adam launch alone, on copies of the buffers the last step left (lr 0: the timed launches move nothing but the moments)
        ts = G[legs[0]]["ts"]
        lib, n = L.load(), ts.n_params
        p, g_, m, v = (t.detach().clone() for t in (ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v))
        state, hyper = ts.adam_state.clone(), ts.hyper.clone()
        hyper[0] = 0.0
        out["n_params"] = n
        if "on" in legs:
            e, rec = p[:n].clone(), torch.zeros(8, dtype=torch.float32, device=dev)
            L.check(lib.gfv_ema_init(rec.data_ptr(), 0.999, 1, 0, L.stream_ptr()), "ema_init")

        def launch(leg):
            if leg == "on":
                L.check(lib.gfv_adam_step_ema_dev(p.data_ptr(), g_.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n,
                                                  state.data_ptr(), hyper.data_ptr(), None, None, rec.data_ptr(), L.stream_ptr()),
                        "adam_step_ema")
            else:
                L.check(lib.gfv_adam_step_dev(p.data_ptr(), g_.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(),
                                              hyper.data_ptr(), L.stream_ptr()), "adam_step")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = {leg: [] for leg in legs}
        for blk in range(args.launch_blocks + 1):          # (the first block of each leg warms up and is dropped)
            for leg in legs:
                e0.record()
                for _ in range(args.launches):
                    launch(leg)
                e1.record()
                torch.cuda.synchronize()
                if blk:
                    per[leg].append(1e3 * e0.elapsed_time(e1) / args.launches)
        for leg in legs:
            out["launch"][leg]["us"].append(round(statistics.median(per[leg]), 3))
        del G, ts
        torch.cuda.empty_cache()
    for leg in legs:
        vals = [x["ms_per_step"] for x in out["step"][leg]["runs"]]
        out["step"][leg]["ms_per_step_median"] = round(statistics.median(vals), 4)
        out["step"][leg]["ms_per_step_spread"] = round(max(vals) - min(vals), 4)
        out["launch"][leg]["us_median"] = round(statistics.median(out["launch"][leg]["us"]), 3)
        out["launch"][leg]["us_spread"] = round(max(out["launch"][leg]["us"]) - min(out["launch"][leg]["us"]), 3)
    if set(legs) == {"off", "on"}:
        out["step_on_minus_off_us"] = round(1e3 * (out["step"]["on"]["ms_per_step_median"] - out["step"]["off"]["ms_per_step_median"]), 2)
        out["launch_on_minus_off_us"] = round(out["launch"]["on"]["us_median"] - out["launch"]["off"]["us_median"], 3)
    print(json.dumps(out))
    if args.out:
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[args.label] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
