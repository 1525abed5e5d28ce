#!/usr/bin/env python3
"""Time per closure evaluation of the reference's L-BFGS loop (solve_with_grad_GPU_LBFGS.py:67-202) on the drop-in model, two ways:

  a  torch.optim.LBFGS (the parent's path)
  b  gfv.optim.LBFGS   (csrc/lbfgs.hip)

both with the reference's history_size = 100 and line_search_fn = "strong_wolfe", on the reference's closure.

    python profiles/tools/lbfgs_timing.py --workload cavity|50k [--runs 3] [--iters 160] [--max-iter 20]

prints ONE JSON line and (--out, default profiles/lbfgs_timing.json) merges it into that file under the workload's name.
A run: a fresh model and optimiser per leg, from the same weights; `step()` calls of `--max-iter` iterations each, the legs
ALTERNATING call by call, until each has done `--iters` iterations (so that the history is full for iters - 100 of them).  Per leg
and run: wall time of its step() calls (host clock, each call ending in a device synchronise) over its closure evaluations -
the two legs take slightly different paths, so it is the time PER EVALUATION that compares, not the totals -, the same over the
calls that started with a full history, iterations and evaluations.  `spread_a`: max - min of leg a over the runs.

Per-launch time of leg b comes from a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/tools/lbfgs_timing.py --legs b --workload cavity --runs 1 --out ''
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKLOADS = {"cavity": ("cavity", 5041), "50k": ("cylinder", 50000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cavity")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=160)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import bench                                   # the tree's own workload builder
    from gfv import host as gfv_host
    from gfv.optim import LBFGS
    from gfv.params import default_params
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    wl, cells = WORKLOADS[args.workload]
    graphs, sizes = bench.build_workload(wl, cells, 1, 0, dev)
    params = default_params(dataset_size=1)
    weights = O.init_parameters(0)
    kw = dict(max_iter=args.max_iter, history_size=args.history, tolerance_grad=0.0, tolerance_change=0.0,
              line_search_fn="strong_wolfe")

    def make_leg(leg):
        model = NNmodel(params)
        sd = model.state_dict()
        for k, v in weights.items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        model = model.to(dev)
        hg = tuple(g.clone().to(dev) for g in graphs)
        gn = hg[0]
        x0 = gn.x.clone()
        opt = (torch.optim.LBFGS if leg == "a" else LBFGS)(model.parameters(), **kw)

        def closure():
            opt.zero_grad()
            gn.x = x0.clone()
            gn.norm_uvp, gn.norm_global = params.norm_uvp, params.norm_global
            lc, lmx, lmy, lp, _, _ = model(*hg)
            lb = params.loss_press * lp + params.loss_cont * lc + params.loss_mom * lmx + params.loss_mom * lmy
            loss = torch.mean(torch.log(torch.clamp(lb, min=1e-10, max=1e10)))
            loss.backward()
            return loss

        state = lambda: opt.state[opt.param_groups[0]["params"][0]]   # noqa: E731
        return dict(opt=opt, closure=closure, state=state, wall=0.0, wall_full=0.0, evals_full=0, iters_full=0, calls=0, last=None)

    legs = args.legs.split(",")
    out = {"workload": args.workload, "sizes": sizes, "history_size": args.history, "max_iter_per_step": args.max_iter,
           "iterations_wanted": args.iters, "legs": {leg: {"runs": []} for leg in legs}}
    for _ in range(args.runs):
        L = {leg: make_leg(leg) for leg in legs}
        busy = set(legs)
        while busy:
            for leg in legs:
                if leg not in busy:
                    continue
                g = L[leg]
                st = g["state"]()
                it0, ev0 = st.get("n_iter", 0), st.get("func_evals", 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g["last"] = g["opt"].step(g["closure"])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                st = g["state"]()
                g["wall"] += dt
                g["calls"] += 1
                if it0 >= args.history:
                    g["wall_full"] += dt
                    g["evals_full"] += st["func_evals"] - ev0
                    g["iters_full"] += st["n_iter"] - it0
                if st["n_iter"] >= args.iters or g["calls"] >= 40 * (args.iters // args.max_iter + 1):
                    busy.discard(leg)
        for leg in legs:
            g, st = L[leg], L[leg]["state"]()
            out["legs"][leg]["runs"].append({
                "ms_per_eval": round(1e3 * g["wall"] / st["func_evals"], 4),
                "ms_per_eval_full_history": round(1e3 * g["wall_full"] / max(g["evals_full"], 1), 4),
                "iterations": st["n_iter"], "evaluations": st["func_evals"], "iterations_full_history": g["iters_full"],
                "evaluations_full_history": g["evals_full"], "step_calls": g["calls"], "wall_s": round(g["wall"], 4),
                "last_loss": float(g["last"])})
        del L
        torch.cuda.empty_cache()
    for leg in legs:
        r = out["legs"][leg]["runs"]
        for key in ("ms_per_eval", "ms_per_eval_full_history"):
            vals = [x[key] for x in r]
            out["legs"][leg][key + "_median"] = round(statistics.median(vals), 4)
            out["legs"][leg][key + "_spread"] = round(max(vals) - min(vals), 4)
    if "a" in legs and "b" in legs:
        a, b = out["legs"]["a"], out["legs"]["b"]
        out["spread_a"] = a["ms_per_eval_spread"]
        out["b_below_a_by_more_than_the_spread"] = bool(a["ms_per_eval_median"] - b["ms_per_eval_median"] > a["ms_per_eval_spread"])
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
