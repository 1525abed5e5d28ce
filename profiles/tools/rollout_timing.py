#!/usr/bin/env python3
"""Time per step of running a trained model forward in time (the loop of solve_without_grad_GPU.py:117-173), four ways:

  a  the parent commit's way: `with torch.no_grad(): model(*graphs)` + the two copies of the write-back, on a checkout of the
     parent commit (--parent-tree DIR: an exported, built tree of it; without it leg a is reported as not measured)
  b  the same call on this tree (the forward-only engine path behind torch.no_grad())
  c  gfv.rollout.Rollout, launch_mode="eager"
  d  gfv.rollout.Rollout, launch_mode="cmd_list"

    python profiles/tools/rollout_timing.py --workload cavity|50k|poly [--parent-tree DIR] [--steps 200] [--runs 5]

prints ONE JSON line and (--out, default profiles/rollout_timing.json) merges it into that file under the workload's name.
Per leg: the `--runs` timed windows of `--steps` steps each (host clock around the window, ending in a device synchronise, after
`--warmup` untimed steps that include every recording), their median, and the peak of torch.cuda.max_memory_allocated over the
windows.  Every tree runs in a process of its own (nothing of one version is imported into the other); the legs of this tree are
interleaved window by window in one process, and the parent's leg is run before AND after them, so that a drift of the box shows
as a difference between `a_first` and `a_second`.  Host threads are pinned as bench.py pins them (gfv.host.pin_to_l3).

Per-kernel time of leg d comes from a run of its own - tracing slows the host, so never beside the timing above:

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/tools/rollout_timing.py --child d --workload 50k --runs 1 --steps 50

(counters, if wanted, in yet another run with --pmc and no tracing beside it).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKLOADS = {"cavity": ("cavity", 5041), "50k": ("cylinder", 50000), "poly": ("poly", 0)}


def child(args):
    root = os.path.abspath(args.root or ROOT)
    for p in (root, os.path.join(root, "gen-fvgn-steady_amd"), os.path.join(root, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import bench                                   # the tree's own workload builder
    from gfv import host as gfv_host
    from gfv.params import default_params
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    wl, cells = WORKLOADS[args.workload]
    graphs, sizes = bench.build_workload(wl, cells, 1, 0, dev)
    model = NNmodel(default_params(dataset_size=1))      # a trained model: the Normalizer no longer accumulates
    sd = model.state_dict()
    for k, v in O.init_parameters(0).items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    model = model.to(dev)

    def fresh():
        hg = tuple(g.clone().to(dev) for g in graphs)
        hg[0].norm_uvp, hg[0].norm_global = True, True
        return hg

    def no_grad_leg():
        hg = fresh()
        gn = hg[0]
        x_backup = gn.x.clone()

        def step():
            gn.norm_uvp = gn.norm_global = True
            with torch.no_grad():
                out = model(*hg)
            x_backup[:, 0:3].copy_(out[4])
            gn.x.copy_(x_backup)
        return step

    def rollout_leg(mode):
        from gfv.rollout import Rollout
        r = Rollout(model, fresh(), max_steps=args.warmup + args.runs * args.steps + 8, launch_mode=mode)
        return r.step

    legs = {}
    for leg in args.child.split(","):
        legs[leg] = no_grad_leg() if leg in ("a", "b") else rollout_leg("eager" if leg == "c" else "cmd_list")
    for step in legs.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    res = {leg: {"ms_per_step_runs": [], "peak_alloc_MiB": 0.0} for leg in legs}
    for _ in range(args.runs):
        for leg, step in legs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[leg]["ms_per_step_runs"].append(round(1e3 * dt / args.steps, 5))
            res[leg]["peak_alloc_MiB"] = max(res[leg]["peak_alloc_MiB"],
                                             round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2))
    for leg in res:
        res[leg]["ms_per_step_median"] = round(statistics.median(res[leg]["ms_per_step_runs"]), 5)
    print("ROLLOUT_TIMING_CHILD " + json.dumps({"sizes": sizes, "legs": res}), flush=True)


def run_child(tree, legs, args):
    tree = os.path.abspath(tree)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", legs, "--root", tree, "--workload", args.workload,
           "--steps", str(args.steps), "--runs", str(args.runs), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=args.child_timeout)
    for line in p.stdout.splitlines():
        if line.startswith("ROLLOUT_TIMING_CHILD "):
            return json.loads(line[len("ROLLOUT_TIMING_CHILD "):])
    raise RuntimeError(f"child {legs} in {tree} failed (rc {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cavity")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-tree", default=None, help="an exported and built checkout of the parent commit (leg a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_timing.json"))
    ap.add_argument("--child", default=None, help="(internal) comma-separated legs to run in this process")
    ap.add_argument("--root", default=None, help="(internal) the tree the child imports")
    ap.add_argument("--child-timeout", type=float, default=900.0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"workload": args.workload, "steps_per_window": args.steps, "windows": args.runs, "warmup_steps": args.warmup, "legs": {}}
    first = run_child(args.parent_tree, "a", args) if args.parent_tree else None
    mine = run_child(ROOT, "b,c,d", args)
    second = run_child(args.parent_tree, "a", args) if args.parent_tree else None
    out["sizes"] = mine["sizes"]
    out["legs"].update(mine["legs"])
    if first is not None:
        runs = first["legs"]["a"]["ms_per_step_runs"] + second["legs"]["a"]["ms_per_step_runs"]
        out["legs"]["a"] = {"ms_per_step_runs": runs, "ms_per_step_median": round(statistics.median(runs), 5),
                            "a_first_median": first["legs"]["a"]["ms_per_step_median"],
                            "a_second_median": second["legs"]["a"]["ms_per_step_median"],
                            "peak_alloc_MiB": max(first["legs"]["a"]["peak_alloc_MiB"], second["legs"]["a"]["peak_alloc_MiB"])}
        ta = out["legs"]["a"]["ms_per_step_median"]
        out["ratio_to_a"] = {leg: round(out["legs"][leg]["ms_per_step_median"] / ta, 4) for leg in ("b", "c", "d")}
    else:
        out["legs"]["a"] = "not measured (no --parent-tree)"
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
