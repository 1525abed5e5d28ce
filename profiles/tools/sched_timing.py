#!/usr/bin/env python3
"""What the schedule's FOLLOW launch costs a march: ms per inner iteration of `MarchStep(schedule=StepExp(...))`
against `MarchStep` without a schedule (the parent commit's march: no launch of the schedule's is issued there), both with a fixed
count (tol off, min_inner = max_inner = 20, list mode), and the schedule launch on its own.

    python profiles/tools/sched_timing.py --mesh poly|real_cylinder [--runs 7] [--levels 5] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/sched_timing.json) under the mesh's name.
A run (the method of march_timing.py): fresh models from one seed, two levels of warm-up per leg (the lists are recorded there),
then blocks of `--levels` levels, the two legs ALTERNATING block by block; ms_per_inner = host wall time of a block (ending in
run()'s one synchronisation) over its inner iterations; median, min and max over the blocks.  The launch alone: 200 back-to-back
`gfv_lr_schedule` between two device events, us per launch - FOLLOW with a counter that does not move (no groups, and with 32
group rows) and TICK of the STEPEXP kind inside its decay (one pow per launch)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INNER, LAUNCH_BLOCK = 20, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="poly", choices=("poly", "real_cylinder"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import cases
    from FVMmodel.importer import NNmodel
    from gfv import lib as L
    from gfv.march import MarchStep
    from gfv.params import default_params
    from gfv.schedule import StepExp
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    if args.mesh == "poly":
        from test_config5_gpu import _small_polygon_graphs
        cpu_graphs = _small_polygon_graphs()
    else:
        cpu_graphs = cases.real_cylinder(os.path.join(ROOT, "tests", "golden"))[0]

    def graphs():
        return tuple(g.clone().to("cuda") for g in cpu_graphs)

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    blocks = args.runs
    n_levels = (blocks + 1) * args.levels + 2
    kw = dict(use_graph="list", tol=-1, abs_tol=-1, min_inner=INNER, max_inner=INNER, max_levels=n_levels)
    # the drivers' configuration over the levels of this run: a new rate at every level of its second half
    sched = StepExp(startlr=5e-5, steplr_milestone=int(n_levels * 0.1), steplr_gamma=1, explr_milestone=int(n_levels * 0.5),
                    explr_gamma=1e-1, total_epoch=n_levels, min_lr=1e-6)
    legs = {"scheduled": MarchStep(model(), graphs(), lr=5e-5, schedule=sched, **kw),
            "plain": MarchStep(model(), graphs(), lr=5e-5, **kw)}
    for ms in legs.values():
        ms.run(levels=2, max_ahead=64)
    times = {k: [] for k in legs}
    for _ in range(blocks):
        for name, ms in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms.run(levels=args.levels, max_ahead=64)          # (ends in its one synchronisation)
            times[name].append(1e3 * (time.perf_counter() - t0) / (args.levels * INNER))
    for ms in legs.values():
        st = ms.stats()
        assert st["held"] == 0 and st["seen"] == (2 + blocks * args.levels) * INNER, st
    ms = legs["scheduled"]
    assert sched.epoch == 2 + blocks * args.levels - 1
    out = {"mesh": args.mesh, "nodes": int(ms.plan.N), "graphs": int(ms.plan.B), "inner_per_level": INNER,
           "levels_per_block": args.levels, "blocks": blocks, "ms_per_inner": {}}
    for name, v in times.items():
        out["ms_per_inner"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["scheduled_minus_plain_us"] = round(1e3 * (out["ms_per_inner"]["scheduled"]["median"]
                                                   - out["ms_per_inner"]["plain"]["median"]), 2)

    # ---- the launch alone ----------------------------------------------------------------------------------------------------
    dev, lib = ms.dev, L.load()
    hyper = torch.zeros(8, dtype=torch.float32, device=dev)
    table = torch.zeros((L.MAX_PARAM_GROUPS + 2) * 8, dtype=torch.float32, device=dev)
    scales = torch.ones(L.MAX_PARAM_GROUPS, dtype=torch.float64, device=dev)
    counter = torch.full((1,), 3, dtype=torch.int32, device=dev)
    one = StepExp(startlr=5e-5, steplr_milestone=1, steplr_gamma=1, explr_milestone=2, explr_gamma=1e-1, total_epoch=1000,
                  min_lr=1e-6)
    out["launch_us"] = {}
    for name, mode, n_groups in (("follow", L.SCHED_FOLLOW, 0), ("follow_32_groups", L.SCHED_FOLLOW, L.MAX_PARAM_GROUPS),
                                 ("tick", L.SCHED_TICK, 0)):
        rec = one.pack().to(dev)

        def launch():
            L.check(lib.gfv_lr_schedule(rec.data_ptr(), mode, hyper.data_ptr(), table.data_ptr() if n_groups else None,
                                        scales.data_ptr(), n_groups, None, 0, None, counter.data_ptr(), L.stream_ptr()),
                    "gfv_lr_schedule")
        for _ in range(20):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            launch()
        e1.record()
        torch.cuda.synchronize()
        epoch = int(rec.cpu().view(torch.int32)[1])
        assert epoch == (3 if mode == L.SCHED_FOLLOW else LAUNCH_BLOCK + 20), epoch
        out["launch_us"][name] = round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)
    print(json.dumps(out))
    if args.out:
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[args.mesh] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
