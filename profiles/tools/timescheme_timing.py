#!/usr/bin/env python3
"""What the time scheme's launch costs: the launch on its own, and ms per step of a list-mode `TrainStep` with and
without a scheme.

    python profiles/tools/timescheme_timing.py --mesh poly|cylinder50k [--blocks 5] [--steps 50] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/timescheme_timing.json) under the mesh's name.
The launch alone: 200 back-to-back `TimeScheme.launch()` between two device events, us per launch (the issue path of an eager
ctypes call included), once while the scheme is still first order (clock 0: no ring slot is read) and once at second order (after
one `advance_time()`).  The step: fresh models from one seed, two warm-up blocks per leg (the lists are recorded there), then
`--blocks` blocks of `--steps` steps, the legs - no scheme, "bdf2" at second order - ALTERNATING block by block;
ms_per_step = host wall time of a block (ending in one device synchronise) over its steps; median, min and max over the blocks.
A `TrainStep` step issues no launch of the scheme (`advance_time()` does): the legs differ by `gfv_phi_fwd_ts` in place of
`gfv_phi_fwd` and the addresses of the baseline and the step.  Under `rocprofv3 --kernel-trace --stats -- python ...` the kernel's
own duration is the row `time_scheme_kernel` of the statistics."""
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
    ap.add_argument("--mesh", default="poly", choices=("poly", "cylinder50k"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timescheme_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    from gfv.timescheme import TimeScheme
    from gfv.trainer import TrainStep
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    if args.mesh == "poly":
        from test_config5_gpu import _small_polygon_graphs
        cpu_graphs = _small_polygon_graphs()
    else:
        from gfv import meshgen
        from gfv.graph import build_batch
        nx, ny = meshgen.cylinder_grid_for_cells(50000)
        m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234))
        cpu_graphs = build_batch([m], [meshgen.random_fields(m, seed=1234 + 7)])

    def graphs():
        return tuple(g.clone().to("cuda") for g in cpu_graphs)

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    sch = TimeScheme("bdf2")
    legs = {"plain": TrainStep(model(), graphs(), lr=5e-5, use_graph="list"),
            "bdf2": TrainStep(model(), graphs(), lr=5e-5, use_graph="list", time_scheme=sch)}
    out = {"mesh": args.mesh, "nodes": int(legs["plain"].plan.N), "graphs": int(legs["plain"].plan.B),
           "steps_per_block": args.steps, "blocks": args.blocks, "launch_us": {}, "ms_per_step": {}}

    def launch_us():
        for _ in range(20):
            sch.launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            sch.launch()
        e1.record()
        torch.cuda.synchronize()
        return round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)

    assert sch.read()["order"] == 1
    out["launch_us"]["first_order"] = launch_us()
    for ts in legs.values():
        ts.step()
        ts.advance_time()
    assert sch.read()["order"] == 2
    out["launch_us"]["second_order"] = launch_us()

    def block(ts):
        for _ in range(args.steps):
            ts.step()
        torch.cuda.synchronize()

    for ts in legs.values():
        block(ts)
        block(ts)
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, ts in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block(ts)
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["bdf2_minus_plain_us"] = round(1e3 * (out["ms_per_step"]["bdf2"]["median"] - out["ms_per_step"]["plain"]["median"]), 2)
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
