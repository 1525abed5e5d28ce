#!/usr/bin/env python3
"""What the adaptive step's two launches cost: a short march with a fixed-step "bdf2" scheme and the same march
with `adapt=StepControl(...)`, one after the other in one process.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python profiles/tools/stepcontrol_timing.py --mesh poly|cylinder50k

The kernels' own durations are the rows `time_scheme_kernel` (the fixed-step leg: one dispatch per step), `step_rate_kernel` and
`step_rows_kernel` (the adaptive leg: one dispatch each per step) of the statistics.  Each leg: a fresh model from one seed,
`MarchStep(..., use_graph="list", tol=None, max_inner=--inner)`, `run(levels=--levels)`.  Prints ONE JSON line: the mesh, the
dispatches to expect per kernel, host wall time per leg and the adaptive leg's step history."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="poly", choices=("poly", "cylinder50k"))
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    from FVMmodel.importer import NNmodel
    from gfv.march import MarchStep
    from gfv.params import default_params
    from gfv.timescheme import StepControl, TimeScheme
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
    out = {"mesh": args.mesh, "levels": args.levels, "inner": args.inner, "wall_s": {}}
    schemes = {"fixed": TimeScheme("bdf2"), "adaptive": TimeScheme("bdf2", adapt=StepControl(courant=2.0, grow=1.5, shrink=0.5))}
    for name, sch in schemes.items():
        torch.manual_seed(0)
        model = NNmodel(default_params(dataset_size=1)).cuda()
        graphs = tuple(g.clone().to("cuda") for g in cpu_graphs)
        ms = MarchStep(model, graphs, lr=5e-5, use_graph="list", tol=None, max_inner=args.inner, max_levels=args.levels,
                       time_scheme=sch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms.run(levels=args.levels)
        out["wall_s"][name] = round(time.perf_counter() - t0, 4)
        out.update(nodes=int(ms.plan.N), cells=int(ms.plan.C), graphs=int(ms.plan.B))
    # (attach issues each leg's launch once, every step once more)
    out["dispatches_per_kernel"] = 1 + args.levels * args.inner
    out["history"] = [{"clock": r["clock"], "dt": r["dt"].tolist(), "courant": r["courant"].tolist()}
                      for r in schemes["adaptive"].step_history()]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
