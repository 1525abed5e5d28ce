#!/usr/bin/env python3
"""What the unsteady-boundary-data launch costs: ms per step of a list-mode `Rollout` in three legs -
  plain   no boundary data (`time_bc=None`: the launches of the parent commit)
  const   TimeBC(velocity=Const(1), source=Const(1)): the launch writes the base values back (the tool asserts that this leg's
          history has the bits of the plain leg's)
  sine    TimeBC(velocity=Sine, source=Sine): every row evaluates a double-precision sin
- and the launch on its own.

    python profiles/tools/timebc_timing.py --mesh poly|real_cylinder|cylinder50k [--blocks 7] [--steps 100] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/timebc_timing.json) under the mesh's name.
A run: fresh models from one seed, two warm-up blocks per leg (the lists are recorded there), then `--blocks` blocks of `--steps`
steps, the three legs ALTERNATING block by block; every block starts from the initial state (`reset()`, outside the timed region).
ms_per_step = host wall time of a block (ending in one device synchronise) over its steps; median, min and max over the blocks, and
the differences of the medians.  The launch alone: 200 back-to-back `TimeBC.launch()` of the const and the sine leg's objects
between two device events, us per launch (the issue path of an eager ctypes call included).  Under `rocprofv3 --kernel-trace
--stats -- python ...` the kernel's own duration is the row `time_bc_kernel` of the statistics."""
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
    ap.add_argument("--mesh", default="poly", choices=("poly", "real_cylinder", "cylinder50k"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timebc_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import cases
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    from gfv.rollout import Rollout
    from gfv.timebc import Const, Sine, TimeBC
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    if args.mesh == "poly":
        from test_config5_gpu import _small_polygon_graphs
        cpu_graphs = _small_polygon_graphs()
    elif args.mesh == "real_cylinder":
        cpu_graphs = cases.real_cylinder(os.path.join(ROOT, "tests", "golden"))[0]
    else:
        from gfv import meshgen
        from gfv.graph import build_batch
        nx, ny = meshgen.cylinder_grid_for_cells(50000)
        m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234))
        cpu_graphs = build_batch([m], [meshgen.random_fields(m, seed=1234 + 7)])

    def graphs():
        hg = tuple(g.clone().to("cuda") for g in cpu_graphs)
        hg[0].norm_uvp, hg[0].norm_global = True, True
        return hg

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    bcs = {"plain": None, "const": TimeBC(velocity=Const(1.0), source=Const(1.0)),
           "sine": TimeBC(velocity=Sine(1.0, 0.3, 0.2), source=Sine(1.0, 0.5, 0.1, phase=0.3))}
    legs = {k: Rollout(model(), graphs(), max_steps=args.steps, time_bc=bc) for k, bc in bcs.items()}

    def block(r):
        for _ in range(args.steps):
            r.step()
        torch.cuda.synchronize()

    for r in legs.values():
        block(r)
        r.reset()
        block(r)
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, r in legs.items():
            r.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block(r)
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    hist = {k: r.history.cpu() for k, r in legs.items()}
    assert torch.equal(hist["const"].view(torch.int32), hist["plain"].view(torch.int32)), "the const leg's history differs"
    assert all(r._lists.stats()["recorded"] == 1 for r in legs.values())
    assert bcs["sine"].read()["clock"].tolist() == list(range(1, args.steps + 2))
    pl = legs["plain"].plan
    nt = pl.node_type.cpu()
    out = {"mesh": args.mesh, "nodes": int(pl.N), "graphs": int(pl.B), "masked_rows": int(((nt == 1) | (nt == 5)).sum()),
           "steps_per_block": args.steps, "blocks": args.blocks, "ms_per_step": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    med = lambda k: out["ms_per_step"][k]["median"]
    out["const_minus_plain_us"] = round(1e3 * (med("const") - med("plain")), 2)
    out["sine_minus_plain_us"] = round(1e3 * (med("sine") - med("plain")), 2)

    # ---- the launch alone ----------------------------------------------------------------------------------------------------
    out["launch_us"] = {}
    for name in ("const", "sine"):
        bc = bcs[name]
        for _ in range(20):
            bc.launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            bc.launch()
        e1.record()
        torch.cuda.synchronize()
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
