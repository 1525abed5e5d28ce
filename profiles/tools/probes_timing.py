#!/usr/bin/env python3
"""What the probe launch costs: steps per second of a list-mode `Rollout` in three legs -
  plain     neither (`probes=None`, `wall_forces=None`: the launches of the parent commit)
  forces    wall forces that sample every step (two launches: a pivoted LU per body node, then the sums)
  probes    64 probes that sample every step (one launch: a sparse dot product per probe) - a wake rake of 32, a centreline rake of
            24 and 8 points around the cylinder
- and the probe launch on its own.  The tool asserts that the three legs' fields, node states and histories have the same bits.

    python profiles/tools/probes_timing.py --mesh cyl_b3|cylinder50k [--blocks 7] [--steps 100] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/probes_timing.json) under the mesh's name.
A run: fresh models from one seed, two warm-up blocks per leg (the lists are recorded there), then `--blocks` blocks of `--steps`
steps, the three legs ALTERNATING block by block; every block starts from the initial state (`reset()`, outside the timed region),
so the three legs compute the same `--steps` steps every time.  ms_per_step = host wall time of a block (ending in one device
synchronise) over its steps; median, min and max over the blocks, steps per second from the medians.  The launch alone: 200
back-to-back launches between two device events on a record that samples every time (each launch is handed the next word of a row
of ascending clock values), us per launch."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LAUNCH_BLOCK = 200
BOX, ORIGIN = (0.05, 0.35, 0.08, 0.32), (0.2, 0.2)      # the cylinder of the generated channel meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="cylinder50k", choices=("cyl_b3", "cylinder50k"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import cases
    from FVMmodel.importer import NNmodel
    from gfv import lib as L
    from gfv import probes as PR
    from gfv.params import default_params
    from gfv.rollout import Rollout
    from gfv.wallforce import WallForces
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    if args.mesh == "cyl_b3":
        cpu_graphs = cases.make_graphs("cyl_b3")
    else:
        from gfv import meshgen
        from gfv.graph import build_batch
        nx, ny = meshgen.cylinder_grid_for_cells(50000)
        m = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234))
        cpu_graphs = build_batch([m], [meshgen.random_fields(m, seed=1234 + 7)])
    points = torch.cat((PR.line((0.3, 0.05), (0.3, 0.36), 32), PR.line((0.32, 0.2), (2.0, 0.2), 24),
                        torch.tensor([[0.12, 0.2], [0.2, 0.29], [0.2, 0.11], [0.28, 0.2], [0.1, 0.3], [0.1, 0.1], [1.0, 0.3], [1.0, 0.1]],
                                     dtype=torch.float64)))
    assert tuple(points.shape) == (64, 2)

    def graphs():
        hg = tuple(g.clone().to("cuda") for g in cpu_graphs)
        hg[0].norm_uvp, hg[0].norm_global = True, True
        return hg

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    wf, pr = WallForces(box=BOX, origin=ORIGIN, keep=args.steps), PR.Probes(points, graph=0, keep=args.steps)
    legs = {"plain": Rollout(model(), graphs(), max_steps=args.steps),
            "forces": Rollout(model(), graphs(), max_steps=args.steps, wall_forces=wf)}
    t1 = time.perf_counter()
    legs["probes"] = Rollout(model(), graphs(), max_steps=args.steps, probes=pr)
    attach_s = time.perf_counter() - t1

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
    for what in ("history", "x_backup", "x"):
        ref = getattr(legs["plain"], what).cpu().view(torch.int32)
        for k in ("forces", "probes"):
            assert torch.equal(getattr(legs[k], what).cpu().view(torch.int32), ref), f"the {k} leg's {what} differs"
    assert pr.count() == args.steps and wf.count() == args.steps
    assert all(r._lists.stats()["recorded"] == 1 for r in legs.values())
    pl, t = legs["plain"].plan, pr.tables
    out = {"mesh": args.mesh, "nodes": int(pl.N), "cells": int(pl.C), "graphs": int(pl.B), "probes": pr.P, "entries": t.nnz,
           "entries_per_probe_max": int((t.pw_ptr[1:] - t.pw_ptr[:-1]).max()), "body_nodes": wf.tables.Nb, "terms": int(pl.M),
           "attach_s": round(attach_s, 3), "steps_per_block": args.steps, "blocks": args.blocks, "ms_per_step": {}, "steps_per_s": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["steps_per_s"][name] = round(1e3 / statistics.median(v), 1)
    med = lambda k: out["ms_per_step"][k]["median"]
    out["forces_minus_plain_us"] = round(1e3 * (med("forces") - med("plain")), 2)
    out["probes_minus_plain_us"] = round(1e3 * (med("probes") - med("plain")), 2)

    # ---- the launch alone ---------------------------------------------------------------------------------------------------
    lib = L.load()
    xb = legs["plain"].x_backup.clone()
    n_launch = LAUNCH_BLOCK + 20
    clocks = torch.arange(1, n_launch + 1, dtype=torch.int32, device=legs["plain"].dev)
    lone = PR.Probes(points, graph=0, keep=16).attach("probes_timing", graphs(), pl, xb, clocks)
    lt = lone.tables

    def sample(i):
        L.check(lib.gfv_probe_sample(xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.batch.data_ptr(), lt.pw_ptr.data_ptr(),
                                     lt.pw_node.data_ptr(), lt.pw_w.data_ptr(), lone.P, clocks.data_ptr() + 4 * i, lone.rec.data_ptr(),
                                     lone.hist.data_ptr(), lone.hist_clock.data_ptr(), lone.keep, L.stream_ptr()), "gfv_probe_sample")

    for i in range(20):
        sample(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(20, n_launch):
        sample(i)
    e1.record()
    torch.cuda.synchronize()
    out["launch_us"] = {"sample": round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)}
    assert lone.count() == n_launch
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
