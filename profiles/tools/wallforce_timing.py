#!/usr/bin/env python3
"""What the wall-force pair costs: steps per second of a list-mode `Rollout` in three legs -
  plain     neither (`wall_forces=None`, `field_stats=None`: the launches of the parent commit; the tool asserts that its history
            has the bits of the other two legs')
  stats     field statistics that sample every step (one launch over all N rows)
  forces    wall forces that sample every step (two launches over the body's nodes and faces)
- and each launch of the pair on its own.

    python profiles/tools/wallforce_timing.py --mesh cyl_b3|real_cylinder|cylinder50k [--blocks 7] [--steps 100] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/wallforce_timing.json) under the mesh's name.
A run: fresh models from one seed, two warm-up blocks per leg (the lists are recorded there), then `--blocks` blocks of `--steps`
steps, the three legs ALTERNATING block by block; every block starts from the initial state (`reset()`, outside the timed region),
so the three legs compute the same `--steps` steps every time.  ms_per_step = host wall time of a block (ending in one device
synchronise) over its steps; median, min and max over the blocks, steps per second from the medians.  The launches alone: 200
back-to-back launches of each between two device events on a record that samples every time (each launch is handed the next word
of a row of ascending clock values; the first launch writes no record word, so it is timed on the clock words the second has not
seen yet), us per launch."""
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
    ap.add_argument("--mesh", default="cylinder50k", choices=("cyl_b3", "real_cylinder", "cylinder50k"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wallforce_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import cases
    from FVMmodel.importer import NNmodel
    from gfv import lib as L
    from gfv.fieldstats import FieldStats
    from gfv.params import default_params
    from gfv.rollout import Rollout
    from gfv.wallforce import WallForces
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    box = BOX
    if args.mesh == "cyl_b3":
        cpu_graphs = cases.make_graphs("cyl_b3")
    elif args.mesh == "real_cylinder":
        cpu_graphs, box = cases.real_cylinder(os.path.join(ROOT, "tests", "golden"))[0], None     # (every wall face of the mesh)
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

    wf, fs = WallForces(box=box, origin=ORIGIN, keep=args.steps), FieldStats(start=1)
    legs = {"plain": Rollout(model(), graphs(), max_steps=args.steps),
            "stats": Rollout(model(), graphs(), max_steps=args.steps, field_stats=fs),
            "forces": Rollout(model(), graphs(), max_steps=args.steps, wall_forces=wf)}

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
    for k in ("stats", "forces"):
        assert torch.equal(hist[k].view(torch.int32), hist["plain"].view(torch.int32)), f"the {k} leg's history differs"
    assert fs.count() == args.steps and wf.count() == args.steps
    assert all(r._lists.stats()["recorded"] == 1 for r in legs.values())
    pl, t = legs["plain"].plan, wf.tables
    out = {"mesh": args.mesh, "nodes": int(pl.N), "graphs": int(pl.B), "body_faces": t.faces.tolist(), "body_nodes": t.Nb,
           "terms": int(pl.M), "steps_per_block": args.steps, "blocks": args.blocks, "ms_per_step": {}, "steps_per_s": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["steps_per_s"][name] = round(1e3 / statistics.median(v), 1)
    med = lambda k: out["ms_per_step"][k]["median"]
    out["stats_minus_plain_us"] = round(1e3 * (med("stats") - med("plain")), 2)
    out["forces_minus_plain_us"] = round(1e3 * (med("forces") - med("plain")), 2)

    # ---- the launches alone -------------------------------------------------------------------------------------------------
    lib, dev = L.load(), legs["plain"].dev
    xb = legs["plain"].x_backup.clone()
    n_launch = LAUNCH_BLOCK + 20
    clocks = torch.arange(1, 2 * n_launch + 1, dtype=torch.int32, device=dev)
    lone = WallForces(box=box, origin=ORIGIN, keep=16).attach("wallforce_timing", graphs(), pl, xb, clocks)
    lt = lone.tables

    def grad(i):
        L.check(lib.gfv_wall_force_grad(xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.batch.data_ptr(), pl.x_rowptr.data_ptr(),
                                        pl.x_out.data_ptr(), pl.x_B.data_ptr(), pl.An.data_ptr(), pl.rn.data_ptr(),
                                        lt.bnode.data_ptr(), lt.Nb, int(pl.M), clocks.data_ptr() + 4 * i, lone.rec.data_ptr(),
                                        lone.gb.data_ptr(), L.stream_ptr()), "gfv_wall_force_grad")

    def total(i):
        L.check(lib.gfv_wall_force_sum(xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.theta.data_ptr(), int(pl.theta.shape[1]),
                                       pl.pos.data_ptr(), pl.fpos.data_ptr(), pl.kS.data_ptr(), pl.es.data_ptr(), pl.er.data_ptr(),
                                       lt.wface.data_ptr(), lt.wchunk_beg.data_ptr(), lt.wchunk_end.data_ptr(),
                                       lt.gwchunk_ptr.data_ptr(), lt.n_wchunks, lt.Nf, lt.B, lone.origin.data_ptr(),
                                       lone.gb.data_ptr(), clocks.data_ptr() + 4 * i, lone.rec.data_ptr(), lone.partial.data_ptr(),
                                       lone.hist.data_ptr(), lone.hist_clock.data_ptr(), lone.keep, L.stream_ptr()),
                "gfv_wall_force_sum")

    out["launch_us"] = {}
    for name, fn, first in (("sum", total, 0), ("grad", grad, n_launch)):
        for i in range(20):
            fn(first + i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(20, n_launch):
            fn(first + i)
        e1.record()
        torch.cuda.synchronize()
        out["launch_us"][name] = round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)
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
