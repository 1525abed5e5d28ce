#!/usr/bin/env python3
"""What Anderson acceleration per slot costs per step of a `gfv.sweep.Sweep` (cost table).  No pass / fail.

ms per step of a Sweep in command-list mode with anderson = 0 and anderson = `--depth` in ONE process, on a pool of `--slots`
variants of the 5 041-cell cavity mesh and of the 50 020-cell cylinder mesh, `max_graphs = --slots`, `tol = -1` (nothing latches:
every slot is live in every timed step).  The step is `Sweep._step` on the batch of all slots, set up as `Sweep.run` sets it up.
Per leg `--warmup` steps (warm-up, recording, first replays); then blocks that ALTERNATE between the legs: the pool's fields
restored and loaded, the slots and the acceleration's state zeroed, 8 untimed steps (the ring fills), a synchronise, `--block`
timed steps, a synchronise.  Reported: median and min / max over the blocks of a leg, their difference, and the share of the
block's steps that WERE accelerated (from the per-slot counts).

    python profiles/tools/sweep_anderson_timing.py [--workloads cavity,50k] [--slots 8] [--depth 5] [--blocks 7] [--block 20]

prints ONE JSON line and (--out, default profiles/sweep_anderson_timing.json) writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FILL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cavity,50k")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_anderson_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    from FVMmodel.importer import NNmodel
    from gfv import anderson as AA
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.params import default_params
    from gfv.pool import DevicePool
    from gfv.sweep import Sweep
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()

    def mesh_of(name):
        if name == "cavity":
            return meshgen.finish_mesh(meshgen.raw_quad_cavity(n=71, jitter=0.0, tri_fraction=0.0, seed=1234), U=1.0)
        nx, ny = meshgen.cylinder_grid_for_cells(50000)
        return meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234), U=0.15)

    def new_model():
        model = NNmodel(default_params(dataset_size=1))      # a trained model: the Normalizer no longer accumulates
        sd = model.state_dict()
        for k, v in O.init_parameters(0).items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        return model.cuda()

    class Leg:
        def __init__(self, mesh, m):
            self.pool = DevicePool([mesh], [meshgen.random_fields(mesh, seed=5)])
            for j in range(args.slots - 1):
                self.pool.add_variant(0, fields=meshgen.random_fields(mesh, seed=11 + j), U=0.12 + 0.01 * j, mu=1e-3 * (1 + j),
                                      dt=0.01 * (2 + j))
            self.x0 = [x.clone() for x in self.pool.x]
            self.sw = Sweep(new_model(), self.pool, max_graphs=args.slots, tol=-1, max_steps=2 ** 30, anderson=m)
            self.cur = list(range(args.slots))
            self.sw._write_ctl()
            self.arm()

        def arm(self):
            sw = self.sw
            for x, x0 in zip(self.pool.x, self.x0):
                x.copy_(x0)
            sw._slots.zero_()
            sw._last.zero_()
            if sw._aa is not None:
                sw._aa.reset()
            graphs, pl = sw.arena.load(self.cur)
            self.step_args = (sw.arena.signature(self.cur), graphs, pl)

        def steps(self, n):
            for _ in range(n):
                self.sw._step(*self.step_args)

    out = {"depth": args.depth, "slots": args.slots, "block_steps": args.block, "blocks_per_leg": args.blocks, "cost": {}}
    for name in (w for w in args.workloads.split(",") if w):
        mesh = mesh_of(name)
        print(f"{name}: mesh built", file=sys.stderr, flush=True)
        legs = {m: Leg(mesh, m) for m in (0, args.depth)}
        for leg in legs.values():
            leg.steps(args.warmup)
        torch.cuda.synchronize()
        print(f"{name}: both legs warmed up", file=sys.stderr, flush=True)
        ms = {m: [] for m in legs}
        share = []
        for _ in range(args.blocks):
            for m, leg in legs.items():
                leg.arm()
                leg.steps(FILL)
                torch.cuda.synchronize()
                before = leg.sw._aa.aa_count[:, 0].sum().item() if m else 0
                t0 = time.perf_counter()
                leg.steps(args.block)
                torch.cuda.synchronize()
                ms[m].append(1e3 * (time.perf_counter() - t0) / args.block)
                if m:
                    share.append((leg.sw._aa.aa_count[:, 0].sum().item() - before) / (args.block * args.slots))
        sizes = legs[0].pool.sizes[0]
        res = {"cells": int(sizes["c"]), "nodes_per_entry": int(sizes["n"]), "nodes_per_step": int(sizes["n"]) * args.slots,
               "lists": {m: leg.sw.stats()["lists"] for m, leg in legs.items()}}
        for m in legs:
            res[f"anderson_{m}"] = {"ms_per_step_median": round(statistics.median(ms[m]), 5),
                                    "ms_per_step_min": round(min(ms[m]), 5), "ms_per_step_max": round(max(ms[m]), 5)}
        res["on_minus_off_us"] = round(1e3 * (statistics.median(ms[args.depth]) - statistics.median(ms[0])), 2)
        res["share_of_timed_steps_accelerated"] = round(statistics.mean(share), 3)
        res["ring_bytes"] = AA.ring_bytes(args.slots, sizes["n"], args.depth)
        out["cost"][name] = res
        del legs
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
