#!/usr/bin/env python3
"""What an evaluation pass over a device pool costs per batch, three ways, on two pools:

  variants15k   16 variants of one ~15 k-cell cylinder mesh, max_graphs=8   (2 batches per pass)
  entries50k    16 entries of ~50 k cells each, max_graphs=1                (16 batches per pass)

Both pools are variants of ONE mesh, so every batch of a pool has one size signature: list mode records once and replays every
other batch - the friendliest case for it.  A pool of distinct meshes pays two eager batches and a recording per signature first.

  list    gfv.evaluate.Evaluate(launch_mode="cmd_list"): recorded body replayed, the collect launch behind it, one synchronisation
          per pass
  eager   gfv.evaluate.Evaluate(launch_mode="eager"): the same launches issued one by one
  loop    what Evaluate replaces: per batch `pool.batch(idx)`, a new `Rollout(model, graphs)`, `step()`, `losses.cpu()`

`--warmup` passes of each way first (list mode: two eager batches per signature, the recording, first replays), then `--blocks`
timed blocks per way of `--passes` passes each, the ways ALTERNATING block by block; ms_per_batch = host wall time of a block
(every pass ends in a device synchronise) over its batches.  Reported per way: the median over the blocks and the spread
(min, max).  No threshold: the figures are what they are.

    python profiles/tools/eval_timing.py [--cases variants15k,entries50k] [--blocks 5] [--passes 5] [--warmup 3] [--out FILE]

prints ONE JSON line and (--out, default profiles/eval_timing.json) writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

CASES = {"variants15k": dict(cells=15000, max_graphs=8), "entries50k": dict(cells=50000, max_graphs=1)}
N_ENTRIES = 16
WAYS = ("list", "eager", "loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="variants15k,entries50k")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_timing.json"))
    args = ap.parse_args()
    import torch
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.evaluate import Evaluate, split_batches
    from gfv.params import default_params
    from gfv.pool import DevicePool
    from gfv.rollout import Rollout
    from FVMmodel.importer import NNmodel
    from oracle import fvgn_oracle as O
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    model = NNmodel(default_params(dataset_size=1))
    sd = model.state_dict()
    for k, v in O.init_parameters(0).items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    model = model.to(dev)
    out = {"entries": N_ENTRIES, "blocks": args.blocks, "passes_per_block": args.passes, "cases": {}}
    for case in (c for c in args.cases.split(",") if c):
        cfg = CASES[case]
        nx, ny = meshgen.cylinder_grid_for_cells(cfg["cells"])
        mesh = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234), U=0.15, device=dev)
        pool = DevicePool([mesh], [meshgen.random_fields(mesh, seed=1)], device=dev)
        for j in range(N_ENTRIES - 1):
            pool.add_variant(0, fields=meshgen.random_fields(mesh, seed=2 + j), U=0.10 + 0.01 * j, mu=1e-3 * (1 + 0.1 * j))
        idx = list(range(N_ENTRIES))
        batches = split_batches(idx, cfg["max_graphs"])
        ev = {"list": Evaluate(model, pool, max_graphs=cfg["max_graphs"]),
              "eager": Evaluate(model, pool, max_graphs=cfg["max_graphs"], launch_mode="eager")}

        def one_pass(way):
            if way != "loop":
                return ev[way].run(idx).losses
            rows = []
            for b in batches:
                graphs, _ = pool.batch(b)
                rows.append(Rollout(model, graphs).step()[0].cpu())
            return torch.cat(rows)

        for way in WAYS:
            for _ in range(args.warmup):
                last = one_pass(way)
            if way == "list":
                ref = last
            assert torch.equal(last, ref), f"{case}: the {way} pass does not give the bits of the list pass"
        torch.cuda.synchronize()
        ms = {way: [] for way in WAYS}
        for _ in range(args.blocks):
            for way in WAYS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.passes):
                    one_pass(way)
                torch.cuda.synchronize()
                ms[way].append(1e3 * (time.perf_counter() - t0) / (args.passes * len(batches)))
        res = {"cells_per_entry": int(pool.sizes[0]["c"]), "nodes_per_entry": int(pool.sizes[0]["n"]), "max_graphs": cfg["max_graphs"],
               "batches_per_pass": len(batches), "stats_list": ev["list"].stats(), "ms_per_batch": {}}
        for way in WAYS:
            res["ms_per_batch"][way] = {"median": round(statistics.median(ms[way]), 4), "min": round(min(ms[way]), 4),
                                        "max": round(max(ms[way]), 4)}
        out["cases"][case] = res
        del ev, pool
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
