#!/usr/bin/env python3
"""What the field-statistics launch costs: ms per step of a list-mode `Rollout` in three legs -
  plain     no statistics (`field_stats=None`: the launches of the parent commit; the tool asserts that its history has the bits of
            the other two legs')
  idle      statistics that never sample (start = 2^30): the launch reads the record and the clock and leaves
  sampling  statistics that sample every step
- and the launch on its own.

    python profiles/tools/fieldstats_timing.py --mesh poly|real_cylinder|cylinder50k [--blocks 7] [--steps 100] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/fieldstats_timing.json) under the mesh's name.
A run: fresh models from one seed, two warm-up blocks per leg (the lists are recorded there), then `--blocks` blocks of `--steps`
steps, the three legs ALTERNATING block by block; every block starts from the initial state (`reset()`, outside the timed region),
so the three legs compute the same `--steps` steps every time.  ms_per_step = host wall time of a block (ending in one device
synchronise) over its steps; median, min and max over the blocks, and the differences of the medians.  The launch alone: 200
back-to-back `gfv_field_stats_update` on buffers of the mesh's size between two device events, us per launch - once with a record
that never samples, once sampling every launch (each launch is handed the next word of a row of ascending clock values - a clock
pointer is what an owner hands in), with bytes over time for the latter."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LAUNCH_BLOCK, NEVER = 200, 1 << 30
BYTES_PER_ROW = 16 + 112 + 48 + 12      # what the entry point prices for a sampling launch (include/gfv.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="poly", choices=("poly", "real_cylinder", "cylinder50k"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldstats_timing.json"))
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

    stats = {"plain": None, "idle": FieldStats(start=NEVER), "sampling": FieldStats(start=1)}
    legs = {k: Rollout(model(), graphs(), max_steps=args.steps, field_stats=fs) for k, fs in stats.items()}

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
    for k in ("idle", "sampling"):
        assert torch.equal(hist[k].view(torch.int32), hist["plain"].view(torch.int32)), f"the {k} leg's history differs"
    assert stats["idle"].count() == 0 and stats["sampling"].count() == args.steps
    assert all(r._lists.stats()["recorded"] == 1 for r in legs.values())
    pl = legs["plain"].plan
    out = {"mesh": args.mesh, "nodes": int(pl.N), "graphs": int(pl.B), "steps_per_block": args.steps, "blocks": args.blocks,
           "ms_per_step": {}}
    for name, v in times.items():
        out["ms_per_step"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    med = lambda k: out["ms_per_step"][k]["median"]
    out["idle_minus_plain_us"] = round(1e3 * (med("idle") - med("plain")), 2)
    out["sampling_minus_plain_us"] = round(1e3 * (med("sampling") - med("plain")), 2)

    # ---- the launch alone ----------------------------------------------------------------------------------------------------
    # never: a record that never samples.  always: start = stride = 1; launch i reads clock word i of a row 1, 2, 3, ...
    lib, dev, N = L.load(), legs["plain"].dev, int(pl.N)
    xb = legs["plain"].x_backup.clone()
    n_launch = LAUNCH_BLOCK + 20
    clocks = torch.arange(1, n_launch + 1, dtype=torch.int32, device=dev)
    out["launch_us"] = {}
    for name, start in (("never", NEVER), ("always", 1)):
        rec = torch.tensor([start, 1, -1, -1, 0, 0, 1, 0], dtype=torch.int32).to(dev)
        sums = torch.zeros((L.FIELD_STATS_SUMS, N), dtype=torch.float64, device=dev)
        aux = torch.zeros((L.FIELD_STATS_AUX, N), dtype=torch.float32, device=dev)

        def launch(i):
            L.check(lib.gfv_field_stats_update(xb.data_ptr(), N, clocks.data_ptr() + 4 * i, rec.data_ptr(), sums.data_ptr(),
                                               aux.data_ptr(), L.stream_ptr()), "gfv_field_stats_update")
        for i in range(20):
            launch(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(20, n_launch):
            launch(i)
        e1.record()
        torch.cuda.synchronize()
        words = rec.cpu().tolist()
        assert words[3] == n_launch and words[4] == (n_launch if start == 1 else 0) and words[5] == 0, words
        us = 1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK
        out["launch_us"][name] = round(us, 3)
        if start == 1:
            out["launch_always_gb_per_s"] = round(BYTES_PER_ROW * N / (us * 1e-6) / 1e9, 2)
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
