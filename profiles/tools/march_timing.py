#!/usr/bin/env python3
"""What the march launch costs: ms per inner iteration of `MarchStep` with a fixed count (tol off,
min_inner = max_inner = 20, list mode) against `TrainStep.step()` x 20 + `advance_time()` (list mode; the launches of the parent
commit's TrainStep - `_after_backward()` issues nothing there), and the march launch on its own.

    python profiles/tools/march_timing.py --mesh poly|real_cylinder [--runs 7] [--levels 5] [--out FILE]

prints ONE JSON line and merges it into --out (default profiles/march_timing.json) under the mesh's name.
A run: fresh models from one seed, two levels of warm-up per leg (the lists are recorded there), then blocks of `--levels` levels
(20 inner iterations each), the two legs ALTERNATING block by block; ms_per_inner = host wall time of a block (ending in one
device synchronise) over its inner iterations; median, min and max over the blocks.  The launch alone: 200 back-to-back
`gfv_march_advance` on buffers of the mesh's size between two device events, us per launch - once with a record that never
latches, once with max_inner = 1 (every launch latches: write-back, restore, two norms, a history row), with and without a
snapshot ring."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "march_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import cases
    from FVMmodel.importer import NNmodel
    from gfv import lib as L
    from gfv.march import MarchStep, _f2w
    from gfv.params import default_params
    from gfv.trainer import TrainStep
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
    ms = MarchStep(model(), graphs(), use_graph="list", tol=-1, abs_tol=-1, min_inner=INNER, max_inner=INNER,
                   max_levels=(blocks + 1) * args.levels + 2)
    ts = TrainStep(model(), graphs(), use_graph="list")

    def march_block(levels):
        ms.run(levels=levels, max_ahead=64)             # (ends in its one synchronisation)

    def train_block(levels):
        for _ in range(levels):
            for _ in range(INNER):
                ts.step()
            ts.advance_time()
        torch.cuda.synchronize()

    legs = {"march": march_block, "trainstep": train_block}
    for fn in legs.values():
        fn(2)
    times = {k: [] for k in legs}
    for _ in range(blocks):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.levels)
            times[name].append(1e3 * (time.perf_counter() - t0) / (args.levels * INNER))
    st = ms.stats()
    assert st["held"] == 0 and st["seen"] == (2 + blocks * args.levels) * INNER, st
    out = {"mesh": args.mesh, "nodes": int(ms.plan.N), "graphs": int(ms.plan.B), "chunks": int(ms.plan.n_chunks),
           "inner_per_level": INNER, "levels_per_block": args.levels, "blocks": blocks, "ms_per_inner": {}}
    for name, v in times.items():
        out["ms_per_inner"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["march_minus_trainstep_us"] = round(1e3 * (out["ms_per_inner"]["march"]["median"]
                                                   - out["ms_per_inner"]["trainstep"]["median"]), 2)

    # ---- the launch alone ----------------------------------------------------------------------------------------------------
    pl, dev, lib = ms.plan, ms.dev, L.load()
    n_launch = LAUNCH_BLOCK + 20
    uvp = ms.uvp_node.clone()
    xb, x = ms.x_backup.clone(), ms.x.clone()
    losses = ms.losses.clone()
    partial = torch.zeros((pl.n_chunks, 2), dtype=torch.float64, device=dev)
    r0 = torch.zeros(pl.B, dtype=torch.float32, device=dev)
    hist = torch.zeros((n_launch, L.MARCH_HEAD + L.MARCH_GRAPH * pl.B), dtype=torch.int32, device=dev)
    snap = torch.zeros((2, pl.N, 3), dtype=torch.float32, device=dev)
    out["launch_us"] = {}
    for name, max_inner, keep in (("no_latch", 1 << 30, 0), ("latch", 1, 0), ("latch_keep2", 1, 2)):
        rec = torch.zeros(L.MARCH_RECORD, dtype=torch.int32)
        rec[0], rec[1], rec[4], rec[5], rec[8], rec[12] = max_inner, 1, _f2w(-1.0), _f2w(-1.0), n_launch, keep
        rec = rec.to(dev)

        def launch():
            L.check(lib.gfv_march_advance(
                uvp.data_ptr(), xb.data_ptr(), x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(),
                pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, losses.data_ptr(), partial.data_ptr(), ms.hyper.data_ptr(),
                rec.data_ptr(), r0.data_ptr(), hist.data_ptr(), n_launch, max_inner, 1, snap.data_ptr() if keep else None, keep,
                None, L.stream_ptr()), "gfv_march_advance")
        for _ in range(20):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCH_BLOCK):
            launch()
        e1.record()
        torch.cuda.synchronize()
        words = rec.cpu()
        assert int(words[11]) == 0 and int(words[10]) == n_launch and int(words[6]) == (n_launch if max_inner == 1 else 0), words
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
