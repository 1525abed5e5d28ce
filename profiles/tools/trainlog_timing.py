#!/usr/bin/env python3
"""What the training log costs per step: PoolTrainStep(max_graphs=1) over eight variants of one mesh - every step a
replay of the one recorded list, a different entry every step - with `log=None` and with `log=4096`, and the two log launches on
their own.

    python profiles/tools/trainlog_timing.py --mesh cavity|cyl50k [--legs none,log,launches] [--root TREE] [--label NAME]

prints ONE JSON line and (--out, default profiles/trainlog_timing.json) merges it into that file under `--label` (default the
mesh).  `--root`: measure the package of ANOTHER checkout of this repository (the parent commit, which has leg `none` only) with
this one tool, so that both sides of the comparison are timed by the same code.
A run: fresh models from one seed, `--warmup` steps per leg, then `--steps` timed ones in blocks of 50, the legs ALTERNATING block
by block; ms_per_step = host wall time of a leg's blocks (each ending in one device synchronise) over its steps.  Leg `launches`:
blocks of 200 back-to-back appends (norms + append) on the log of leg `log` between two device events, us per pair, and the same
for the norms launch alone."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BLOCK, LAUNCH_BLOCK = 50, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="cavity", choices=("cavity", "cyl50k"))
    ap.add_argument("--legs", default="none,log,launches")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainlog_timing.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (root, os.path.join(root, "gen-fvgn-steady_amd")):
        sys.path.insert(0, p)
    import torch
    from FVMmodel.importer import NNmodel
    from gfv import host as gfv_host
    from gfv import meshgen
    from gfv.params import default_params
    from gfv.pool import DevicePool
    from gfv.pool_trainer import PoolTrainStep
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    legs = [x for x in args.legs.split(",") if x]
    assert set(legs) <= {"none", "log", "launches"}, legs
    assert "launches" not in legs or "log" in legs, "leg `launches` times the log object of leg `log`"

    if args.mesh == "cavity":
        raw = meshgen.raw_quad_cavity(n=71, jitter=0.0, seed=1234)                  # the 5 041-cell cavity of bench.py
    else:
        nx, ny = meshgen.cylinder_grid_for_cells(50000)
        raw = meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, jitter=0.2, seed=1234)
    m = meshgen.finish_mesh(raw, device="cuda")

    def make_pool():
        pool = DevicePool([m], [meshgen.random_fields(m, seed=1)])
        for j in range(7):
            pool.add_variant(0, fields=meshgen.random_fields(m, seed=100 + j), U=0.1 + 0.01 * j, mu=1e-3 * (1 + j % 5))
        return pool

    def model():
        torch.manual_seed(0)
        return NNmodel(default_params(dataset_size=1)).cuda()

    step_legs = [leg for leg in legs if leg != "launches"]
    out = {"mesh": args.mesh, "root_is_this_tree": root == ROOT, "steps_per_leg": args.steps, "legs": {leg: {"runs": []} for leg in legs}}
    for _ in range(args.runs):
        G = {}
        for leg in step_legs:
            ts = PoolTrainStep(model(), make_pool(), max_graphs=1, want_outputs=False, **(dict(log=4096) if leg == "log" else {}))
            for k in range(args.warmup):
                ts.step([k % 8])
            torch.cuda.synchronize()
            G[leg] = dict(ts=ts, wall=0.0, steps=0)
        out["cells"] = int(G[step_legs[0]]["ts"].pool.sizes[0]["c"])
        out["n_params"] = int(G[step_legs[0]]["ts"].n_params)
        while any(G[leg]["steps"] < args.steps for leg in step_legs):
            for leg in step_legs:
                g = G[leg]
                if g["steps"] >= args.steps:
                    continue
                ts = g["ts"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(BLOCK):
                    ts.step([(g["steps"] + k) % 8])
                torch.cuda.synchronize()
                g["wall"] += time.perf_counter() - t0
                g["steps"] += BLOCK
        for leg in step_legs:
            g = G[leg]
            out["legs"][leg]["runs"].append({"ms_per_step": round(1e3 * g["wall"] / g["steps"], 4), "stats": g["ts"].stats()})
        if "launches" in legs:
            ts = G["log"]["ts"]
            lg = ts.log
            from gfv import lib as L
            lib, res = L.load(), {}

            def pair():
                ts._log_step([0], ts.pool.n)

            def norms():
                L.check(lib.gfv_train_log_norms(ts.flat_g.data_ptr(), ts.flat_p.data_ptr(), lg.segs.data_ptr(), lg.bucket_tab.data_ptr(),
                                                lg.K, lg.n_chunks, lg.sums.data_ptr(), lg.ws.data_ptr(), L.stream_ptr()), "norms")
            for name, fn in (("pair_us", pair), ("norms_us", norms)):
                for _ in range(20):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(LAUNCH_BLOCK):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name] = round(1e3 * e0.elapsed_time(e1) / LAUNCH_BLOCK, 3)
            res["append_us"] = round(res["pair_us"] - res["norms_us"], 3)
            out["legs"]["launches"]["runs"].append(res)
        del G
        torch.cuda.empty_cache()
    for leg in step_legs:
        vals = [x["ms_per_step"] for x in out["legs"][leg]["runs"]]
        out["legs"][leg]["ms_per_step_median"] = round(statistics.median(vals), 4)
        out["legs"][leg]["ms_per_step_spread"] = round(max(vals) - min(vals), 4)
    if "launches" in legs:
        for key in ("pair_us", "norms_us", "append_us"):
            vals = [x[key] for x in out["legs"]["launches"]["runs"]]
            out["legs"]["launches"][key + "_median"] = round(statistics.median(vals), 3)
            out["legs"]["launches"][key + "_spread"] = round(max(vals) - min(vals), 3)
    if "none" in step_legs and "log" in step_legs:
        out["log_minus_none_us_per_step"] = round(1e3 * (out["legs"]["log"]["ms_per_step_median"]
                                                         - out["legs"]["none"]["ms_per_step_median"]), 2)
    print(json.dumps(out))
    if args.out:
        try:
            with open(args.out) as f:
                allw = json.load(f)
        except (OSError, ValueError):
            allw = {}
        allw[args.label or args.mesh] = out
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allw, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
