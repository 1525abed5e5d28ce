#!/usr/bin/env python3
"""What the parameter groups cost in the Adam launch.

The Adam launch alone on flat buffers laid out as the model's parameters are (its tensor shapes, alignment padding included:
1.18 M elements, one run per tensor):

    plain     gfv_adam_step_dev of this tree (the kernel without the tables)
    parent    gfv_adam_step_dev of ANOTHER build of the library - the parent commit's libgfv.so, given with --parent-lib;
              loaded beside this tree's, so both are timed by one process in alternating blocks
    g1        gfv_adam_step_groups_dev, every run in one group
    g3        three groups (encoder / processor / decoder tensors)
    gmax      the runs dealt round-robin over all 32 groups the table has (one group per tensor needs more rows than
              GFV_MAX_PARAM_GROUPS): every pair of neighbouring runs differs, every run change re-reads a row
    gmax_wd   the same with a decoupled weight decay on every group

Device time between two events around `--launches` launches issued back to back, over their number, in blocks that ALTERNATE
between the legs (the buffers are then L2 / Infinity-Cache warm, as they are behind a backward that has just written the
gradient); the first block of every leg is dropped, the median of the rest is the figure; `--runs` repeats of all that, median
and spread over them.  lr = 0: the timed launches move nothing but the moments.

    python profiles/tools/groups_timing.py [--parent-lib PATH/libgfv.so] [--runs 3] [--launches 200] [--launch-blocks 7]

prints ONE JSON line and (--out, default profiles/groups_timing.json) writes it there."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--launch-blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_timing.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    from gfv import host as gfv_host
    from gfv import lib as L
    from gfv.engine import GradStore
    from gfv.functions import unused_param_names
    from gfv.groups import MAX_GROUPS, ParamGroups
    from gfv.params import default_params
    from FVMmodel.importer import NNmodel
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU fallback"
    gfv_host.pin_to_l3()
    dev = torch.device("cuda:0")
    names, tensors = NNmodel(default_params(dataset_size=1)).param_names_tensors()
    store = GradStore(names, [t.shape for t in tensors], dev, skip=unused_param_names(names))
    n = store.total
    lib = L.load()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.gfv_adam_step_dev.restype = C.c_int
        parent.gfv_adam_step_dev.argtypes = L._SIGNATURES["gfv_adam_step_dev"][1]

    def block_of(name):
        return 0 if ".encoder." in name else (2 if ".decoder." in name else 1)
    tables = {
        "g1": ParamGroups(store, dev, {nm: 0 for nm in names}, [(0.0, 0.0, False)], True),
        "g3": ParamGroups(store, dev, {nm: block_of(nm) for nm in names}, [(0.0, 0.0, False)] * 3, True),
        "gmax": ParamGroups(store, dev, {nm: i % MAX_GROUPS for i, nm in enumerate(names)}, [(0.0, 0.0, False)] * MAX_GROUPS, True),
        "gmax_wd": ParamGroups(store, dev, {nm: i % MAX_GROUPS for i, nm in enumerate(names)}, [(0.0, 0.01, False)] * MAX_GROUPS, True),
    }
    legs = ["plain"] + (["parent"] if parent is not None else []) + list(tables)
    gen = torch.Generator().manual_seed(0)
    p, g, m, v = (torch.randn(n, generator=gen).to(dev) for _ in range(4))
    v.abs_()
    state = torch.zeros(16, dtype=torch.float32, device=dev)
    hyper = torch.tensor([0.0, 0.9, 0.999, 1e-8, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    L.check(lib.gfv_adam_state_init(state.data_ptr(), 0.9, 0.999, 0.0, L.stream_ptr()), "adam_state_init")
    L.status_mirror()

    def launch(leg):
        st = L.stream_ptr()
        if leg in ("plain", "parent"):
            fn = (lib if leg == "plain" else parent).gfv_adam_step_dev
            L.check(fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), hyper.data_ptr(), st), "adam_step")
        else:
            t = tables[leg]
            L.check(lib.gfv_adam_step_groups_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, state.data_ptr(),
                                                 hyper.data_ptr(), None, None, None, t.run_start.data_ptr(), t.run_group.data_ptr(),
                                                 t.n_runs, t.table.data_ptr(), st), "adam_step_groups")
    out = {"n_params": n, "n_runs": tables["g1"].n_runs, "launches_per_block": args.launches, "us": {leg: [] for leg in legs}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.runs):
        per = {leg: [] for leg in legs}
        for blk in range(args.launch_blocks + 1):          # (the first block of each leg warms up and is dropped)
            for leg in legs:
                e0.record()
                for _ in range(args.launches):
                    launch(leg)
                e1.record()
                torch.cuda.synchronize()
                if blk:
                    per[leg].append(1e3 * e0.elapsed_time(e1) / args.launches)
        for leg in legs:
            out["us"][leg].append(round(statistics.median(per[leg]), 3))
    out["us_median"] = {leg: round(statistics.median(out["us"][leg]), 3) for leg in legs}
    out["us_spread"] = {leg: round(max(out["us"][leg]) - min(out["us"][leg]), 3) for leg in legs}
    base = "parent" if parent is not None else "plain"
    out["baseline"] = base
    out["ratio_to_baseline"] = {leg: round(out["us_median"][leg] / out["us_median"][base], 4) for leg in legs}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
