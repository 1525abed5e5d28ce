"""Worker of tests/test_grad_guard_gpu.py::test_guarded_step_through_rccl_one_rank_is_bit_identical (launched with
torch.distributed.run --nproc-per-node 1, backend nccl = RCCL): TrainStep(distributed=True, max_grad_norm=c) on a one-rank group.
In the data-parallel step the Adam launch sits behind the all-reduce, outside the recorded list - the guard's two launches take
its place there; a one-rank all-reduce being the identity, parameters, moments, Adam state and the guard's own record must be
BIT-IDENTICAL to the non-distributed guarded step.  Eager and command-list mode."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

NSTEPS = 5   # command list: two warm-up steps, the recording, two replays


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    import cases
    from oracle import fvgn_oracle as O
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    from gfv.trainer import TrainStep
    P = O.init_parameters(cases.WEIGHT_SEED)
    bound = [None]

    def run(distributed, use_graph):
        model = NNmodel(default_params(dataset_size=1))
        sd = model.state_dict()
        for k, v in P.items():
            sd[k].copy_(v)
        model.load_state_dict(sd)
        model = model.cuda()
        g = tuple(t.clone().to("cuda") for t in cases.make_graphs("cyl_cavity_b2"))
        ts = TrainStep(model, g, lr=1e-3, world_size=1, use_graph=use_graph, distributed=distributed, max_grad_norm=1e30,
                       skip_nonfinite=True)
        for k in range(NSTEPS):
            if k == 1:
                if bound[0] is None:
                    bound[0] = 0.5 * ts.guard_stats()["norm"]   # (measured once; every run gets the same bound)
                ts.max_grad_norm = bound[0]
            ts.step()
        torch.cuda.synchronize()
        ns = ts.named_state()
        parts = dict(p=torch.cat([v[0].reshape(-1) for v in ns.values()]), m=torch.cat([v[1].reshape(-1) for v in ns.values()]),
                     v=torch.cat([v[2].reshape(-1) for v in ns.values()]), state=ts.adam_state, guard=ts._guard.guard,
                     loss=ts.loss.reshape(-1))
        return {k: v.detach().cpu().view(torch.int32).clone() for k, v in parts.items()}, ts.guard_stats()

    ok = True
    for use_graph in (False, "list"):
        ref, _ = run(False, use_graph)
        got, st = run(True, use_graph)
        diff = [k for k in ref if not torch.equal(ref[k], got[k])]
        if diff:
            print("GUARDDIFF", use_graph, diff)
        ok = ok and not diff and st["clipped"] >= 1
        print(f"GUARDRESULT mode={ {False: 'eager', 'list': 'list'}[use_graph] } same={int(not diff)} clipped={st['clipped']} "
              f"backend={dist.get_backend()} world={dist.get_world_size()}")
    print(f"GUARDOK {int(ok)}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
