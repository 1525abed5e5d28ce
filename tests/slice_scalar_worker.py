"""Worker of tests/test_slice_gpu.py::test_scalar_forms_in_a_child_process.  GFV_SLICE_MFMA is read once per process, so the
scalar forms of csrc/slice.hip - slice_token_partial_kernel, slice_post_bwd_kernel over every workgroup, deslice_kernel over
uniform workgroups with its LDS-staged slice tensor - are reached only by a fresh interpreter started with GFV_SLICE_MFMA=0.
Runs the node-kernel checks of tests/slice_float64.py and prints one `SLICECHECK <case> <ok> <kind> <value> <name>` line per
check, then `SLICEDONE <number of checks>`."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd")):
    sys.path.insert(0, p)

CASES = ("thirteen_graphs", "one_graph_96")


def main():
    assert os.environ.get("GFV_SLICE_MFMA") == "0", "start me with GFV_SLICE_MFMA=0"
    import torch
    import slice_float64 as S
    assert torch.cuda.is_available()
    impl, n = S.Gpu(), 0
    for case in CASES:
        for c in S.node_checks(S.node_case(*S.NODE_CASES[case]), impl):
            print(f"SLICECHECK {case} {int(c.ok)} {c.kind} {c.value:.3e} {c.name}", flush=True)
            n += 1
    print(f"SLICEDONE {n}", flush=True)


if __name__ == "__main__":
    main()
