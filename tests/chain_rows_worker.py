"""Worker of tests/test_chain_rows_gpu.py::test_deep_walks_in_a_child_process.  GFV_COLCHAIN_WGS (the number of persistent
workgroups of csrc/colchain_kernel.h) is read once per process, so a walk of 5 - 14 tiles per workgroup at a test-sized M is
reached only by a fresh interpreter started with it: 3 keeps the identity workgroup order, 8 takes the permuted one.  Runs the
row checks of tests/chain_rows.py on the column-owner kernel (read and recompute form) at M = 2597 - tile starts off 64-row
alignment - and prints one `ROWCHECK <family>/<name> <ok> <value> <bound>` line per check, `ROWACC ...` lines for the record,
`ROWCLIFF <family> <log2 of the largest ratio of reported g3 scales over the small side of cliff_down, a tile and more behind the cliff>`, then
`ROWDONE <number of checks>`."""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd")):
    sys.path.insert(0, p)

M = 2597
FAMILIES = ("col_read", "col_rc")


def plan(R):
    """(shape, layout) of every run: all layouts on the EdgeBlock shape, zigzag and zeros on the other two."""
    return [("edge", lay) for lay in R.LAYOUTS] + [(s, lay) for s in ("node", "enc") for lay in ("zigzag", "zeros")]


def main():
    n = int(os.environ.get("GFV_COLCHAIN_WGS", "0"))
    assert n > 0, "start me with GFV_COLCHAIN_WGS=<workgroups>"
    import torch
    import chain_rows as R
    from gfv import lib as L
    assert torch.cuda.is_available()
    assert L.load().gfv_rowtile_dw_partials() == n, (L.load().gfv_rowtile_dw_partials(), n)
    count = 0
    for fam in FAMILIES:
        impl = R.Gpu(fam)
        for shape, layout in plan(R):
            c = R.case(shape, M)
            out = impl.run(c, layout)
            for k in R.checks(c, layout, out, names=R.ROWS_COL[shape]):
                print(f"ROWCHECK {fam}/{k.name} {int(k.ok)} {k.value:.3e} {k.bound:.3e}", flush=True)
                count += 1
            if layout in ("mixed", "cliff_down"):
                print("\n".join(R.rowacc(f"{fam}_wgs{n}", c, layout, out)), flush=True)
            if layout == "cliff_down":
                # groups at least one tile behind the cliff: the tile that straddles it carries the large rows' scale anyway
                small = torch.arange(M) >= int(0.45 * M) + 64
                grp = small[: M // 16 * 16].view(-1, 16).all(1)
                s = out.gscale[0][: M // 16][grp]
                print(f"ROWCLIFF {fam} {math.log2(float(s.max() / s.min())):.1f}", flush=True)
    print(f"ROWDONE {count}", flush=True)


if __name__ == "__main__":
    main()
