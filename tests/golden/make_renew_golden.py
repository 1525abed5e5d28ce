"""Reference-generated fixture of pool renewal (gfv.pool.DevicePool.renew, csrc/pool.hip gfv_pool_renew): what the REFERENCE's
own `CFDdatasetBase.init_env` (Load_mesh.py:80-131, with `velocity_profile`, Set_BC.py:6-66) returns - `uvp_node` [N, 3] and
`target|uvp` [N, 2] - on the two synthetic meshes of tests/test_pool_gpu.py, float64 positions, for the profile kinds
`DevicePool.reset_env` does not know: `uniform_aoa` at 3 degrees, `Taylor_Green`, and a parabolic inlet over a uniform initial
field.  Beside them the arrays gfv.meshgen.velocity_profile returns for the two kinds it already knew, over all nodes and over the
inlet nodes: recorded with the meshgen.py of the commit BEFORE the new kinds were added (`--parent-meshgen FILE`: that file, e.g.
from `git show <parent>:gen-fvgn-steady_amd/gfv/meshgen.py`), so that tests/test_pool_renew_cpu.py can hold the extended
function to them bit for bit.  Only arrays (data) are stored.  Run: python tests/golden/make_renew_golden.py [--parent-meshgen FILE]"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "refstubs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases  # noqa: E402

for p in (cases.ROOT, os.path.join(cases.ROOT, "gen-fvgn-steady_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from gfv import meshgen  # noqa: E402   (the tests import MESHES / CASES / raws from here: the reference is needed by main() only)

# name -> (generator, its arguments, U)
MESHES = {
    "channel": ("raw_tri_channel_cylinder", dict(nx=30, ny=6, quad_fraction=0.0, seed=21), 0.31),
    "cavity": ("raw_quad_cavity", dict(n=7, jitter=0.1, tri_fraction=0.3, seed=13), 1.3),
}
# name -> (inlet_type, init_field_type, aoa in degrees)
CASES = {
    "aoa": ("uniform_aoa", "uniform_aoa", 3.0),
    "tg": ("Taylor_Green", "Taylor_Green", 0.0),
    "mixed": ("parabolic", "uniform", 0.0),
}
NODE_TYPES = (meshgen.NORMAL, meshgen.WALL, meshgen.INFLOW, meshgen.OUTFLOW, meshgen.IN_WALL, meshgen.PRESS_POINT)


def raws():
    out = {name: getattr(meshgen, fac)(**kw) for name, (fac, kw, _) in MESHES.items()}
    seen = set()
    for r in out.values():
        seen |= set(int(t) for t in np.unique(r["node|node_type"]))
    assert seen == set(NODE_TYPES), seen        # between them: every node type the kernel branches on
    return out


def main():
    import ref_import
    parent = meshgen
    if "--parent-meshgen" in sys.argv:
        spec = importlib.util.spec_from_file_location("meshgen_parent", sys.argv[sys.argv.index("--parent-meshgen") + 1])
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
    M = ref_import.reference_mesh_modules()
    out = {}
    for name, raw in raws().items():
        U = MESHES[name][2]
        pos, nt = raw["node|pos"], raw["node|node_type"]
        assert pos.dtype == np.float64
        inlet = (nt == meshgen.INFLOW) | (nt == meshgen.IN_WALL) | (nt == meshgen.PRESS_POINT)
        for case, (inlet_type, init_type, aoa) in CASES.items():
            mesh = {"node|pos": torch.from_numpy(pos.copy()), "node|node_type": torch.from_numpy(nt.copy()),
                    "aoa": torch.tensor(aoa, dtype=torch.float32), "inlet_type": inlet_type, "init_field_type": init_type}
            mesh, uvp_node = M.Load_mesh.CFDdatasetBase.init_env(mesh, mean_u=U)
            assert uvp_node.dtype == torch.float32 and mesh["target|uvp"].dtype == torch.float32
            out[f"{name}.{case}.uvp_node"] = uvp_node.numpy().copy()
            out[f"{name}.{case}.target"] = mesh["target|uvp"].numpy().copy()
            print(name, case, "max |u v p|", np.abs(out[f"{name}.{case}.uvp_node"]).max(axis=0))
        for kind in ("parabolic", "uniform"):
            out[f"{name}.old.{kind}.all"] = np.asarray(parent.velocity_profile(pos, U, kind), dtype=np.float64)
            out[f"{name}.old.{kind}.inlet"] = np.asarray(parent.velocity_profile(pos[inlet], U, kind), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "renew_small.npz"), **out)
    print("wrote renew_small.npz:", os.path.getsize(os.path.join(HERE, "renew_small.npz")), "bytes")


if __name__ == "__main__":
    main()
