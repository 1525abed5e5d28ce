"""Launch trace of one recorded training step: what the host issues, in order, without its pointers.

    GFV_CMDLIST_NATIVE=0 python profiles/tools/launch_trace.py --case cyl_cavity_b2
    GFV_CMDLIST_NATIVE=0 GFV_CBWD=0 python profiles/tools/launch_trace.py --cells 4500 [--net EPD]

Builds the default model on the mesh, runs TrainStep(use_graph="list") for three steps (two warm-ups, one recording) and prints
  - every request to Engine._workspace of the three steps: the floats asked for, which of the two slab workspaces was current
    (`side` = _dw_ws, `main` = _dw_ws_main swapped in by flush(on_main=True)) and its size before -> after;
  - the recorded CommandList.cmds, one per line: the callable's name, the stream (main / side / other), every integer argument
    below 2^31 as itself and anything larger as P, and for ctypes struct / struct-array arguments their non-pointer fields.
Two trees issue the same step exactly when their outputs are equal (`diff`): the tool for host-side refactors of gfv/engine.py.
It reads arguments at the C-ABI boundary only - no kernel code."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch   # noqa: E402


def _num(v):
    if isinstance(v, bool):
        return str(int(v))
    if isinstance(v, int):
        return str(v) if -(1 << 31) <= v < (1 << 31) else "P"
    if isinstance(v, float):
        return repr(v)
    return None


def _fields(s):
    """The non-pointer fields of a ctypes structure (nested structures and arrays included)."""
    out = []
    for name, tp in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out.append(f"{name}={{{_fields(v)}}}")
        elif isinstance(v, C.Array):
            if issubclass(v._type_, C.Structure):
                out.append(f"{name}=[" + " ".join("{" + _fields(e) + "}" for e in v) + "]")
            elif v._type_ is not C.c_void_p and not hasattr(v._type_, "contents"):
                out.append(f"{name}=[" + " ".join(_num(e) or "?" for e in v) + "]")
        elif tp is C.c_void_p or tp is C.c_char_p or hasattr(tp, "contents"):
            continue
        else:
            out.append(f"{name}={_num(v) or '?'}")
    return " ".join(out)


def _arg(a, main, side):
    if a is None:
        return "0"
    if isinstance(a, C.c_void_p):
        if a.value is None:
            return "0"
        return "side" if a.value == side else "main" if a.value == main else "P"
    if hasattr(a, "_obj"):          # ctypes.byref(struct)
        a = a._obj
    if isinstance(a, C.Structure):
        return "{" + _fields(a) + "}"
    if isinstance(a, C.Array):
        if issubclass(a._type_, C.Structure):
            return "[" + " ".join("{" + _fields(e) + "}" for e in a) + "]"
        return "[" + " ".join(_num(e) or "?" for e in a) + "]"
    if isinstance(a, C._SimpleCData):
        return _num(a.value) or "?"
    if torch.is_tensor(a):
        return "T" + str(list(a.shape))
    return _num(a) or type(a).__name__


def _stream_of(args, st, main, side):
    if st is not None:            # a host-side command noted with the stream it ran under
        return "side" if st.cuda_stream == side else "main" if st.cuda_stream == main else "other"
    ptrs = [a.value or 0 for a in args if isinstance(a, C.c_void_p)]
    if side and side in ptrs:
        return "side"
    if (main in ptrs) if main else (bool(args) and isinstance(args[-1], C.c_void_p) and not args[-1].value):
        return "main"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="a batch of tests/golden/cases.py (default: cyl_cavity_b2)")
    ap.add_argument("--cells", type=int, default=0, help="a meshgen channel-cylinder mesh of about this many cells instead")
    ap.add_argument("--net", default="TransFVGN_v2")
    a = ap.parse_args()
    if os.environ.get("GFV_CMDLIST_NATIVE", "1") != "0":
        sys.exit("launch_trace.py reads the Python-level command list: run it with GFV_CMDLIST_NATIVE=0")
    from FVMmodel.importer import NNmodel
    from gfv import engine as E
    from gfv.params import default_params
    from gfv.trainer import TrainStep
    if a.cells:
        from gfv import meshgen
        from gfv.graph import build_batch
        nx, ny = meshgen.cylinder_grid_for_cells(a.cells)
        mesh = meshgen.finish_mesh(meshgen.raw_tri_channel_cylinder(nx=nx, ny=ny, seed=5), U=0.3)
        graphs = build_batch([mesh], [meshgen.random_fields(mesh, seed=9)])
    else:
        import cases
        graphs = cases.make_graphs(a.case or "cyl_cavity_b2")
    print(f"# net={a.net} N={graphs[0].x.shape[0]} E={graphs[0].edge_index.shape[1]}")
    torch.manual_seed(0)
    # (the drop-in model has no net="EPD" - the plain encoder / GnBlocks / decoder simulator is TransFVGN_v1 without its Transolver
    # block: the engine of a TransFVGN_v1 model takes that branch; the block's parameters then receive no gradient)
    model = NNmodel(default_params(dataset_size=1, net="TransFVGN_v1" if a.net == "EPD" else a.net)).cuda()
    eng = model.engine()
    eng.net = a.net

    swapped = [0]
    plain_ws, plain_flush = E.Engine._workspace, E.Engine.flush

    def workspace(self, n_floats, dev):
        before = 0 if self._dw_ws is None else self._dw_ws.numel()
        ws = plain_ws(self, n_floats, dev)
        print(f"workspace {int(n_floats)} {'main' if swapped[0] else 'side'} {before}->{ws.numel()}")
        return ws

    def flush(self, on_main=False, split=0):
        swap = bool(self._pending and on_main and not (split and len(self._pending) > 1))   # (the branch that swaps the workspaces)
        swapped[0] += swap
        try:
            return plain_flush(self, on_main=on_main, split=split)
        finally:
            swapped[0] -= swap

    E.Engine._workspace, E.Engine.flush = workspace, flush
    ts = TrainStep(model, tuple(g.clone().to("cuda") for g in graphs), use_graph="list")
    cl = None
    for step in range(6):
        print(f"# step {step}")
        ts.step()
        cl = next((e.cl for e in ts._lists.values()), None)
        if cl is not None:
            break
    torch.cuda.synchronize()
    if cl is None:
        sys.exit("no command list was recorded")
    main_h = cl.main.cuda_stream
    side_h = 0 if eng._side is None else eng._side.cuda_stream
    print(f"# recorded list: {len(cl.cmds)} commands")
    for cmd in cl.cmds:
        fn, args, st = cmd[0], cmd[1], cmd[2]
        name = getattr(fn, "__name__", None) or type(fn).__name__
        print(name, _stream_of(args, st, main_h, side_h), " ".join(_arg(x, main_h, side_h) for x in args))


if __name__ == "__main__":
    main()
