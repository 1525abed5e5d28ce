"""Probe of the host's fp32 LAPACK rounding for tests/test_oracle_golden.py::test_oracle_wlsq_orders_match_reference
(tests/golden/order_solve_probe.npz).  The 3rd / 4th-order moment matrices are ill-conditioned in fp32: the row-normalised
solve of the oracle (and of the reference) rounds differently on another LAPACK code path (MKL on another instruction set),
and the order fixtures then differ from what the same algorithm computes there by 1e-1, not by 1e-5.  The probe holds the
first PROBE_ROWS row-normalised moment matrices of the fixtures' mesh, a seeded right-hand side, and the solve as the host the
order fixtures were recorded on computed it; the test compares before it does any work.
Run on the host the order fixtures come from:  python tests/golden/make_order_solve_probe.py"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd")]

import cases  # noqa: E402

PROBE_ROWS = 16


def main():
    out = {}
    for order in ("3rd", "4th"):
        A = cases.make_graphs("cyl_cavity_b2", order=order)[1].A_node_to_node[:PROBE_ROWS]
        A = A / (torch.norm(A, p=2, dim=2, keepdim=True) + 1e-8)          # as oracle/fvgn_oracle.py node_based_WLSQ
        rhs = torch.from_numpy(np.random.default_rng(0).standard_normal((A.shape[0], A.shape[1], 3)).astype(np.float32))
        out[f"{order}.A"], out[f"{order}.rhs"] = A.numpy(), rhs.numpy()
        out[f"{order}.x"] = torch.linalg.solve(A, rhs).numpy()
    path = os.path.join(HERE, "order_solve_probe.npz")
    np.savez(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
