"""The limits of tests/test_slice_gpu.py are not taken from the kernels: the float64 statements of tests/slice_float64.py,
evaluated in FLOAT32 torch on the CPU on the committed inputs, must keep a quarter of every limit - 2.5e-6 where a kernel has
1e-5 of max|ref|, 5e-7 where a summed parameter gradient has 2e-6 of the sum of the absolute values of its terms - and the inputs
must be the hard ones (the preconditions: sharp slice weights, slice norms below eps, sharp attention, |dots| <= 20).

Worst float32 torch figures on these inputs (element-wise / summed):
  thirteen_graphs 1.1e-6 / 9.0e-8    four_graphs_one_workgroup 4.0e-7 / 2.7e-7    one_node 3.1e-7 / 1.9e-7    one_graph_96 7.9e-7 / 2.5e-7
  attention, hidden 128: 7.2e-7 / 2.5e-7    hidden 64: 8.1e-7 / 2.2e-7    gfv_reduce_partials_seg 1.3e-7 / 1.7e-7"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_float64 as S  # noqa: E402


def _within_margin(ck):
    bad = ck.failed(margin=True)
    assert not bad, "\n".join(f"{c.kind} {c.value:.3e} {c.name}" for c in bad) + "\n\n" + ck.report()


@pytest.mark.parametrize("name", list(S.NODE_CASES))
def test_float32_torch_keeps_a_quarter_of_the_node_kernel_limits(name):
    _within_margin(S.node_checks(S.node_case(*S.NODE_CASES[name]), S.Torch32()))


@pytest.mark.parametrize("hidden", [128, 64])
def test_float32_torch_keeps_a_quarter_of_the_attention_limits(hidden):
    _within_margin(S.attention_checks(S.attention_case(S.ATTN_SEED, hidden), S.Torch32()))


def test_float32_torch_keeps_a_quarter_of_the_segment_sum_limits():
    _within_margin(S.seg_checks(S.seg_case(S.SEG_SEED), S.Torch32()))
