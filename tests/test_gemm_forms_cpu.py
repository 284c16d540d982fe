"""The inputs of tests/test_gemm_forms_gpu.py discriminate, shown without a GPU: for every case, a reference with the last k-chunk of the
contraction dropped and one whose last 8-column group is taken from the neighbouring group both fail tests/test_kernels_gpu.py's check
against the true float64 reference - for every output of the case - while the true reference, rounded to the output type, passes."""
import pytest
import torch

from l4p_amd import ops
from l4p_amd._lib import L4P_BF16, L4P_F16
from tests import gemm_forms_cases as G
from tests.test_kernels_gpu import check


def _discriminates(case):
    ref = G.reference(case)
    td = ops.torch_dtype(case.mode)
    for name in case.outs:
        dt = torch.float32 if name == "f32" else td
        assert ref[name].shape == (len(G.ref_rows(case)), case.N) and bool(torch.isfinite(ref[name]).all())
        check(ref[name].to(dt), ref[name], case.mode, name != "f32")  # the bounds accept the reference itself
    for kind in G.wrong_kinds(case):
        wrong = G.reference(case, kind)
        for name in case.outs:
            dt = torch.float32 if name == "f32" else td
            with pytest.raises(AssertionError):
                check(wrong[name].to(dt), ref[name], case.mode, name != "f32")


@pytest.mark.parametrize("case", G.DENSE_CASES + G.CONV_CASES + G.SCATTER_CASES, ids=G.case_id)
def test_wrong_references_fail_the_bounds(case):
    _discriminates(case)


@pytest.mark.parametrize("mode", [L4P_BF16, L4P_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("eight_phase", [True, False], ids=["8p", "staged"])
def test_wrong_references_fail_the_bounds_in_the_epilogue_sweep(mode, eight_phase):
    for gen in (0, 1):
        cases = G.sweep_cases(mode, eight_phase, gen)
        assert len(cases) == 3 * 5 * 4 + 2
        for case in cases:
            _discriminates(case)


def test_case_lists():
    """every case appears once, and the only case without a neighbouring column group is the single-group one"""
    assert len(set(G.ALL_CASES)) == len(G.ALL_CASES)
    assert {(c.M, c.N, c.K) for c in G.ALL_CASES if G.wrong_kinds(c) == ("dropk",)} == {(129, 8, 72)}
    lean = [c for c in G.sweep_cases(L4P_BF16, True, 0) if c.form == "8p t256x192"]
    assert len(lean) == 4 * (3 + 1 + 2 * 2)  # outputs x ((any act, no residual) + (none, float) + (none | ReLU, T) x (one | two residuals))
