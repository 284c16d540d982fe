"""The inputs of tests/test_attention_forms_gpu.py discriminate, shown without a GPU: building a case asserts that a reference whose
last two KV blocks of V are exchanged fails check_attn (the project's attention bounds) against the true fp64 reference."""
import pytest
import torch

from l4p_amd._lib import L4P_BF16, L4P_F16, L4P_F32
from tests.test_attention_forms_gpu import case
from tests.test_kernels_gpu import check_attn


@pytest.mark.parametrize("mode", [L4P_BF16, L4P_F16, L4P_F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("B,S,H,Dh", [(1, 384, 2, 88), (1, 640, 3, 64), (2, 256, 2, 88)])
def test_exchanged_kv_blocks_fail_the_attention_bounds(mode, prescaled, B, S, H, Dh):
    qT, kT, vT, ref = case(B, S, H, Dh, mode, prescaled)  # (asserts the exchanged reference fails)
    assert ref.shape == (B * S, H * Dh) and bool(torch.isfinite(ref).all())
    assert bool((qT[..., Dh:] == 0).all() and (kT[..., Dh:] == 0).all() and (vT[..., Dh:] == 0).all())
    check_attn(ref, ref, mode, prescaled)  # and the bounds accept the reference itself
