"""Every kernel form l4p_attention can launch (csrc/attention.hip launch_attention / launch_attention16, csrc/attention64.hip), each at
the smallest shape that reaches it and at sequence lengths that are not a power of two, against fp64 softmax(q k^T) v on the same
rounded operands (reference call site: modeling_finetune.py:169-190).  Every case asserts, through the event profiler's tag
(l4p_prof_detail: "B S H Dh form", include/l4p_hip.h), that the launch really was the form it is about.

What the shapes reach:
  * KV-split with an ODD number of KV blocks per wave group (nit = 3, 5, 9): the pipeline's single-block tail after the steady-state
    loop, score registers and ring slots in the opposite phase to nit = 1;
  * the 4-wave unsplit kernel, the f32 kernel and the 64-row kernel at S % 256 != 0 / S / 256 = 3;
  * the 8-wave query-split kernel: persistent (the seam: next tile's K / V^T on the rings, Q through LDS) and one workgroup per
    tile, which must agree BIT FOR BIT (same instantiation, same per-tile arithmetic; a difference is state leaking across a seam);
  * the compiler-scheduled bodies (knob attn_variant = 1) and the "no query split" aid (attn_variant = 2).

Tolerances: tests/test_kernels_gpu.py's check_attn, unchanged.  Inputs: random, head-dim padding zero, first KV block * 0.01, eight
dominant keys (* 6) in the last KV block and eight in the one before it (the peeled final step; under KV-split the last block of
each wave group), query row 17 * 8.  That these inputs discriminate is asserted on the CPU for every case: a reference whose last
two KV blocks of V are exchanged fails check_attn against the true one (tests/test_attention_forms_cpu.py runs that without a GPU).
"""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib, ops
from l4p_amd._lib import L4P_BF16, L4P_F16, L4P_F32
from tests.test_gemm8p_gpu import prof_tags
from tests.test_kernels_gpu import LOG2E, _attn_inputs, as_mode, check_attn

E_INVALID = _lib.L4P_E_INVALID
MODES16 = pytest.mark.parametrize("mode", [L4P_BF16, L4P_F16], ids=["bf16", "f16"])


@functools.lru_cache(maxsize=None)
def case(B, S, H, Dh, mode, prescaled):
    """CPU side of one case (shared by the tests that run it, never modified): operands [B,S,H,96] rounded to the engine type and
    the fp64 reference [B*S, H*Dh] (as float), one batch item at a time.  Asserts that the inputs discriminate (module docstring)."""
    td = ops.torch_dtype(mode)
    kvb = ops.kv_block(td)
    g = torch.Generator().manual_seed(B * 100003 + S * 101 + H * 7 + Dh)
    q4 = torch.randn(B, S, H, ops.DP, generator=g)
    k4 = torch.randn(B, S, H, ops.DP, generator=g)
    v4 = torch.randn(B, S, H, ops.DP, generator=g)
    for t in (q4, k4, v4):
        t[..., Dh:] = 0
    k4[:, :kvb] *= 0.01                           # first block nearly flat: every later block raises the maximum
    k4[:, S - 12:S - 4] *= 6.0                    # eight dominant keys in the last KV block
    k4[:, S - 2 * kvb + 5:S - 2 * kvb + 13] *= 6.0  # ... and eight in the one before it
    q4[:, 17] *= 8.0
    if prescaled:
        q4 = q4 * (Dh ** -0.5 * LOG2E)
    qT, kT, vT = q4.to(td), k4.to(td), v4.to(td)
    mult = math.log(2.0) if prescaled else Dh ** -0.5  # pre-scaled q: the weights are exp2(q' k^T)
    ref, swapped = torch.empty(B, S, H, Dh), torch.empty(B, S, H, Dh)
    for b in range(B):
        qh, kh, vh = (t[b].permute(1, 0, 2).double() for t in (qT, kT, vT))  # H S 96
        attn = torch.softmax((qh * mult) @ kh.transpose(-2, -1), dim=-1)
        ref[b] = (attn @ vh)[..., :Dh].permute(1, 0, 2).float()
        vx = torch.cat([vh[:, :S - 2 * kvb], vh[:, S - kvb:], vh[:, S - 2 * kvb:S - kvb]], dim=1)
        swapped[b] = (attn @ vx)[..., :Dh].permute(1, 0, 2).float()
    ref, swapped = ref.reshape(B * S, H * Dh), swapped.reshape(B * S, H * Dh)
    with pytest.raises(AssertionError):  # a kernel that mixed up the last two KV blocks would not pass
        check_attn(swapped.to(td), ref, mode, prescaled)
    return qT, kT, vT, ref


def run(B, S, H, Dh, mode, prescaled, form):
    """One launch on the case's operands; asserts the kernel form through the profiler tag."""
    qT, kT, vT, _ = case(B, S, H, Dh, mode, prescaled)
    q, kt, vt = _attn_inputs(qT.float(), kT.float(), vT.float(), mode)[:3]
    with prof_tags() as p:
        out = ops.attention(q, kt, vt, Dh, scale=0.0 if prescaled else None)
    tags = [ln[1] for ln in p.lines if ln[0] == "attention"]
    assert tags == [f"B{B} S{S} H{H} Dh{Dh} {form}"], p.lines
    return out


def compare(out, B, S, H, Dh, mode, prescaled, form):
    ref = case(B, S, H, Dh, mode, prescaled)[3]
    y = out.float().cpu()
    assert bool(torch.isfinite(y).all())
    rel_l2 = ((y - ref).norm() / ref.norm()).item()
    err = ((y - ref).abs().max() / ref.abs().max()).item()
    print(f"ATTN_FORM form='{form}' mode={mode} B={B} S={S} H={H} Dh={Dh} prescaled={int(prescaled)} rel_l2={rel_l2:.3e} max_err/max|ref|={err:.3e}")
    check_attn(out, ref, mode, prescaled)


SCALE_FORMS = pytest.mark.parametrize("prescaled", [True, False], ids=["prescaled", "scale_inside"])


@MODES16
@SCALE_FORMS
@pytest.mark.parametrize("B,S,H,Dh", [(1, 384, 2, 88), (1, 640, 3, 64), (1, 1152, 16, 88)])  # nit = 3, 5, 9
def test_kv_split_odd_blocks_per_wave_group(dev, mode, prescaled, B, S, H, Dh):
    """nit = (S / 64) / 2 odd and > 1: the single-block tail of the pipeline after the steady-state loop has run.  (1, 1152, 16, 88)
    is the encoder's 192 x 192 clip at batch 1.  Pre-scaled q (the engine's form) and the scale-inside form; the latter runs the
    hand-scheduled body for f16 and, for bf16, the compiler-scheduled one (launch_attention: the hand-scheduled body would round
    q * scale * log2 e to bf16 a second time, which on these inputs - the * 8 query row against the * 6 keys - costs 2.7e-2 of
    max|ref| at (1, 640, 3, 64), measured, and as much in an fp64 softmax on q re-rounded that way: past check_attn's 2^-6)."""
    form = "kvsplit cs" if mode == L4P_BF16 and not prescaled else "kvsplit"
    compare(run(B, S, H, Dh, mode, prescaled, form), B, S, H, Dh, mode, prescaled, form)


@MODES16
@SCALE_FORMS
def test_kv_split_compiler_scheduled(dev, knob, mode, prescaled):
    knob("attn_variant", 1)
    compare(run(1, 384, 2, 88, mode, prescaled, "kvsplit cs"), 1, 384, 2, 88, mode, prescaled, "kvsplit cs")


@MODES16
@pytest.mark.parametrize("Dh", [88, 64])
def test_unsplit_4_wave_at_six_kv_blocks(dev, mode, Dh):
    """528 tiles of 128 rows (no KV split), S % 256 != 0 (neither the 64-row nor the query-split kernel)."""
    compare(run(11, 384, 16, Dh, mode, True, "unsplit"), 11, 384, 16, Dh, mode, True, "unsplit")


@MODES16
def test_unsplit_4_wave_compiler_scheduled(dev, knob, mode):
    knob("attn_variant", 1)
    compare(run(11, 384, 16, 64, mode, True, "unsplit cs"), 11, 384, 16, 64, mode, True, "unsplit cs")


@MODES16
@pytest.mark.parametrize("B,S,H,Dh", [(32, 256, 16, 88),   # 512 tiles, two per workgroup; nit = 4: Q of the next tile is issued at step 0
                                      (33, 256, 16, 88),   # 528 tiles: workgroups with two and with three tiles
                                      (8, 1024, 16, 88)])  # 16 KV blocks
def test_query_split_8_wave_persistent_equals_one_workgroup_per_tile(dev, knob, mode, B, S, H, Dh):
    """attn_kernel<T16, 64, 88, 1, true, 2>: both launch forms against the reference, and bit for bit against each other."""
    knob("attn64", 0)
    out = {}
    for persist, form in ((1, "qsplit persist"), (0, "qsplit pertile")):
        knob("attn_persist", persist)
        out[persist] = run(B, S, H, Dh, mode, True, form)
        compare(out[persist], B, S, H, Dh, mode, True, form)
    differ = (out[1].view(torch.int16) != out[0].view(torch.int16)).any(dim=1).nonzero().flatten()
    assert differ.numel() == 0, f"{differ.numel()} output rows differ between attn_persist 1 and 0, first {differ[:8].tolist()}"


@MODES16
def test_no_query_split_aid(dev, knob, mode):
    """attn_variant = 2 at a launch the query-split kernel would take: the 4-wave unsplit kernel."""
    knob("attn64", 0)
    knob("attn_variant", 2)
    compare(run(32, 256, 16, 88, mode, True, "unsplit"), 32, 256, 16, 88, mode, True, "unsplit")


@MODES16
@pytest.mark.parametrize("Dh", [88, 64])
def test_rows64_at_three_tiles_per_head(dev, knob, mode, Dh):
    """csrc/attention64.hip with S / 256 = 3: 264 tiles (some workgroups walk two), 12 KV blocks; and against the 4-wave kernel on the
    same inputs (attn64 = 0) under tests/test_kernels_gpu.py's bound for that pair: the two agree to the rounding of P."""
    B, S, H = 11, 768, 8
    out64 = run(B, S, H, Dh, mode, True, "rows64")
    compare(out64, B, S, H, Dh, mode, True, "rows64")
    knob("attn64", 0)
    out4 = run(B, S, H, Dh, mode, True, "unsplit")
    compare(out4, B, S, H, Dh, mode, True, "unsplit")
    ref = case(B, S, H, Dh, mode, True)[3]
    d = (out64.float() - out4.float()).abs().max().item()
    assert d <= ref.abs().max().item() * 2 ** (-6 if mode == L4P_BF16 else -9), d


@SCALE_FORMS
@pytest.mark.parametrize("B,S,H,Dh", [(1, 384, 2, 88), (1, 384, 3, 64)])  # 12 KV blocks of 32
def test_f32_kernel_at_s_384(dev, prescaled, B, S, H, Dh):
    compare(run(B, S, H, Dh, L4P_F32, prescaled, "f32"), B, S, H, Dh, L4P_F32, prescaled, "f32")


@pytest.mark.parametrize("S,Dh,scale,names", [(192, 88, 0.0, "S=192"), (256, 80, 0.0, "Dh=80"), (256, 88, -1.0, "scale=-1"),
                                              (256, 88, float("nan"), "scale=nan")])
def test_argument_errors(dev, S, Dh, scale, names):
    """Refused before any launch: L4P_E_INVALID, the message names the argument, the output is untouched."""
    lib = _lib.load()
    H = 2
    q = as_mode(torch.zeros(256, H * ops.DP), L4P_BF16)[0]
    kt, vt = q.clone().view(-1), q.clone().view(1, H, ops.DP, 256)
    out = torch.full((256, H * 88), 7.0, dtype=torch.bfloat16, device="cuda")
    with prof_tags() as p:
        rc = lib.l4p_attention(torch.cuda.current_stream().cuda_stream, L4P_BF16, q.data_ptr(), kt.data_ptr(), vt.data_ptr(), out.data_ptr(),
                               1, S, H, Dh, C.c_float(scale))
    assert rc == E_INVALID
    msg = lib.l4p_last_error().decode()
    assert "attention" in msg and names in msg, msg
    assert not [ln for ln in p.lines if ln[0] == "attention"], p.lines
    assert bool((out == 7.0).all())
