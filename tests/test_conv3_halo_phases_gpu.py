"""The LDS-halo 3x3x3 conv's two main-loop bodies (csrc/conv3_halo.hpp) are the same function, bit for bit: the default body (knob
conv_halo = 1: one phase of 32 MFMAs per tap, the 27 taps of a channel slice unrolled) against its predecessor (conv_halo = 2: two
phases of 16 MFMAs per k-tile).  Every accumulator takes the same k-tiles in the same order (channel slice outermost, tap inner), so
EVERY output voxel must be equal - torch.equal, no tolerance.

Shapes: the smallest volumes the launcher admits for each tile (M / BM >= 192, whole 2 x (8|16) x 16 blocks, H != W: the ones
tests/gemm_forms_cases.py names), with Cin = 64 (two slices: one seam, planes 2 / 3 refilled on the very first slice change) and
Cin = 192 (six slices: the W ring's slot rotates by three per slice, every residue occurs); a T = 2 volume (one t block: planes 0 and
3 are zero rows for every block) and the head2 width (224 = 14 w blocks, the benchmark's top launch shrunk in t and batch).  Two
epilogues that differ in register pressure, both 16-bit types.  Each call's profiler tag proves which body ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import ops
from l4p_amd._lib import ACT_NONE, ACT_RELU, L4P_BF16, L4P_F16
from tests.test_gemm8p_gpu import prof_tags
from tests.test_kernels_gpu import as_mode, rnd

CASES = [(vol, cin, cout, epi) for vol, cout in (((2, 4, 64, 96), 256), ((2, 4, 96, 128), 128)) for cin in (64, 192)
         for epi in ("relu", "res2")]
CASES += [((2, 2, 128, 96), 64, 256, "res2"),      # T = 2: a single t block
          ((1, 2, 224, 224), 128, 128, "relu")]    # head2 width: 14 w blocks


def _run(x, wp, cout, bias, epi, res):
    if epi == "relu":
        outs = (ops.conv3d_k3(x, wp, cout, bias=bias, act=ACT_RELU),)
    else:  # two residuals of the output's type + the relu copy
        outs = ops.conv3d_k3(x, wp, cout, bias=bias, act=ACT_NONE, res1=res[0], res2=res[1], relu_copy=True)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("mode", [L4P_BF16, L4P_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("vol,cin,cout,epi", CASES, ids=[f"{'x'.join(map(str, v))}-cin{c}-n{n}-{e}" for v, c, n, e in CASES])
def test_one_phase_body_equals_two_phase_body(dev, knob, mode, vol, cin, cout, epi):
    B, T, H, W = vol
    tile = "t256x256" if cout == 256 else "t512x128"
    x, _ = as_mode(rnd((B, T, H, W, cin), 500), mode)
    w = rnd((cout, cin, 3, 3, 3), 501, (27 * cin) ** -0.5)
    wT, _ = as_mode(w.permute(0, 2, 3, 4, 1).reshape(cout, 27 * cin), mode)
    wp = ops.pad_rows(wT, 256)
    bias = rnd((cout,), 502).cuda()
    res = [as_mode(rnd((B, T, H, W, cout), 503 + i), mode)[0] for i in range(2)] if epi == "res2" else None
    got = {}
    for body, form in ((1, f"halo {tile}"), (2, f"halo 2p {tile}")):
        knob("conv_halo", body)
        with prof_tags() as p:
            got[body] = _run(x, wp, cout, bias, epi, res)
        tags = [ln[1] for ln in p.lines if ln[0] == "conv3d"]
        assert len(tags) == 1 and tags[0].endswith(f" act{ACT_RELU if epi == 'relu' else ACT_NONE} {form}"), (body, p.lines)
    assert len(got[1]) == len(got[2]) == (1 if epi == "relu" else 2)
    for a, b in zip(got[1], got[2]):
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0.1
        assert torch.equal(a, b), (int((a != b).sum()), float((a.float() - b.float()).abs().max()))
