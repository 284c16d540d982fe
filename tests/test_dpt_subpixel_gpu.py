"""GPU: the sub-pixel conv (l4p_conv3d_subpixel: the DPT up-scaling ConvTranspose3d folded into the 3x3x3 conv behind it).

Kernel level, through the C ABI.  The reference is the float64 torch chain conv3d(conv_transpose3d(x)) on the UN-ROUNDED weights and
the storage-rounded input.
  * f32 engine: the bound of the f32 conv kernel tests (`check` of tests/test_kernels_gpu.py).
  * 16-bit engines: the folded result's relative L2 error against that reference must not exceed the error of the unfolded native
    path (l4p_gemm ConvTranspose, then l4p_conv3d_k3) on the same inputs: the fold removes the rounding of the intermediate and one of
    the two weight roundings.  No margin.  Measured folded / unfolded (bf16 and f16; MI355X), in the order of CASES below:
    0.665 / 0.663, 0.634 / 0.658, 0.643 / 0.642, 0.661 / 0.656, 0.645 / 0.647.
Model level (mini geometry, two clips, depth + camray): the knob dpt_fold_rn switches the decoder between the two forms - seen in the
event profiler's tags - and the dense outputs of the two settings agree within the per-precision bounds of
test_mini_encoder_and_dense_heads_vs_oracle_and_golden.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from l4p_amd import _lib, ops, packing
from l4p_amd._lib import L4P_BF16, L4P_F16, L4P_F32
from tests.test_kernels_gpu import as_mode, check, rnd

MODES = [L4P_F32, L4P_BF16, L4P_F16]

# k, B, grid, Cin, Cout, 8-phase form (16-bit engines; forced through the gemm_variant knob: its own threshold is 256 tiles of 256 x 256)
CASES = [
    ((2, 4, 4), 2, (2, 3, 5), 64, 128, False),     # 60 rows: a partial tile with a batch boundary inside; every border class, all four cell patterns
    ((2, 2, 2), 2, (1, 3, 2), 128, 128, False),    # a grid axis of one cell: first cell == last cell; two k-tiles per cell
    ((2, 1, 1), 1, (2, 3, 3), 64, 128, False),     # un-scaled axes: three cells along h and w
    ((2, 2, 2), 1, (4, 16, 16), 64, 256, True),    # 1024 rows, power-of-two grid: 4 x 8 tiles of the 8-phase form
    ((2, 4, 4), 2, (2, 3, 5), 128, 256, True),     # the 8-phase form on short, unequal k-loops (2 / 4 / 8 cells), a partial tile, divisions
]


class prof_tags:
    """The (class, tag, count) lines of every launch inside the block (l4p_prof_detail)."""

    def __enter__(self):
        self.lib = _lib.load()
        torch.cuda.synchronize()
        self.lib.l4p_prof_reset()
        self.lib.l4p_prof_enable(1)
        self.lines = []
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.l4p_prof_enable(0)
        n = self.lib.l4p_prof_detail(None, 0)
        buf = C.create_string_buffer(int(n) + 16)
        self.lib.l4p_prof_detail(buf, len(buf))
        self.lines = [ln.split("\t") for ln in buf.value.decode().splitlines() if ln]
        self.lib.l4p_prof_reset()
        return False

    def count(self, *needles):
        return sum(int(ln[2]) for ln in self.lines if ln[0] == "conv3d" and all(s in ln[1] for s in needles))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


_INPUTS = {}


def inputs(case):
    """Un-rounded operands and the float64 reference per (case, storage type of x), computed once."""
    if case not in _INPUTS:
        k, B, grid, cin, cout, _ = case
        w_ct = rnd((cin, cin) + k, 81, cin ** -0.5)  # ConvTranspose3d layout [in][out][kt][kh][kw]
        b_ct = rnd((cin,), 82)
        w_rn = rnd((cout, cin, 3, 3, 3), 83, (27 * cin) ** -0.5)
        x = rnd((B,) + grid + (cin,), 84)
        _INPUTS[case] = dict(w_ct=w_ct, b_ct=b_ct, w_rn=w_rn, x=x, fold=packing.fold_convT_rn(w_ct, b_ct, w_rn), ref={})
    return _INPUTS[case]


def reference(case, x_ref):
    d = inputs(case)
    k = case[0]
    y = F.conv_transpose3d(x_ref.double().permute(0, 4, 1, 2, 3), d["w_ct"].double(), d["b_ct"].double(), stride=k)
    return F.conv3d(y, d["w_rn"].double(), padding=1).permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("relu_copy", [False, True], ids=["plain", "relu_copy"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d%d%d_B%d_g%dx%dx%d_ci%d_co%d%s" % (c[0] + (c[1],) + c[2] + (c[3], c[4], "_8p" if c[5] else "")))
@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16", "f16"])
def test_subpixel_conv_vs_float64_chain(dev, knob, mode, case, relu_copy):
    k, B, grid, cin, cout, want8p = case
    d = inputs(case)
    x, x_ref = as_mode(d["x"], mode)
    if mode not in d["ref"]:
        d["ref"][mode] = reference(case, x_ref)
    ref = d["ref"][mode]
    fw, fb, _ = d["fold"]
    wT = fw.to(ops.torch_dtype(mode)).cuda()  # formed in float64 from the un-rounded weights, rounded once
    form8p = want8p and mode != L4P_F32
    if form8p:
        knob("gemm_variant", 10)
    with prof_tags() as pt:
        got = ops.conv3d_subpixel(x, wT, cout, k, bias_cls=fb.float().cuda(), relu_copy=relu_copy)
    if relu_copy:
        got, got_relu = got
        assert torch.equal(got_relu, torch.relu(got))
    assert tuple(got.shape) == tuple(ref.shape)
    tags = [ln[1] for ln in pt.lines if ln[0] == "conv3d"]
    assert len(tags) == 1 and ("subpix 8p" in tags[0]) == form8p and "subpix" in tags[0], pt.lines
    # K of the tag = mean executed K: 2 M N K = executed FLOPs
    nblk = d["fold"][2]
    assert f" K{nblk * cin // (k[0] * k[1] * k[2])} " in tags[0], tags
    if mode == L4P_F32:
        print(f"f32 max err / scale = {float((got.cpu().double() - ref).abs().max() / ref.abs().max()):.3g}")
        check(got, ref.float(), mode, True)
        return
    # the unfolded native path on the same inputs: ConvTranspose (its output rounded to T), then the 27-tap conv
    taps = k[0] * k[1] * k[2]
    wct_T = ops.pad_rows(packing.convT_matrix(d["w_ct"]).to(ops.torch_dtype(mode))).cuda()
    wrn_T = ops.pad_rows(packing.conv3_matrix(d["w_rn"]).to(ops.torch_dtype(mode))).cuda()
    mid = ops.conv_transpose(x, wct_T, cin, k, bias_taps=d["b_ct"].repeat(taps).cuda())
    unf = ops.conv3d_k3(mid, wrn_T, cout)
    e_fold, e_unf = rel_l2(got, ref), rel_l2(unf, ref)
    print(f"rel-L2 folded {e_fold:.4g}  unfolded {e_unf:.4g}  ratio {e_fold / e_unf:.3f}")
    assert e_unf < (2e-2 if mode == L4P_BF16 else 2e-3), e_unf  # (the yardstick itself is sane)
    assert e_fold <= e_unf, (e_fold, e_unf)


def test_subpixel_conv_rejects_what_the_kernels_do_not_take(dev):
    x = torch.zeros((1, 1, 4, 4, 64), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((2 * 128, 18 * 64), dtype=torch.bfloat16, device="cuda")
    ops.conv3d_subpixel(x, w, 128, (2, 1, 1))
    with pytest.raises(_lib.L4PHipError):  # an up-scaled axis of length 1: no border class
        ops.conv3d_subpixel(torch.zeros((1, 1, 1, 4, 64), dtype=torch.bfloat16, device="cuda"), w, 128, (2, 1, 1))
    with pytest.raises(_lib.L4PHipError):  # Cout not a multiple of the tile width
        ops.conv3d_subpixel(x, w, 64, (2, 1, 1))
    with pytest.raises(_lib.L4PHipError):  # weight rows shorter than the sub-positions' cells
        ops.conv3d_subpixel(x, torch.zeros((2 * 128, 8 * 64), dtype=torch.bfloat16, device="cuda"), 128, (2, 1, 1))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def mini():
    from l4p_amd.weights import ModelCfg, seeded_state_dict

    cfg = ModelCfg.mini()
    return cfg, seeded_state_dict(cfg)


@pytest.mark.parametrize("precision,tol_max,tol_l2", [("32-true", 1e-3, 1e-3), ("bf16", None, 3e-2), ("16-mixed", None, 4e-3)])
def test_decoder_takes_the_folded_form_by_knob(dev, knob, mini, precision, tol_max, tol_l2):
    from tests.golden_utils import make_batch
    from tests.test_encoder_dpt_gpu import build

    cfg, sd = mini
    model = build(cfg, sd, precision)
    clips = [make_batch(16, 2, seed=1234), make_batch(16, 2, seed=4321)]  # a batch of two clips
    batch = {k: torch.cat([c[k] for c in clips]) for k in clips[0]}
    tasks = ["depth", "camray"]
    keys = ("depth_est_b1thw", "traj3d_est_b16t")
    # the mini geometry at two clips: level 0 of depth is 131072 up-scaled voxels (its rn0 has the shape of the level's four
    # ResidualConvUnit convs: K = 27 * 256), level 1 is 32768 (rn1 alone has K = 27 * 512)
    out, tags = {}, {}
    for v in (2, 1, 0):  # 2: every up-scaling level; 1 (default): the levels whose three axes are up-scaled - depth, not camray; 0: none
        knob("dpt_fold_rn", v)
        with torch.no_grad(), prof_tags() as pt:
            out[v] = model.forward({k: t.clone() for k, t in batch.items()}, tasks)
        tags[v] = pt
    torch.cuda.synchronize()
    on, off = tags[2], tags[0]
    assert on.count("subpix") == 4 and off.count("subpix") == 0, (on.lines, off.lines)  # levels 0 and 1 of both heads
    assert tags[1].count("subpix") == 2 and tags[1].count("N512", "subpix") == 0 and tags[1].count("K13824 ") == 1  # camray unfolded
    assert torch.equal(out[1]["traj3d_est_b16t"], out[0]["traj3d_est_b16t"]) and torch.equal(out[1]["depth_est_b1thw"], out[2]["depth_est_b1thw"])
    assert on.count("M4096 N8192 K1152 ", "subpix") == 1 and on.count("M4096 N2048 K4096 ", "subpix") == 1  # depth
    assert on.count("M4096 N512 K4608 ", "subpix") == 1 and on.count("M4096 N512 K9216 ", "subpix") == 1    # camray, k = (2, 1, 1): 18 cells
    assert on.count("K13824 ") == 0 and off.count("M32768 N256 K13824 ") == 1       # rn1 of depth (and of camray: M8192)
    assert off.count("M131072 N256 K6912 ") - on.count("M131072 N256 K6912 ") == 1  # rn0 of depth
    assert off.count("M8192 N256 K13824 ") == 1 and off.count("M8192 N256 K6912 ") - on.count("M8192 N256 K6912 ") == 1  # camray
    for key in keys:
        a, b = out[2][key].float().cpu(), out[0][key].float().cpu()
        e = float((a - b).norm() / (b.norm() + 1e-30))
        print(f"{precision} {key}: rel-L2 folded vs unfolded {e:.3g}")
        assert e <= tol_l2, (key, e)
        if tol_max is not None:
            assert (a - b).abs().max() <= tol_max * b.abs().max(), key
