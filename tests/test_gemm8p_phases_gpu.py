"""The 8-phase GEMM's two main-loop bodies (csrc/gemm8p.hpp) are the same function, bit for bit: two phases of two C quadrants per k-tile
with predicate-free steady-state staging (knob gemm_8p_body = 1) against four phases of one quadrant (gemm_8p_body = 2).  Inside a
quadrant the k order is kept and every accumulator takes the k-tiles in order, so EVERY output element must be equal - torch.equal, no
tolerance - and the two-phase body must give the same bits on every one of ten launches: a misplaced fragment read or an early
re-stage shows up as a rare differing tile.

Knob gemm_variant = 10 admits small problems to the 8-phase kernel.  Shapes, the smallest at which each part of the loop can go wrong:
K = 64 (one k-tile: prologue and peeled k-tiles only), K = 128 / 192 (even / odd k-tile counts: both buffer parities at the end),
K = 352 (5.5 k-tiles: the K-tail tile; also under the mask-product epilogue), K = 1408 (the steady-state loop, 9 pairs), K = 136 with
row-mapped A; M = 300 and N = 264 (clamped rows and columns), N = 384 (256 x 192 tiles: filler W rows), N = 1408 (256 x 192 with a
ragged last column tile); every lean epilogue the 4 x 6 form takes, QKV at both small head geometries and the ConvTranspose scatter.
Each launch's profiler tag proves which body ran.  Both 16-bit types."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib, ops
from l4p_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, EPI_MASKDOT, L4P_BF16, L4P_F16, GemmDesc
from tests import gemm_forms_cases as G
from tests.test_gemm8p_gpu import prof_tags
from tests.test_gemm_forms_gpu import NAN, Run, _desc_ints, _padded, _stream, launches
from tests.test_kernels_gpu import as_mode, rnd

BODY = {1: "8p 2ph", 2: "8p 4ph"}
REPEATS = 10
MODES = pytest.mark.parametrize("mode", [L4P_BF16, L4P_F16], ids=["bf16", "f16"])


def _knobs(tile, body):
    return (("gemm_variant", 10), ("gemm_t192", 1 if tile == 192 else 0), ("gemm_8p_body", body))


def _form(tile, body):
    return f"{BODY[body]} t256x{tile}"


def _assert_same(two, four, what):
    """two: the outputs of each launch of the two-phase body, four: the four-phase body's"""
    for y in four:
        assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0.1, what
    for i, outs in enumerate(two):
        assert len(outs) == len(four)
        for a, b in zip(outs, four):
            assert torch.equal(a, b), (what, f"launch {i}", int((a != b).sum()), float((a.float() - b.float()).abs().max()))


# (M, N, K, tile, epilogue / row map)
T, F32 = "T", "f32"
DENSE = [(300, 264, k, 256, {}) for k in (64, 128, 192, 352, 1408)] + \
        [(300, 384, k, 192, {}) for k in (64, 128, 192, 352, 1408)] + \
        [(300, 1408, 256, 192, {}), (300, 1408, 1408, 192, {}),
         (300, 264, 136, 256, dict(rowmap=(100, 250, 50), outs=(F32,)))] + \
        [(300, 384, 192, 192, e) for e in (dict(act=ACT_GELU, outs=(T, F32)), dict(act=ACT_RELU, outs=(T, "relu")),
                                           dict(res=F32, outs=(F32,)), dict(res=T, outs=(T,)),
                                           dict(res=T, act=ACT_RELU, outs=(T, F32)), dict(res=T, res2=True, outs=(T, "relu")))]


def _dense_id(c):
    M, N, K, tile, e = c
    return f"{M}x{N}x{K}-t{tile}" + "".join(f"-{k}{'+'.join(v) if isinstance(v, tuple) and k == 'outs' else v}" for k, v in e.items())


@MODES
@pytest.mark.parametrize("shape", DENSE, ids=[_dense_id(c) for c in DENSE])
def test_dense_two_phase_body_equals_four_phase_body(dev, knob, mode, shape):
    M, N, K, tile, epi = shape
    case = G.Case("", M, N, K, mode, cls="gemm", **epi)
    runs = {body: Run(dataclasses.replace(case, form=_form(tile, body), knobs=_knobs(tile, body)), knob) for body in (2, 1)}
    def launch(body):  # (Run.launch asserts the one launch and its tag, the guards around [M, N] and that all of it was written)
        for name, value in _knobs(tile, body):
            knob(name, value)
        return [runs[body].launch().out(name).clone() for name in case.outs]

    four = launch(2)
    two = [launch(1) for _ in range(REPEATS)]
    _assert_same(two, four, _dense_id(shape))


QKV = [(geo, tile) for geo in ((1, 128, 3, 64), (2, 256, 2, 88)) for tile in (192, 256)]


@MODES
@pytest.mark.parametrize("geo,tile", QKV, ids=[f"{'x'.join(map(str, g))}-t{t}" for g, t in QKV])
def test_qkv_epilogue_two_phase_body_equals_four_phase_body(dev, knob, mode, geo, tile):
    B, S, H, Dh = geo
    td, HD = ops.torch_dtype(mode), H * ops.DP
    case = G.Case("", B * S, 3 * HD, H * Dh, mode, epi=1, geo=geo, cls="gemm")
    a, w, bias = G.operands(case)
    A, Wd, bd = _padded(a, 100.0), _padded(w, 100.0, rows=(case.N + 255) // 256 * 256), bias.cuda()
    d = _desc_ints(case)
    d.A, d.W, d.bias = A.data_ptr(), Wd.data_ptr(), bd.data_ptr()
    d.q_scale = Dh ** -0.5 * G.LOG2E

    def launch(body):
        for name, value in _knobs(tile, body):
            knob(name, value)
        q = torch.full((case.M, HD + G.PAD), NAN, dtype=td, device="cuda")
        kt, vt = (torch.full((case.M * HD,), NAN, dtype=td, device="cuda") for _ in range(2))
        d.out_T, d.k_tiled, d.vt = q.data_ptr(), kt.data_ptr(), vt.data_ptr()
        with prof_tags() as p:
            _lib.check(_lib.load().l4p_gemm(_stream(), mode, C.byref(d)), "l4p_gemm(qkv)")
        assert launches(p) == [("gemm", dataclasses.replace(case, form=_form(tile, body)).tag, 1)], p.lines
        return [q[:, :HD], kt, vt]

    four = launch(2)
    _assert_same([launch(1) for _ in range(REPEATS)], four, (geo, tile))


CONVT = [((2, 2, 2), 192), ((2, 2, 2), 256), ((2, 1, 1), 192)]


@MODES
@pytest.mark.parametrize("k,tile", CONVT, ids=[f"k{'x'.join(map(str, k))}-t{t}" for k, t in CONVT])
def test_conv_transpose_epilogue_two_phase_body_equals_four_phase_body(dev, knob, mode, k, tile):
    """L4P_EPI_CONVT: the pixel-shuffle scatter, cout = 72 (a tap boundary inside a wave's columns)"""
    td = ops.torch_dtype(mode)
    case = G.Case("", 1 * 4 * 8 * 8, k[0] * k[1] * k[2] * 72, 192, mode, epi=2, geo=(1, 4, 8, 8) + k + (72,), cls="gemm")
    a, w, bias = G.operands(case)
    A, Wd, bd = _padded(a, 100.0), _padded(w, 100.0, rows=(case.N + 255) // 256 * 256), bias.cuda()
    d = _desc_ints(case)
    d.A, d.W, d.bias = A.data_ptr(), Wd.data_ptr(), bd.data_ptr()

    def launch(body):
        for name, value in _knobs(tile, body):
            knob(name, value)
        out = torch.full((case.M * case.N,), NAN, dtype=td, device="cuda")
        d.out_T = out.data_ptr()
        with prof_tags() as p:
            _lib.check(_lib.load().l4p_gemm(_stream(), mode, C.byref(d)), "l4p_gemm(convT)")
        assert launches(p) == [("gemm", dataclasses.replace(case, form=_form(tile, body)).tag, 1)], p.lines
        return [out]

    four = launch(2)
    _assert_same([launch(1) for _ in range(REPEATS)], four, (k, tile))


@MODES
def test_mask_product_epilogue_two_phase_body_equals_four_phase_body(dev, knob, mode):
    """L4P_EPI_MASKDOT at the mask product's K = 352 (5.5 k-tiles: one steady pair, then the peeled k-tiles with the K-tail): M = 384,
    N = 4 x 64; the float partial sums [chunk][3][M] are the output"""
    Nq, T_, h, w_, Cin, d1 = 3, 2, 8, 8, 352, 40
    d1p, M = 64, Nq * T_ * h * w_
    x, _ = as_mode(rnd((M, Cin), 190), mode)
    wp, _ = as_mode(rnd((4 * d1p, Cin), 191, Cin ** -0.5), mode)
    wpad = ops.pad_rows(wp, 256)
    bp = rnd((4 * d1p,), 192).cuda()
    hp = rnd((Nq, 3, d1p), 193).cuda()
    d = GemmDesc()
    d.A, d.lda, d.W, d.ldw = x.data_ptr(), Cin, wpad.data_ptr(), Cin
    d.M, d.N, d.K = M, 4 * d1p, Cin
    d.bias, d.act = bp.data_ptr(), ACT_GELU
    d.epi, d.Cout = EPI_MASKDOT, d1p
    d.hyper, d.hyper_rows = hp.data_ptr(), M // Nq

    def launch(body):
        for name, value in _knobs(256, body):
            knob(name, value)
        partial = torch.full((4 * (d1p // 32), 3, M), NAN, dtype=torch.float32, device="cuda")
        d.out_f32 = partial.data_ptr()
        with prof_tags() as p:
            _lib.check(_lib.load().l4p_gemm(_stream(), mode, C.byref(d)), "l4p_gemm(maskdot)")
        assert launches(p) == [("gemm", f"M{M} N{4 * d1p} K{Cin} epi{EPI_MASKDOT} act{ACT_GELU} {_form(256, body)}", 1)], p.lines
        return [partial]

    four = launch(2)
    _assert_same([launch(1) for _ in range(REPEATS)], four, "maskdot")
