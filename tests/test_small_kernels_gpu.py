"""Unit parity of the tracker / DPT kernels that had no direct test, against the float64 references of tests/kernel_refs.py.

The references are checked on the CPU (tests/test_kernel_refs_cpu.py: against torch's float64 ops and oracle/l4p_oracle.py);
here the HIP kernels are checked against them, through l4p_amd.ops where a wrapper exists and through the C ABI (ctypes)
otherwise.  Inputs are rounded to the engine type first and the reference sees the same rounded values in float64.  Every shape is
chosen to reach one host-side dispatch branch or index path of a launcher; the comment beside it says which.

Tolerances: `check()` of tests/test_kernels_gpu.py (the project's stated bounds) wherever a result is not exact, plus
  * up-sampling, f32 engine: max abs <= 1e-5 max|ref| against the float32-index reference (eight float products and sums of values
    <= max stay below 16 * 2^-24 ~ 1e-6; a factor 10 for a weight that differs in its last bit).  MEASURED on MI355X: see UPS_F32_SEEN.
  * up-sampling, 16-bit engines: every output within one output ulp of the float64 value rounded to T (same-sign taps, see there).
  * track_tokens' sin / cos row: TOKENS_PE_GATE, a measured gate with a derived floor (see there).
No case is skipped: a launcher that refuses a shape is asserted to return L4P_E_INVALID before any launch.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib, ops
from l4p_amd._lib import ACT_GELU, ACT_NONE, L4P_F32
from tests import kernel_refs as R
from tests.test_kernels_gpu import MODES, as_mode, check, rnd

E_INVALID = _lib.L4P_E_INVALID
SENT = 0xA5     # sentinel byte of pre-filled buffers


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr()


def sentinel(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def is_sentinel(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def report(what, value):
    print(f"[measured] {what}: {value:.3e}")


# ------------------------------------------------------------------------------------------------
# l4p_upsample_trilinear
# ------------------------------------------------------------------------------------------------
UPS_F32_SEEN = 1.8e-7  # largest max|y - ref| / max|ref| of the f32 engine over UPSAMPLE_CASES, measured on MI355X (float round-off; < 2e-6)


def _ups_check(y, ref, mode, ulp_gate):
    y64 = y.double().cpu()
    scale = ref.abs().max().item()
    err = (y64 - ref).abs().max().item()
    report(f"upsample mode {mode} max err / max|ref|", err / scale)
    if mode == L4P_F32:
        assert err <= 1e-5 * scale, f"max err {err:.3e} vs scale {scale:.3e}"
        return
    check(y, ref, mode, True)
    if ulp_gate:
        r = ref.to(ops.torch_dtype(mode)).double()
        over = (y64 - r).abs() - R.ulp_of(r, ops.torch_dtype(mode))
        assert bool((over <= 0).all()), f"{int((over > 0).sum())} outputs further than one ulp from the rounded float64 value"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,isz,osz,C,align", R.UPSAMPLE_CASES, ids=[c[0] for c in R.UPSAMPLE_CASES])
def test_upsample_vs_float64(dev, mode, name, B, isz, osz, C, align):
    """Every branch of launch_upsample (R.UPSAMPLE_CASES says which case reaches which) against trilinear_ref with the float32 index.
    Signed data: check() / the f32 gate.  16-bit engines additionally on POSITIVE data, where the one-ulp statement is well posed:
    a convex combination of same-sign taps cannot cancel, so the float accumulation error (<= 8 float ulps of the largest tap) stays far
    below an output ulp of the result and the kernel's value is the float64 value rounded once, or its neighbour."""
    x = rnd((B, *isz, C), 100)
    xd, xr = as_mode(x, mode)
    y = ops.upsample_trilinear(xd, osz, align)
    torch.cuda.synchronize()
    _ups_check(y, R.trilinear_ref(xr, osz, align, np.float32), mode, False)
    if mode != L4P_F32:
        xd, xr = as_mode(x.abs() + 0.25, mode)
        y = ops.upsample_trilinear(xd, osz, align)
        torch.cuda.synchronize()
        _ups_check(y, R.trilinear_ref(xr, osz, align, np.float32), mode, True)


def test_upsample_lines_past_65535_are_written(dev):
    """Case f again, by position: the lines with blockIdx.z = 1 (line >= 65 535) of a sentinel-filled output are all written."""
    name, B, isz, osz, C, align = next(c for c in R.UPSAMPLE_CASES if c[0] == "f_lines_z1")
    assert B * osz[0] * osz[1] >= 70000
    xd, _ = as_mode(rnd((B, *isz, C), 101), L4P_F32)
    y = sentinel((B * osz[0] * osz[1], osz[2] * C), torch.float32)
    rc = lib().l4p_upsample_trilinear(st(), L4P_F32, ptr(xd), ptr(y), B, *isz, *osz, C, int(align))
    torch.cuda.synchronize()
    assert rc == 0
    untouched = (y.view(torch.uint8) == SENT).all(dim=1)
    assert not bool(untouched.any()), f"lines never written: first {int(untouched.nonzero()[0])}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("align", [True, False])
def test_upsample_identity_is_bitwise(dev, mode, align):
    """(h) equal sizes: the source coordinate is the destination's, every weight 0 or 1 - the output equals the input bit for bit.
    (ops.upsample_trilinear returns its input without a launch: the entry point is called directly.)"""
    B, sz, C = 2, (3, 5, 7), 16
    xd, _ = as_mode(rnd((B, *sz, C), 102), mode)
    y = sentinel(xd.shape, xd.dtype)
    rc = lib().l4p_upsample_trilinear(st(), mode, ptr(xd), ptr(y), B, *sz, *sz, C, int(align))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(bits(y), bits(xd))


@pytest.mark.parametrize("mode", MODES)
def test_upsample_refuses_channels_not_multiple_of_8(dev, mode):
    """launch_upsample returns before any launch when C % 8 != 0."""
    xd, _ = as_mode(rnd((1, 2, 2, 2, 12), 103), mode)
    y = sentinel((1, 2, 4, 4, 12), xd.dtype)
    rc = lib().l4p_upsample_trilinear(st(), mode, ptr(xd), ptr(y), 1, 2, 2, 2, 2, 4, 4, 12, 1)
    torch.cuda.synchronize()
    assert rc == E_INVALID and is_sentinel(y)


# ------------------------------------------------------------------------------------------------
# l4p_head_out
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("vox", R.HEAD_OUT_VOX)
def test_head_out_vs_float64(dev, mode, vox):
    """head_out_lds_kernel (16-bit) / head_out_kernel (f32): vox_per_b = 768 whole tiles; 1000: with B = 3 the 256-row tiles straddle the
    batch boundaries and the last one is ragged (nrow = 184 masks lanes inside the LDS-DMA instruction); 255 and 1: a single ragged
    tile; Cout 1 .. 8, with and without exp (checked on the LOG of the output so small values are not hidden under a large maximum)."""
    for B in R.HEAD_OUT_B:
        xd, xr = as_mode(rnd((B, 1, 1, vox, 128), 200 + B), mode)
        for cout in R.HEAD_OUT_COUT:
            w, b = rnd((cout, 128), 210 + cout, 1.5 * 128 ** -0.5), rnd((cout,), 220 + cout, 0.3)
            lin = R.head_out_ref(xr.reshape(B, vox, 128), w, b, 0)
            assert lin.max().item() < math.log(1e4)
            for post_exp in (0, 1):
                y = ops.head_out(xd, w.cuda(), b.cuda(), bool(post_exp)).reshape(B, cout, vox)
                torch.cuda.synchronize()
                if post_exp:
                    ex = R.head_out_ref(xr.reshape(B, vox, 128), w, b, 1)
                    assert bool((y.cpu() > 0).all())
                    check(torch.log(y.double().cpu()), lin, mode, False)
                    check(y, ex, mode, False)
                else:
                    check(y, lin, mode, False)


def test_head_out_f32_grid_stride(dev):
    """The f32 kernel's grid is capped at 8192 blocks of 256: with more voxels a thread strides.  The input is a 65 521-row block
    (a prime: no alignment with the 2 097 152-voxel stride) repeated, so the reference is formed once for the block."""
    vox, blk, cout = 8192 * 256 + 300, 65521, 3
    xb, xr = as_mode(rnd((blk, 128), 230), L4P_F32)
    reps = (vox + blk - 1) // blk
    xd = xb.repeat(reps, 1)[:vox].contiguous().reshape(1, 1, 1, vox, 128)
    w, b = rnd((cout, 128), 231, 128 ** -0.5), rnd((cout,), 232)
    y = ops.head_out(xd, w.cuda(), b.cuda(), False).reshape(cout, vox)
    torch.cuda.synchronize()
    ref = R.head_out_ref(xr.reshape(1, blk, 128), w, b, 0)[0].repeat(1, reps)[:, :vox]
    check(y, ref, L4P_F32, False)


def _one_hot_rows(rows, C, mode):
    """Row r is zero except a one at channel (7 r + r / C) % C: walks every channel, and every 16-byte chunk position per row residue."""
    r = torch.arange(rows)
    ch = (7 * r + r // C) % C
    x = torch.zeros(rows, C)
    x[r, ch] = 1.0
    return x.to(ops.torch_dtype(mode)).cuda(), ch


@pytest.mark.parametrize("mode", MODES)
def test_head_out_positioned_input_is_exact(dev, mode):
    """The XOR swizzle of head_out_lds_kernel by position: one channel per voxel is one, w[o][c] = c + 128 o, so the output NAMES the
    channel each thread read (a wrong chunk shows as a shifted channel index, not as 'wrong numbers').  Small integers: exact in all
    three engines.  vox_per_b = 1000, B = 3: straddling and ragged tiles included."""
    B, vox, cout = 3, 1000, 8
    xd, ch = _one_hot_rows(B * vox, 128, mode)
    w = (torch.arange(128.0)[None, :] + 128.0 * torch.arange(float(cout))[:, None]).contiguous()
    y = ops.head_out(xd.reshape(B, 1, 1, vox, 128), w.cuda(), torch.zeros(cout).cuda(), False).reshape(B, cout, vox)
    torch.cuda.synchronize()
    want = ch.reshape(B, 1, vox).float() + 128.0 * torch.arange(float(cout)).reshape(1, cout, 1)
    got = y.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"first mismatch (b, o, voxel) {bad[0].tolist()}: read channel {got[tuple(bad[0])] % 128}, want {want[tuple(bad[0])] % 128}"


# ------------------------------------------------------------------------------------------------
# l4p_small_attn kinds 1 - 4, l4p_t2i_attn_scores
# ------------------------------------------------------------------------------------------------
def _attn(mode, kind, q, k, v, out, N, P, D, heads):
    rc = lib().l4p_small_attn(st(), mode, kind, ptr(q), ptr(k), ptr(v), ptr(out), N, P, D, heads)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,P,D,heads", R.ATTN_SHAPES)
def test_small_attn_kinds_1_to_4_vs_float64(dev, mode, N, P, D, heads):
    """t2i_attn_kernel (kinds 1 / 3), i2t_attn_lds_kernel / i2t_attn_kernel (kinds 2 / 4) and the scores-passed-in form
    (l4p_t2i_attn_scores) against small_attn_ref; R.ATTN_SHAPES says which shape reaches which branch, and tests/test_track_select_cpu.py
    asserts the kernel form, grid and LDS size of every (kind, shape, engine) here on the host.  Kinds 3 / 4 differ from 1 / 2 by a
    zero stride only: equal to the per-track call on replicated operands BIT FOR BIT."""
    T = ops.torch_dtype(mode)
    q6, q6r = as_mode(rnd((N, 6, D), 300), mode)
    kim, kimr = as_mode(rnd((N, P, D), 301), mode)
    vim, vimr = as_mode(rnd((N, P, D), 302), mode)
    qim, qimr = as_mode(rnd((N, P, D), 303), mode)
    k6, k6r = as_mode(rnd((N, 6, D), 304), mode)
    v6, v6r = as_mode(rnd((N, 6, D), 305), mode)
    # kind 1
    o1 = sentinel((N, 6, D), T)
    assert _attn(mode, 1, q6, kim, vim, o1, N, P, D, heads) == 0
    check(o1, R.small_attn_ref(1, q6r, kimr, vimr, heads), mode, True)
    # kind 3 == kind 1 on replicated K / V
    rep = lambda t: t[0:1].expand(N, -1, -1).contiguous()
    o3, o1r = sentinel((N, 6, D), T), sentinel((N, 6, D), T)
    assert _attn(mode, 3, q6, kim[0].contiguous(), vim[0].contiguous(), o3, N, P, D, heads) == 0
    assert _attn(mode, 1, q6, rep(kim), rep(vim), o1r, N, P, D, heads) == 0
    assert torch.equal(bits(o3), bits(o1r))
    check(o3, R.small_attn_ref(3, q6r, kimr[0], vimr[0], heads), mode, True)
    # kind 2
    o2 = sentinel((N, P, D), T)
    assert _attn(mode, 2, qim, k6, v6, o2, N, P, D, heads) == 0
    check(o2, R.small_attn_ref(2, qimr, k6r, v6r, heads), mode, True)
    # kind 4 == kind 2 on replicated Q
    o4, o2r = sentinel((N, P, D), T), sentinel((N, P, D), T)
    assert _attn(mode, 4, qim[0].contiguous(), k6, v6, o4, N, P, D, heads) == 0
    assert _attn(mode, 2, rep(qim), k6, v6, o2r, N, P, D, heads) == 0
    assert torch.equal(bits(o4), bits(o2r))
    check(o4, R.small_attn_ref(4, qimr[0], k6r, v6r, heads), mode, True)
    # scores passed in (`pre`): a float32 cast of the reference scores, rows padded to ld = 6 heads + 4 with garbage never read
    ld = 6 * heads + 4
    s32 = torch.full((N, P, ld), 1e30)
    s32[:, :, :6 * heads] = R.t2i_scores_ref(q6r, kimr, heads).float()
    o5, s32d = sentinel((N, 6, D), T), s32.cuda()
    rc = lib().l4p_t2i_attn_scores(st(), mode, ptr(s32d), ld, ptr(vim), ptr(o5), N, P, D, heads)
    torch.cuda.synchronize()
    assert rc == 0
    check(o5, R.t2i_from_scores_ref(s32, vimr, heads), mode, True)


@pytest.mark.parametrize("mode", MODES)
def test_t2i_softmax_peaked_key_owned_by_the_fourth_wave(dev, mode):
    """The max-subtraction of t2i_attn_kernel's softmax.  A softmax is shift invariant, so a wrong block maximum only shows once
    exp(score - maximum) overflows: one key row p with p % 256 >= 192 (thread p % 256 scans it: the FOURTH wave owns the maximum) is
    8 x token 0's query, with queries of deviation 2 - its score against token 0 is 8 |q_h|^2 / sqrt(hd) ~ 180, the others' stay near
    +-8: a maximum formed without the fourth wave's makes exp overflow to inf.  Kind 1 and the scores-passed-in form."""
    N, P, D, heads = 2, 1000, 256, 8
    p_peak = 2 * 256 + 200
    q = rnd((N, 6, D), 310, 2.0)
    k = rnd((N, P, D), 311)
    k[:, p_peak] = 8.0 * q[:, 0]
    q6, q6r = as_mode(q, mode)
    kim, kimr = as_mode(k, mode)
    vim, vimr = as_mode(rnd((N, P, D), 312), mode)
    s = R.t2i_scores_ref(q6r, kimr, heads)
    top2 = s[:, :, :heads].topk(2, dim=1).values  # token 0's columns
    assert bool((top2[:, 0] - top2[:, 1] > 100).all()) and bool((s[:, p_peak, :heads] == top2[:, 0]).all())
    ref = R.small_attn_ref(1, q6r, kimr, vimr, heads)
    o1 = sentinel((N, 6, D), ops.torch_dtype(mode))
    assert _attn(mode, 1, q6, kim, vim, o1, N, P, D, heads) == 0
    assert bool(torch.isfinite(o1.float()).all())
    check(o1, ref, mode, True)
    s32 = s.float()
    o5, s32d = sentinel((N, 6, D), ops.torch_dtype(mode)), s32.contiguous().cuda()
    rc = lib().l4p_t2i_attn_scores(st(), mode, ptr(s32d), 6 * heads, ptr(vim), ptr(o5), N, P, D, heads)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(o5.float()).all())
    check(o5, R.t2i_from_scores_ref(s32, vimr, heads), mode, True)


@pytest.mark.parametrize("mode", MODES)
def test_small_attn_refused_shapes_write_nothing(dev, mode):
    """launch_small_attn returns L4P_E_INVALID before any launch for hd > 96 (kinds >= 1: the encoder width 1408 / 8 = 176) and for
    P % 4 != 0 (kinds 1 / 3); launch_t2i_attn_scores likewise.  The sentinel-filled output is unchanged."""
    T = ops.torch_dtype(mode)
    for kind, N, P, D, heads in [(1, 2, 64, 1408, 8), (2, 2, 64, 1408, 8), (3, 2, 64, 1408, 8), (4, 2, 64, 1408, 8),
                                 (1, 2, 98, 352, 4), (3, 2, 98, 352, 4), (1, 2, 64, 100, 3)]:
        big = torch.zeros((N, max(P, 6), D), dtype=T, device="cuda")
        out = sentinel((N, max(P, 6), D), T)
        assert _attn(mode, kind, big, big, big, out, N, P, D, heads) == E_INVALID, (kind, P, D, heads)
        assert is_sentinel(out)
    N, P, D, heads = 2, 98, 352, 4
    v, out = torch.zeros((N, P, D), dtype=T, device="cuda"), sentinel((N, 6, D), T)
    s = torch.zeros((N, P, 6 * heads), device="cuda")
    for args in [(6 * heads, N, P, D, heads), (6 * heads - 1, N, 96, D, heads), (48, N, 96, 1408, 8)]:
        assert lib().l4p_t2i_attn_scores(st(), mode, ptr(s), args[0], ptr(v), ptr(out), *args[1:]) == E_INVALID, args
    torch.cuda.synchronize()
    assert is_sentinel(out)


# ------------------------------------------------------------------------------------------------
# l4p_mask_product
# ------------------------------------------------------------------------------------------------
def _mask_product(mode, up, hyper, N, vox, C):
    masks = sentinel((N, 3, vox), torch.float32)
    rc = lib().l4p_mask_product(st(), mode, ptr(up), ptr(hyper), ptr(masks), N, vox, C)
    torch.cuda.synchronize()
    assert rc == 0
    return masks


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", R.MASK_PRODUCT_C)
def test_mask_product_vs_float64(dev, mode, C):
    """launch_mask_product takes the LDS kernel while 3 C floats + a 128-voxel tile fit 160 KB and the direct kernel otherwise: by that
    size rule the f32 engine with C = 352 (4224 + 128 * 352 * 4 = 184 448 bytes) runs mask_product_kernel and every other (engine, C)
    here mask_product_lds_kernel.  Both carry the profiler tag "mask_product": which kernel each (engine, C, vox, N) here reaches, with
    its grid and LDS size, is asserted on the host by tests/test_track_select_cpu.py (csrc/track_select.hpp mask_product_select).
    vox = 640: whole tiles; 1000: ragged last tile (104 voxels; LDS-DMA chunks masked by c + tid < chunks); 7: one short tile."""
    for vox in R.MASK_PRODUCT_VOX:
        for N in R.MASK_PRODUCT_N:
            up, upr = as_mode(rnd((N, vox, C), 400 + N), mode)
            hyper = rnd((N, 3, C), 410 + N, C ** -0.5)
            hd_ = hyper.cuda()
            masks = _mask_product(mode, up, hd_, N, vox, C)
            check(masks, R.mask_product_ref(upr, hyper), mode, False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", R.MASK_PRODUCT_C)
def test_mask_product_positioned_input_is_exact(dev, mode, C):
    """One channel per voxel is one and hyper[n][m][c] = c + C m + n: the output names the channel every thread read from its LDS row
    (or global row).  Exact: small integers."""
    N, vox = 3, 1000
    up, ch = _one_hot_rows(N * vox, C, mode)
    hyper = (torch.arange(float(C)).reshape(1, 1, C) + C * torch.arange(3.0).reshape(1, 3, 1) + torch.arange(float(N)).reshape(N, 1, 1)).contiguous()
    hd_ = hyper.cuda()
    masks = _mask_product(mode, up, hd_, N, vox, C).cpu()
    want = ch.reshape(N, 1, vox).float() + C * torch.arange(3.0).reshape(1, 3, 1) + torch.arange(float(N)).reshape(N, 1, 1)
    bad = (masks != want).nonzero()
    assert bad.numel() == 0, f"first mismatch (n, m, voxel) {bad[0].tolist()}: got {masks[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def test_dynamic_lds_limit_small_then_over_64k_then_small(dev):
    """The three kernels whose dynamic LDS size follows the geometry and whose launchers raise MaxDynamicSharedMemorySize through
    lds_attr_once: each is launched at a small size, at one above the 64 KB default and at the small size again; every launch
    returns 0 and passes the gate its kernel's parity test uses, whatever ran before in the process (the limit is only ever
    raised).  Sizes by the launchers' own formulas:
      * mask_product_lds_kernel, VT = 128: round16(3 C 4) + 128 C es.  C = 8: 96 + 1024 es; bf16 / f16 C = 352: 4224 + 90112 =
        94336; f32 C = 128: 1536 + 65536 = 67072 (both below the 160 KB switch to the direct kernel).  vox = 130: a ragged tile.
      * t2i_attn_kernel (kind 1), heads = 1, hd = D = 4: (6 P + 832) 4, plus 256 * 6 * 4 * 4 - 24 P when that is positive.
        P = 8: 3520 + 24384 = 27904; P = 2688: 67840.
      * i2t_attn_lds_kernel (kind 2), f32, heads = 1 (256 rows): round16(48 D) + 1024 D.  D = 4: 4288; D = 64: 68608."""
    for mode in MODES:
        big_C = 128 if mode == L4P_F32 else 352
        for C in (8, big_C, 8):
            N, vox = 2, 130
            up, upr = as_mode(rnd((N, vox, C), 420), mode)
            hyper = rnd((N, 3, C), 421, C ** -0.5)
            check(_mask_product(mode, up, hyper.cuda(), N, vox, C), R.mask_product_ref(upr, hyper), mode, False)
        for P in (8, 2688, 8):
            N, D, heads = 1, 4, 1
            q6, q6r = as_mode(rnd((N, 6, D), 422), mode)
            kim, kimr = as_mode(rnd((N, P, D), 423), mode)
            vim, vimr = as_mode(rnd((N, P, D), 424), mode)
            o1 = sentinel((N, 6, D), ops.torch_dtype(mode))
            assert _attn(mode, 1, q6, kim, vim, o1, N, P, D, heads) == 0, (mode, P)
            check(o1, R.small_attn_ref(1, q6r, kimr, vimr, heads), mode, True)
    for D in (4, 64, 4):
        N, P, heads = 2, 8, 1
        qim, qimr = as_mode(rnd((N, P, D), 425), L4P_F32)
        k6, k6r = as_mode(rnd((N, 6, D), 426), L4P_F32)
        v6, v6r = as_mode(rnd((N, 6, D), 427), L4P_F32)
        o2 = sentinel((N, P, D), torch.float32)
        assert _attn(L4P_F32, 2, qim, k6, v6, o2, N, P, D, heads) == 0, D
        check(o2, R.small_attn_ref(2, qimr, k6r, v6r, heads), L4P_F32, True)


# ------------------------------------------------------------------------------------------------
# l4p_layernorm_ex
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm_ex_vs_float64(dev, mode, M, C):
    """layernorm_kernel with the tracker's extras: addend periods M, 6 and 5 (5 divides neither 37 nor 2048; C = 1540 and 2048: the 8-slot instantiations), GELU applied BEFORE the
    addend, every combination of out_T / out_f32 / out_T2 being null or not (out_T2 without out_T included).  M = 37 and 6 are no
    multiple of the four rows a workgroup takes: two guard rows behind every output must keep their sentinel.  out_T of a launch
    with the addend equals the launch without it bit for bit."""
    T = ops.torch_dtype(mode)
    x = rnd((M, C), 500, 3.0) + 0.5
    g, b = rnd((C,), 501, 0.2) + 1.0, rnd((C,), 502, 0.1)
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()

    def launch(want_T, want_f, want_T2, add, am, act):
        oT = sentinel((M + 2, C), T) if want_T else None
        of = sentinel((M + 2, C), torch.float32) if want_f else None
        oT2 = sentinel((M + 2, C), T) if want_T2 else None
        rc = lib().l4p_layernorm_ex(st(), mode, ptr(xd), ptr(gd), ptr(bd), 1e-5, ptr(oT), ptr(of), M, C, ptr(add) if want_T2 else None,
                                    am if want_T2 else 0, ptr(oT2), act)
        torch.cuda.synchronize()
        assert rc == 0
        for o in (oT, of, oT2):
            assert o is None or is_sentinel(o[M:])
        return oT, of, oT2

    for act in (ACT_NONE, ACT_GELU):
        plain_T, _, _ = launch(True, False, False, None, 0, act)
        for am in R.LN_ADD_MODS:
            am = M if am == "M" else am
            add = rnd((am, C), 503 + am)
            y, y2 = R.layernorm_ex_ref(x, g, b, 1e-5, add, am, act)
            addd = add.cuda()
            for want_T in (False, True):
                for want_f in (False, True):
                    for want_T2 in (False, True):
                        oT, of, oT2 = launch(want_T, want_f, want_T2, addd, am, act)
                        if want_T:
                            check(oT[:M], y, mode, True)
                            assert torch.equal(bits(oT[:M]), bits(plain_T[:M]))
                        if want_f:
                            check(of[:M], y, mode, False)
                        if want_T2:
                            check(oT2[:M], y2, mode, True)


# ------------------------------------------------------------------------------------------------
# l4p_track_tokens
# ------------------------------------------------------------------------------------------------
# The sin / cos row: the only inexact pieces are the float32 argument 2 pi a (a = c_t g_t + c_x g_x + c_y g_y: three float products and
# two sums of terms up to a few units) and sinf / cosf.  Floor (derived): max|2 pi a| * 2^-23.  Cap: 1e-4 - the values are of order 1
# and a wrong frequency index gives errors of order 1.  MEASURED on MI355X against the float64 reference fed the same float32 inputs:
# worst |error| TOKENS_PE_SEEN; the gate is 4 x that (fixed seeds: no run-to-run spread, the margin covers compiler / ROCm changes).
TOKENS_PE_SEEN = 3.0e-6  # (N 7, C 1408; the floor of that case is 4.1e-6)
TOKENS_PE_GATE = 4 * TOKENS_PE_SEEN


@pytest.mark.parametrize("N,C", R.TOKENS_CASES)
def test_track_tokens_vs_float64(dev, N, C):
    """track_tokens_kernel: labels / plabel drawn from {0, 1, 2, -1} meet every branch of the two `if` chains, "neither" included (the PE
    is left alone, the feature row stays zero); queries on the borders (t = 0.5, x = W - 0.5).  Everything but the sin / cos row is
    exact (copies and single float adds)."""
    Tt, H, W = 16, 224, 208
    g = torch.Generator().manual_seed(600 + N)
    queries = torch.rand((N, 3), generator=g) * torch.tensor([float(Tt), float(W), float(H)])
    queries[0] = torch.tensor([0.5, W - 0.5, 0.5])
    label_sets = [([2.0], [2.0]), ([0.0], [1.0]), ([1.0], [0.0]), ([-1.0], [-1.0])] if N == 1 else \
        [([0.0, 1.0, 2.0, -1.0, 0.0, 1.0, 2.0], [1.0, 0.0, -1.0, 2.0, 0.0, 1.0, -1.0])]
    gauss, mtok = rnd((3, C // 2), 601), rnd((3, C), 602)
    pe0, pe1, nap, fe0, fe1 = (rnd((C,), 603 + i) for i in range(5))
    pfeat = rnd((N, C), 608)
    for labels, plabel in label_sets:
        labels, plabel = torch.tensor(labels), torch.tensor(plabel)
        tokens = sentinel((N + 1, 6, C), torch.float32)
        args = [t.cuda().contiguous() for t in (queries, labels, pfeat, plabel, gauss, mtok, pe0, pe1, nap, fe0, fe1)]  # (kept alive)
        rc = lib().l4p_track_tokens(st(), *[ptr(t) for t in args], ptr(tokens), N, C, Tt, H, W)
        torch.cuda.synchronize()
        assert rc == 0 and is_sentinel(tokens[N:])
        got = tokens[:N].cpu()
        ref = R.track_tokens_ref(queries, labels, pfeat, plabel, gauss, mtok, pe0, pe1, nap, fe0, fe1, Tt, H, W)
        for row in (0, 1, 2, 4, 5):
            assert torch.equal(got[:, row], ref[:, row].float()), f"token {row}"
        # the argument of the sin / cos row, for the derived floor
        c = 2.0 * torch.stack([queries[:, 0] / Tt, queries[:, 1] / W, queries[:, 2] / H], -1).double() - 1.0
        floor = (2.0 * math.pi * (c @ gauss.double()).abs().max().item()) * 2.0 ** -23
        err = (got[:, 3].double() - ref[:, 3]).abs().max().item()
        report(f"track_tokens N{N} C{C} sin/cos row max err (floor {floor:.2e})", err)
        assert floor <= TOKENS_PE_GATE <= 1e-4
        assert err <= TOKENS_PE_GATE, f"sin / cos row: {err:.3e}"


# ------------------------------------------------------------------------------------------------
# l4p_track_keys_init
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shared_from", [0, 32, 64])
def test_track_keys_init_values_and_untouched_rows(dev, mode, shared_from):
    """track_keys_init_kernel: with shared_from > 0 tracks >= 1 leave rows >= shared_from UNWRITTEN in k32 / kT / kP (the sentinel
    survives) and k32_shared holds track 0's float rows; shared_from = P: nothing shared (k32_shared untouched).  Values are exact: k32 is
    one float add, kT / kP torch's round-to-nearest-even of the float sums."""
    N, P, C = 3, 64, 352
    T = ops.torch_dtype(mode)
    enc, hist, pos = rnd((P, C), 700), rnd((N, P, C), 701), rnd((P, C), 702)
    k, kp, written, shared = R.keys_init_ref(enc, hist, pos, shared_from)
    k32, kT, kP = sentinel((N, P, C), torch.float32), sentinel((N, P, C), T), sentinel((N, P, C), T)
    ksh = sentinel((P, C), torch.float32)
    encd, histd, posd = enc.cuda(), hist.cuda(), pos.cuda()
    rc = lib().l4p_track_keys_init(st(), mode, ptr(encd), ptr(histd), ptr(posd), ptr(k32), ptr(kT), ptr(kP), N, P, C, shared_from, ptr(ksh))
    torch.cuda.synchronize()
    assert rc == 0
    w = written.cuda()
    assert torch.equal(bits(k32[w]), bits(k.float().cuda()[w]))
    assert torch.equal(bits(kT[w]), bits(k.float().to(T).cuda()[w]))
    assert torch.equal(bits(kP[w]), bits(kp.float().to(T).cuda()[w]))
    for buf in (k32, kT, kP):
        assert is_sentinel(buf[~w]) or not bool((~w).any())
    if shared_from > 0:
        ns = P - shared_from
        assert torch.equal(bits(ksh[:ns]), bits(shared.float().cuda())) or ns == 0
        assert is_sentinel(ksh[ns:])
        assert int((~written).sum()) == (N - 1) * ns
    else:
        assert is_sentinel(ksh) and bool(written.all())


@pytest.mark.parametrize("mode", MODES)
def test_track_keys_init_refused_arguments(dev, mode):
    """launch_track_keys_init checks shared_from in [0, P], k32_shared present when shared_from > 0 and C % 8 == 0 before it launches."""
    N, P, C = 2, 16, 32
    T = ops.torch_dtype(mode)
    src = torch.zeros((N, P, C), device="cuda")
    k32, kT, kP, ksh = sentinel((N, P, C), torch.float32), sentinel((N, P, C), T), sentinel((N, P, C), T), sentinel((P, C), torch.float32)
    call = lambda sf, sh, c=C: lib().l4p_track_keys_init(st(), mode, ptr(src), ptr(src), ptr(src), ptr(k32), ptr(kT), ptr(kP), N, P, c, sf, sh)
    assert call(-1, ptr(ksh)) == E_INVALID
    assert call(P + 1, ptr(ksh)) == E_INVALID
    assert call(8, None) == E_INVALID
    assert call(0, ptr(ksh), 12) == E_INVALID
    torch.cuda.synchronize()
    assert all(is_sentinel(t) for t in (k32, kT, kP, ksh))


# ------------------------------------------------------------------------------------------------
# l4p_fill_rows, l4p_broadcast_block
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("nbytes", [16, 16 * 1000])
def test_fill_rows_and_broadcast_block_bytes(dev, n, nbytes):
    """fill_rows_kernel with a row map (group_rows 3 < group_stride 7, offset 2) and broadcast_block_kernel (offset 48 inside groups
    96 bytes longer than the block): byte-exact against the references, everything outside the written region unchanged."""
    rs = np.random.RandomState(800 + n)
    gr, gs, go, C = 3, 7, 2, nbytes // 4
    buf = rs.randint(0, 256, size=(n * gs + 1) * nbytes).astype(np.uint8)
    v = rs.randint(0, 256, size=nbytes).astype(np.uint8)
    out, vd = torch.from_numpy(buf).cuda(), torch.from_numpy(v).cuda()
    rc = lib().l4p_fill_rows(st(), ptr(out), ptr(vd), n * gr, C, gr, gs, go)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(out.cpu().numpy(), R.fill_rows_ref(buf, v, n * gr, nbytes, gr, gs, go))
    off, stride = 48, nbytes + 96
    buf = rs.randint(0, 256, size=n * stride + 32).astype(np.uint8)
    base = torch.from_numpy(buf).cuda()
    rc = lib().l4p_broadcast_block(st(), ptr(base), off, nbytes, stride, n)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(base.cpu().numpy(), R.broadcast_block_ref(buf, off, nbytes, stride, n))


def test_broadcast_block_refuses_misaligned_arguments(dev):
    """launch_broadcast_block checks base, off, bytes and stride for 16-byte multiples before it launches.  (launch_fill_rows checks
    nothing: no refused case is passed to it.)"""
    base = sentinel((4096,), torch.uint8)
    for off, nbytes, stride, shift in [(8, 16, 64, 0), (16, 24, 64, 0), (16, 16, 72, 0), (16, 16, 64, 4)]:
        assert lib().l4p_broadcast_block(st(), base.data_ptr() + shift, off, nbytes, stride, 3) == E_INVALID
    torch.cuda.synchronize()
    assert is_sentinel(base)


# ------------------------------------------------------------------------------------------------
# l4p_track_prepare, l4p_track_commit
# ------------------------------------------------------------------------------------------------
def test_track_prepare_and_commit_recursion_is_exact(dev):
    """track_prepare_kernel / track_commit_kernel / masked_rows_copy_kernel over a recursion as forward_windowed_core drives it:
    N = 70 (two 64-thread blocks, the second ragged), ws = 16, T = 40, windows (start, next) = (0, 8), (8, 16), (16, 24) and the last one
    (24, last_window).  Crafted rows: a query time exactly on a frame centre (valid_t switches at t + 0.5 == q_t), a query after every
    window (valid_n = 0: pfeat / plabel stay), a late query (the re-seed of the early windows would move its time backwards: not applied),
    estimates whose x equals the original query's (one coordinate equal, the others changed: label 1), visibilities on a coarse grid and
    one constant row (ties inside the overlap: the FIRST maximum wins).  Every buffer is compared for exact equality with the
    float32-comparing reference after every call; the clip buffers carry a guard track whose sentinel must survive."""
    N, ws, T, C = 70, 16, 40, 24
    g = torch.Generator().manual_seed(900)
    q = torch.rand((N, 3), generator=g) * torch.tensor([float(T - 8), 224.0, 224.0])
    q[0, 0], q[1, 0], q[2, 0], q[3, 0], q[4, 0], q[5, 0], q[6, 0] = 3.5, 100.0, 12.5, 30.5, 0.0, 15.5, 16.0
    q[69, 0] = 11.5  # (last thread of the ragged block)
    orig = q.clone()
    orig[60:64, :] += 1.0  # no coordinate equal to the original: label 2 when valid, 0 when not
    q[63, 0] = 90.0
    orig[63] = q[63] + 1.0  # never valid and nothing equal: label 0
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # clip state, host (reference) and device; one guard track behind every buffer
    h = {"traj": np.zeros((N, 2, T), np.float32), "vis": np.full((N, T), -10.0, np.float32), "depth": np.zeros((N, T), np.float32),
         "cur_q": q.numpy().copy(), "plabel": np.zeros(N, np.float32), "pfeat": np.zeros((N, C), np.float32)}

    def guarded(a):
        t = sentinel((a.shape[0] + 1, *a.shape[1:]), torch.float32)
        t[:a.shape[0]] = f32(a)
        return t

    d = {k_: guarded(v_) for k_, v_ in h.items()}
    orig_d = orig.cuda()
    seen = {0: 0, 1: 0, 2: 0, "tie": 0, "back": 0, "stay": 0, "moved": 0}
    for start, nxt, last in [(0, 8, 0), (8, 16, 0), (16, 24, 0), (24, 0, 1)]:
        # prepare
        q_off, labels = sentinel((N + 1, 3), torch.float32), sentinel((N + 1,), torch.float32)
        valid_t, valid_n = sentinel((N + 1, ws), torch.uint8), sentinel((N + 1,), torch.uint8)
        rc = lib().l4p_track_prepare(st(), ptr(d["cur_q"]), ptr(orig_d), start, ws, ptr(q_off), ptr(labels), ptr(valid_t), ptr(valid_n), N)
        torch.cuda.synchronize()
        assert rc == 0
        rq, rl, rvt, rvn = R.track_prepare_ref(h["cur_q"], orig.numpy(), start, ws)
        assert np.array_equal(q_off[:N].cpu().numpy(), rq) and np.array_equal(labels[:N].cpu().numpy(), rl)
        assert np.array_equal(valid_t[:N].cpu().numpy(), rvt) and np.array_equal(valid_n[:N].cpu().numpy(), rvn)
        assert all(is_sentinel(t[N:]) for t in (q_off, labels, valid_t, valid_n))
        for v_ in (0, 1, 2):
            seen[v_] += int((rl == v_).sum())
        # a window's estimates
        w_vis = (torch.round(torch.randn((N, ws), generator=g) * 2.0) / 2.0).numpy()
        w_vis[7] = 1.0
        w_traj = (torch.rand((N, 2, ws), generator=g) * 224.0).numpy()
        w_traj[8:20, 0, :] = orig.numpy()[8:20, 1:2]
        w_depth = (torch.rand((N, ws), generator=g) + 0.5).numpy()
        new_pfeat = torch.randn((N, C), generator=g).numpy()
        best = sentinel((N + 1,), torch.int32)
        wt, wv, wd, npf = f32(w_traj), f32(w_vis), f32(w_depth), f32(new_pfeat)
        rc = lib().l4p_track_commit(st(), ptr(wt), ptr(wv), ptr(wd), ptr(valid_t), ptr(valid_n), ptr(d["traj"]), ptr(d["vis"]),
                                    ptr(d["depth"]), T, start, ws, nxt, last, ptr(d["cur_q"]), ptr(d["plabel"]), ptr(npf), ptr(d["pfeat"]),
                                    ptr(best), N, C)
        torch.cuda.synchronize()
        assert rc == 0
        r = R.track_commit_ref(w_traj, w_vis, w_depth, rvt, rvn, h["traj"], h["vis"], h["depth"], start, ws, nxt, last, h["cur_q"],
                               h["plabel"], new_pfeat, h["pfeat"])
        for k_ in h:
            assert np.array_equal(d[k_][:N].cpu().numpy(), r[k_]), f"{k_} after window at {start}"
            assert is_sentinel(d[k_][N:]), k_
        if last:
            assert is_sentinel(best)  # last_window returns before the argmax
        else:
            assert np.array_equal(best[:N].cpu().numpy(), r["best"]) and is_sentinel(best[N:])
            ov = r["vis"][:, nxt:start + ws]
            seen["tie"] += int(((ov == ov.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            moved = (r["cur_q"] != h["cur_q"]).any(axis=1)
            seen["moved"] += int(moved.sum())
            seen["back"] += int((r["best"].astype(np.float32) + nxt + 0.5 <= h["cur_q"][:, 0]).sum())
            seen["stay"] += int((rvn == 0).sum())
        for k_ in h:
            h[k_] = r[k_]
    assert all(v_ > 0 for v_ in seen.values()), seen  # every crafted situation occurred


# ------------------------------------------------------------------------------------------------
# l4p_cast
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cast_is_torchs_conversion_bitwise(dev, mode):
    """cast_kernel: n = 4 and 8 (one / two groups of four), 4000, and 4 (2048 * 256 + 3) - past the 2048-block grid cap, so threads
    stride.  Equal to torch's conversion (and to cast_ref's statement on the bit patterns) in all three engines; +-inf, +-0, rounding
    ties of both 16-bit types and the half overflow edge are carried as torch carries them.  n % 4 != 0 is refused before the launch."""
    T = ops.torch_dtype(mode)
    sp = R.cast_specials()
    for n in R.CAST_SIZES:
        x = rnd((n,), 1000 + n % 97, 30.0)
        m = min(n, sp.numel())
        x[:m] = sp[:m]
        x[n - m:] = sp[:m].flip(0) if n >= 2 * m else x[n - m:]
        y, xd = sentinel((n + 8,), T), x.cuda()
        rc = lib().l4p_cast(st(), mode, ptr(xd), ptr(y), n)
        torch.cuda.synchronize()
        assert rc == 0 and is_sentinel(y[n:])
        assert torch.equal(bits(y[:n]).cpu(), bits(x.to(T))), f"n = {n}"
        assert torch.equal(bits(y[:n]).cpu(), bits(R.cast_ref(x, T))), f"n = {n}"
    y, z = sentinel((16,), T), torch.zeros(16, device="cuda")
    for n in (1, 6, 7):
        assert lib().l4p_cast(st(), mode, ptr(z), ptr(y), n) == E_INVALID
    torch.cuda.synchronize()
    assert is_sentinel(y)
