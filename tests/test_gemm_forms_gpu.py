"""Every kernel form the GEMM / conv launcher can pick (csrc/gemm_select.hpp: gemm_select, gemm_group_select; csrc/gemm_launch.hpp:
launch_cfg, launch_8p, launch_halo), each at the smallest ragged shape that reaches it, against a float64 reference computed from the same rounded operands
(tests/gemm_forms_cases.py holds the cases and their CPU side; reference call sites: include/l4p_hip.h, l4p_gemm_desc).  Every case
asserts through the event profiler (l4p_prof_detail) that there was exactly one launch and that its tag names the form the case is
about, so a moved threshold in the launcher fails here instead of silently leaving a form untested.

What the shapes reach: 1, 2 and 3 k-tiles of the 8-phase kernel (its prologue's look-ahead stages only zero chunks), tile grids
smaller than the 8 XCD slots of decode_tile, uneven last column bands (ntn = 9, 11, 17), split-K slices of unequal length with a
partial last k-tile, the four-slot ring at 6.125 k-tiles, f32 K tails of 4 in a 32-wide k-tile, row maps, row-grouped weights with a
ragged last group, conv batch seams and every border class inside one tile, the LDS-halo conv at two and at six channel slices.

Guard for ragged edges, in every case: outputs (and split-K partials) are allocated with ldc = N + 8 and 16 extra rows and pre-filled
with NaN (an output that aliases its residual: a fixed finite value around the data); the padding columns and the extra rows must
be bit-for-bit untouched and every element inside [M, N] overwritten.  A and W have lda = ldw = K + 8 with 100.0 in the padding, so
a read past K is seen as well.  (The LDS-halo conv requires ldc == N: extra rows only.)

Tolerances: tests/test_kernels_gpu.py's check, unchanged.  One line per case: GEMM_FORM form=... mode=... M= N= K= rel_l2= max_err/max|ref|=.
"""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib, ops
from l4p_amd._lib import EPI_DENSE, EPI_QKV, L4P_BF16, GemmDesc
from tests import gemm_forms_cases as G
from tests.gemm_forms_cases import case_id
from tests.test_gemm8p_gpu import prof_tags
from tests.test_kernels_gpu import check

E_INVALID = _lib.L4P_E_INVALID
PAD, GUARD_ROWS = G.PAD, 16
SENTINEL = -24576.0  # (exact in bf16 and f16; the data are of order 1 to 10)
CLASSES = ("gemm", "gemm_small", "conv3d")
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _padded(t, fill, rows=None):
    """[r, c] -> device [rows or r, c + PAD], padding columns = fill, rows past r zero"""
    r, c = t.shape
    out = torch.zeros((rows or r, c + PAD), dtype=t.dtype)
    out[:r, c:] = fill
    out[:r, :c] = t
    return out.cuda()


def launches(p):
    """(class, tag, number of launches) of the GEMM / conv launches a prof_tags block saw (l4p_prof_detail: class, tag, count, ms)"""
    return [(ln[0], ln[1], int(ln[2])) for ln in p.lines if ln[0] in CLASSES]


def _desc_ints(case):
    """a descriptor with every integer field of the case (tests/gemm_forms_cases.py desc_fields: the values that
    tests/test_gemm_select_cpu.py pushes through the launcher's selection on the host); the caller puts its buffers behind the pointers"""
    d = GemmDesc()
    for name, value in G.desc_fields(case).items():
        if name not in G.POINTERS:
            setattr(d, name, value)
    return d


class Run:
    """One case on the device: builds the descriptor with guarded outputs, launches, asserts the profiler tag and the guards."""

    def __init__(self, case, knob):
        self.case, self.lib = case, _lib.load()
        for name, value in case.knobs:
            knob(name, value)
        td = ops.torch_dtype(case.mode)
        a, w, bias = G.operands(case)
        assert case.epi == EPI_DENSE
        d, fields = _desc_ints(case), G.desc_fields(case)
        self.d = d
        pad = fields["ldc"] - case.N  # (0 for the LDS-halo conv)
        self.keep = []
        if case.conv:
            A = a.cuda()
            Wd = torch.zeros(((case.N + 255) // 256 * 256, case.K), dtype=td)
            Wd[:case.N] = w
            Wd = Wd.cuda()
        else:
            A = _padded(a, 100.0)
            # (plain weights: whole tiles are read, rows >= N zero; a group's matrix has exactly N rows, the next group's behind it)
            Wd = _padded(w, 100.0, rows=(w.shape[0] + 255) // 256 * 256 + (256 if case.wgr else 0))
        bd = bias.cuda()
        d.A, d.W, d.bias = A.data_ptr(), Wd.data_ptr(), bd.data_ptr()
        self.keep += [A, Wd, bd]
        rows = case.rows_phys
        self.inside = torch.zeros((rows + GUARD_ROWS, case.N + pad), dtype=torch.bool, device="cuda")
        self.inside[G.phys_rows(case).cuda(), :case.N] = True
        r1, r2 = G.residuals(case)
        self.bufs = {}
        for name in case.outs:
            dt = torch.float32 if name == "f32" else td
            alias = case.inplace and name == ("f32" if case.res == "f32" else "T")
            buf = torch.full((rows + GUARD_ROWS, case.N + pad), SENTINEL if alias else NAN, dtype=dt, device="cuda")
            if alias:
                buf[:rows, :case.N] = r1.cuda()
                d.res1 = buf.data_ptr()
            setattr(d, {"T": "out_T", "f32": "out_f32", "relu": "out_relu_T"}[name], buf.data_ptr())
            self.bufs[name] = buf
        if r1 is not None and not case.inplace:
            rd = [(_padded(r, 100.0) if pad else r.cuda()) for r in (r1, r2) if r is not None]
            d.res1 = rd[0].data_ptr()
            if r2 is not None:
                d.res2 = rd[1].data_ptr()
            self.keep += rd
        self.partial = None
        if case.splitk > 1:
            self.partial = torch.full((case.splitk * case.M * case.N + GUARD_ROWS * case.N,), NAN, dtype=torch.float32, device="cuda")
            d.partial = self.partial.data_ptr()
        assert all(bool(getattr(d, name)) == bool(fields.get(name)) for name in G.POINTERS), "desc_fields and the buffers disagree"
        self.before = {name: buf.clone() for name, buf in self.bufs.items()}

    def launch(self):
        case = self.case
        fn = self.lib.l4p_conv3d_k3 if case.conv else self.lib.l4p_gemm
        with prof_tags() as p:
            _lib.check(fn(_stream(), case.mode, C.byref(self.d)), "launch")
        assert launches(p) == [(case.cls, case.tag, 1)], f"expected one launch {case.cls} '{case.tag}', launches were {p.lines}"
        for name, buf in self.bufs.items():
            before = self.before[name]
            assert torch.equal(_bits(buf)[~self.inside], _bits(before)[~self.inside]), f"{name}: a store outside [M, N] ({case.tag})"
            # (NaN pre-fill; an output that aliases its residual holds the residual there - that one is overwritten if check passes)
            assert not bool(torch.isnan(buf[self.inside]).any()), f"{name}: elements inside [M, N] were not written ({case.tag})"
        if self.partial is not None:
            n = case.splitk * case.M * case.N
            assert not bool(torch.isnan(self.partial[:n]).any()), "split-K: partials not written"
            assert bool(torch.isnan(self.partial[n:]).all()), "split-K: a store past the partial buffer"
        return self

    def out(self, name):
        """[M, N] of the logical rows"""
        return self.bufs[name][G.phys_rows(self.case).cuda(), :self.case.N]


def compare(case, outs):
    """outs: {name: [M, N] device tensor}; prints the measured errors, then tests/test_kernels_gpu.py's check"""
    ref = G.reference(case)
    rows = G.ref_rows(case)
    for name in case.outs:
        y, r = outs[name].float().cpu()[rows].double(), ref[name]
        assert bool(torch.isfinite(y).all())
        rel_l2, err = ((y - r).norm() / r.norm()).item(), ((y - r).abs().max() / r.abs().max()).item()
        print(f"GEMM_FORM form='{case.form}' mode={case.mode} out={name} M={case.M} N={case.N} K={case.K} act={case.act} res={case.res or '-'}"
              f"{'+res2' if case.res2 else ''} rel_l2={rel_l2:.3e} max_err/max|ref|={err:.3e}")
        check(outs[name][rows.cuda()], r, case.mode, name != "f32")


def run_and_compare(case, knob):
    run = Run(case, knob).launch()
    compare(case, {name: run.out(name) for name in case.outs})
    return run


def same_bits(x, y):
    return torch.equal(_bits(x.contiguous()), _bits(y.contiguous()))


def cases(lst):
    return pytest.mark.parametrize("case", lst, ids=[case_id(c) for c in lst])


@cases(G.STAGED_2 + G.STAGED_WIDE + G.STAGED_F32 + G.P8_T256 + G.P8_T192 + G.P8_ROWMAP)
def test_dense_form(dev, knob, case):
    """The LDS-staged kernel at 128x64 and 128x128 tiles (16-bit and f32) and the 8-phase kernel at 256x256 and 256x192 tiles, plain and
    with row maps (rows outside the map keep the sentinel)."""
    run_and_compare(case, knob)


@cases(G.STAGED_DEEP)
def test_deep_ring_equals_two_stages_bitwise(dev, knob, case):
    """Four stages against two (knob gemm_deep = 0): the same sums in the same order (gemm_select), so bit-identical outputs."""
    deep = run_and_compare(case, knob)
    plain = run_and_compare(dataclasses.replace(case, form="sk1 t128x64", knobs=(("gemm_deep", 0),)), knob)
    for name in case.outs:
        assert same_bits(deep.out(name), plain.out(name)), name


@cases(G.STAGED_SPLITK + G.P8_SPLITK)
def test_splitk_and_finish_kernel(dev, knob, case):
    """Split-K on the staged kernels (slices of 5, 5, 6 k-tiles; f32: 10, 11, 11 with a K tail) and on both 8-phase tile forms (33 k-tiles
    split 8, 8, 8, 9, the last one partial), then splitk_finish_kernel's epilogues; run-to-run bit-equal (fixed summation order)."""
    first = run_and_compare(case, knob)
    again = Run(case, knob).launch()
    for name in case.outs:
        assert same_bits(first.out(name), again.out(name)), name


@cases(G.WGRP)
def test_row_grouped_weights(dev, knob, case):
    run_and_compare(case, knob)


@pytest.mark.parametrize("mode", G.M16, ids=["bf16", "f16"])
def test_row_grouped_64_row_deep_tiles_equal_128_row_tiles_bitwise(dev, knob, mode):
    a, b = [c for c in G.WGRP if c.mode == mode and (c.M, c.N, c.K) == (300, 56, 392)]
    ra, rb = Run(a, knob).launch(), Run(b, knob).launch()
    assert {a.form, b.form} == {"sk1 t64x64 deep wgrp", "sk1 t128x64 wgrp"}
    for name in a.outs:
        assert same_bits(ra.out(name), rb.out(name)), name


@cases(G.CONV_STAGED + G.CONV_8P + G.CONV_HALO)
def test_conv_form(dev, knob, case):
    """Implicit-GEMM conv on the staged kernels (LDS-DMA loader and, with the fused input ReLU, the register loader), on the 8-phase
    kernel (conv_tile_walk's fallback where the plane is not a whole number of tiles) and the LDS-halo kernel (both ConvHaloCfg)."""
    run_and_compare(case, knob)


def k_tiled(k, kvb):
    """ops.k_tile_order with the KV block given (it derives it from the tensor's type): [B, S, H, 96] -> the attention kernels' K order"""
    B, S, H, dp = k.shape
    g = k.view(B, S // kvb, kvb, H, dp // 16, 2, 8).permute(0, 3, 1, 4, 2, 5, 6).contiguous()
    flip = ((torch.arange(kvb) >> 3) & 1).bool()
    g[:, :, :, :, flip] = g[:, :, :, :, flip].flip(-2)
    return g.reshape(-1)


@cases(G.P8_QKV)
def test_qkv_epilogue_on_the_8_phase_kernel(dev, knob, case):
    """L4P_EPI_QKV (q dense and pre-scaled, K in tile order, V transposed) at tests/test_kernels_gpu.py's small shapes, on both 8-phase
    tile forms; the three destinations are guarded like every other output."""
    for name, value in case.knobs:
        knob(name, value)
    B, S, H, Dh = case.geo
    td, HD = ops.torch_dtype(case.mode), H * ops.DP
    a, w, bias = G.operands(case)
    A, Wd, bd = _padded(a, 100.0), _padded(w, 100.0, rows=(case.N + 255) // 256 * 256), bias.cuda()
    q = torch.full((case.M + GUARD_ROWS, HD + PAD), NAN, dtype=td, device="cuda")
    kt = torch.full((case.M * HD + 1024,), NAN, dtype=td, device="cuda")
    vt = torch.full((case.M * HD + 1024,), NAN, dtype=td, device="cuda")
    d = _desc_ints(case)
    assert d.epi == EPI_QKV and d.ldc == HD + PAD
    d.A, d.W, d.bias = A.data_ptr(), Wd.data_ptr(), bd.data_ptr()
    d.out_T, d.k_tiled, d.vt = q.data_ptr(), kt.data_ptr(), vt.data_ptr()
    d.q_scale = Dh ** -0.5 * G.LOG2E
    with prof_tags() as p:
        _lib.check(_lib.load().l4p_gemm(_stream(), case.mode, C.byref(d)), "l4p_gemm(qkv)")
    assert launches(p) == [(case.cls, case.tag, 1)], p.lines
    assert bool(torch.isnan(q[case.M:]).all() and torch.isnan(q[:, HD:]).all() and torch.isnan(kt[case.M * HD:]).all() and torch.isnan(vt[case.M * HD:]).all())
    got = (q[:case.M, :HD], kt[:case.M * HD], vt[:case.M * HD])
    assert not any(bool(torch.isnan(t).any()) for t in got)
    full = G.reference(case)["T"].view(B, S, 3, H, ops.DP)
    want = (full[:, :, 0].reshape(case.M, HD), k_tiled(full[:, :, 1].contiguous(), 64), full[:, :, 2].permute(0, 2, 3, 1).reshape(-1))
    assert torch.equal(k_tiled(full[:, :, 1].contiguous(), 64).to(td), ops.k_tile_order(full[:, :, 1].contiguous().to(td)))
    for name, y, r in zip("qkv", got, want):
        yd = y.float().cpu().double()
        print(f"GEMM_FORM form='{case.form}' mode={case.mode} out={name} M={case.M} N={case.N} K={case.K} epi=qkv "
              f"rel_l2={((yd - r).norm() / r.norm()).item():.3e} max_err/max|ref|={((yd - r).abs().max() / r.abs().max()).item():.3e}")
        check(y, r, case.mode, True)


@cases(G.P8_CONVT)
def test_conv_transpose_epilogue_on_the_8_phase_kernel(dev, knob, case):
    """L4P_EPI_CONVT (pixel-shuffle scatter) for tests/test_kernels_gpu.py's four kernels k, on both 8-phase tile forms."""
    for name, value in case.knobs:
        knob(name, value)
    B, T, H, W, kt, kh, kw, cout = case.geo
    td = ops.torch_dtype(case.mode)
    a, w, bias = G.operands(case)
    A, Wd, bd = _padded(a, 100.0), _padded(w, 100.0, rows=(case.N + 255) // 256 * 256), bias.cuda()
    n_out = case.M * case.N
    out = torch.full((n_out + 1024,), NAN, dtype=td, device="cuda")
    d = _desc_ints(case)
    d.A, d.W, d.bias, d.out_T = A.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    with prof_tags() as p:
        _lib.check(_lib.load().l4p_gemm(_stream(), case.mode, C.byref(d)), "l4p_gemm(convT)")
    assert launches(p) == [(case.cls, case.tag, 1)], p.lines
    assert bool(torch.isnan(out[n_out:]).all()) and not bool(torch.isnan(out[:n_out]).any())
    # [B][T kt][H kh][W kw][cout] -> [M][tap * cout + co], tap = (dt * kh + dh) * kw + dw
    y = out[:n_out].view(B, T, kt, H, kh, W, kw, cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(case.M, case.N)
    compare(case, {"T": y})


@pytest.mark.parametrize("mode", G.M16, ids=["bf16", "f16"])
@pytest.mark.parametrize("eight_phase", [True, False], ids=["8p", "staged"])
def test_epilogue_sweep_lean_and_generic(dev, knob, mode, eight_phase):
    """activation x residual kind x second residual x outputs (+ one broadcast-residual and one row-map case) with epi_generic 0 and 1.

    The twin conditions: on the 8-phase kernel (gemm_variant = 10) the tag must be t256x192 - the form without a generic epilogue -
    exactly when tests/gemm_forms_cases.py's epilogue_is_lean holds and epi_generic = 0, else t256x256; a host twin that called a
    non-lean epilogue lean would launch tiles that write nothing (caught by the NaN guard), the other way round by the tag.  On the
    staged 128x64 kernel the tag does not change, the body does.

    Lean against generic (both bodies read: csrc/gemm_epilogue.hpp gemm_epilogue_dense / gemm_epilogue_row): the same float operations in the same
    order - bias, activation (explicit FMAs, gelu_poly2 = gelu_poly per element), residual, conversion - with ONE exception: two T
    residuals are added as v + (r1 + r2) by the lean body and as (v + r1) + r2 by the generic one.  So outputs are asserted bit-equal,
    and for that combination equal to one output ulp of the element (the form test_layernorm_of_engine_dtype_rows_in_place uses;
    float outputs: the rounding of the three float additions)."""
    outs = {}
    for gen in (0, 1):
        for case in G.sweep_cases(mode, eight_phase, gen):
            run = run_and_compare(case, knob)
            outs[(gen,) + dataclasses.astuple(dataclasses.replace(case, form="", knobs=()))] = (case, run)
    ulp = 2.0 ** (-7 if mode == L4P_BF16 else -10)
    for key, (case, lean) in outs.items():
        if key[0] != 0:
            continue
        generic = outs[(1,) + key[1:]][1]
        for name in case.outs:
            x, y = lean.out(name), generic.out(name)
            if not (case.res == "T" and case.res2):
                assert same_bits(x, y), (case_id(case), name)
                continue
            r1, r2 = (r.cuda().float() for r in G.residuals(case))
            mag = torch.maximum(x.float().abs(), y.float().abs()) + r1.abs() + r2.abs()
            bound = 2.0 ** -21 * mag + (0.0 if name == "f32" else 1.01 * ulp * torch.maximum(x.float().abs(), y.float().abs()))
            assert bool(((x.float() - y.float()).abs() <= bound).all()), (case_id(case), name)


# ---- refusals ----
def _refusal_desc(M=200, N=72, K=200, mode=L4P_BF16):
    td = ops.torch_dtype(mode)
    keep = [torch.ones((M, K + 16), dtype=td, device="cuda"), torch.ones((256, K + 16), dtype=td, device="cuda"),
            torch.full((M, N), 7.0, dtype=td, device="cuda"), torch.full((4 * M * N,), 7.0, dtype=torch.float32, device="cuda")]
    d = GemmDesc()
    d.A, d.lda, d.W, d.ldw = keep[0].data_ptr(), K, keep[1].data_ptr(), K
    d.M, d.N, d.K, d.epi, d.out_T, d.ldc = M, N, K, EPI_DENSE, keep[2].data_ptr(), N
    return d, keep


@pytest.mark.parametrize("what,names", [("N", "N=76"), ("K", "K/ldw"), ("ldw", "K/ldw"), ("lda", "lda"), ("no_partial", "split-K"),
                                        ("splitk_tiles", "split-K"), ("splitk_qkv", "split-K")])
def test_launch_gemm_refusals(dev, what, names):
    """launch_gemm's argument checks: L4P_E_INVALID, a message that names the argument, no launch, the output untouched."""
    d, keep = _refusal_desc()
    if what == "N":
        d.N = 76
    elif what == "K":
        d.K = 196  # (392 bytes)
    elif what == "ldw":
        d.ldw = 204
    elif what == "lda":
        d.lda = 204
    elif what == "no_partial":
        d.splitk = 2
    elif what == "splitk_tiles":
        d.splitk, d.partial = 5, keep[3].data_ptr()  # (K = 200: 4 k-tiles)
    elif what == "splitk_qkv":
        d.splitk, d.partial, d.epi = 2, keep[3].data_ptr(), EPI_QKV
    lib = _lib.load()
    with prof_tags() as p:
        rc = lib.l4p_gemm(_stream(), L4P_BF16, C.byref(d))
    assert rc == E_INVALID
    msg = lib.l4p_last_error().decode()
    assert "gemm" in msg and names in msg, msg
    assert not launches(p), p.lines
    assert bool((keep[2] == 7.0).all()) and bool((keep[3] == 7.0).all())


# ---- grouped launch and kw_cols ----
def _group_members(kw_cols, kw_len, mode=L4P_BF16):
    """two small-deep members (M = 200 rows, K = 384: six k-tiles on the four-stage 128x64 kernel); member 0 has block-structured weights:
    columns [128 g, 128 g + 128) meet inputs [192 g, 192 g + 192) only"""
    td = ops.torch_dtype(mode)
    M, N, K = 200, 256, 384
    g = torch.Generator().manual_seed(77)
    a = torch.randn(M, K, generator=g).to(td)
    w0 = torch.zeros(N, K)
    for blk in range(2):
        w0[128 * blk:128 * blk + 128, 192 * blk:192 * blk + 192] = torch.randn(128, 192, generator=g) * 192 ** -0.5
    w = [w0.to(td), (torch.randn(N, K, generator=g) * K ** -0.5).to(td)]
    dev_ = [a.cuda(), w[0].cuda(), w[1].cuda()]

    def descs(outs):
        ds = (GemmDesc * 2)()
        for i in range(2):
            d = ds[i]
            d.A, d.lda, d.W, d.ldw = dev_[0].data_ptr(), K, dev_[1 + i].data_ptr(), K
            d.M, d.N, d.K, d.epi, d.out_T, d.ldc = M, N, K, EPI_DENSE, outs[i].data_ptr(), N
        ds[0].kw_cols, ds[0].kw_len = kw_cols, kw_len
        return ds

    def outs():
        return [torch.full((M, N), 7.0, dtype=td, device="cuda") for _ in range(2)]

    ref = [a.double() @ w[i].double().t() for i in range(2)]
    return descs, outs, ref, dev_


def test_gemm_group_refuses_a_misaligned_kw_cols_like_l4p_gemm(dev):
    """kw_cols = 64 (not a multiple of the 128-wide tile: gemm_body would contract the wrong k-window): l4p_gemm refuses the
    descriptor, and so must l4p_gemm_group - before anything is launched."""
    descs, outs, _, keep = _group_members(64, 1)
    lib = _lib.load()
    for grouped in (False, True):
        o = outs()
        ds = descs(o)
        with prof_tags() as p:
            rc = lib.l4p_gemm_group(_stream(), L4P_BF16, ds, 2) if grouped else lib.l4p_gemm(_stream(), L4P_BF16, C.byref(ds[0]))
        assert rc == E_INVALID, grouped
        msg = lib.l4p_last_error().decode()
        assert "kw_cols" in msg, msg
        assert not launches(p), p.lines
        assert all(bool((t == 7.0).all()) for t in o)


@pytest.mark.parametrize("mode", G.M16, ids=["bf16", "f16"])
def test_gemm_group_with_kw_cols_equals_separate_launches_bitwise(dev, mode):
    descs, outs, ref, keep = _group_members(128, 192, mode)
    lib = _lib.load()
    grp, sep = outs(), outs()
    dg, dsep = descs(grp), descs(sep)
    with prof_tags() as p:
        _lib.check(lib.l4p_gemm_group(_stream(), mode, dg, 2), "l4p_gemm_group")
    assert launches(p) == [("gemm_small", "group of 2: M200 N256 K384 ... t128x64 deep", 1)], p.lines
    with prof_tags() as p:
        for i in range(2):
            _lib.check(lib.l4p_gemm(_stream(), mode, C.byref(dsep[i])), "l4p_gemm")
    assert launches(p) == [("gemm_small", "M200 N256 K384 epi0 act0 sk1 t128x64 deep", 2)], p.lines
    for i in range(2):
        assert same_bits(grp[i], sep[i]), i
        check(grp[i], ref[i], mode, True)
