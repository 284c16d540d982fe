"""The cases of tests/test_gemm_forms_gpu.py and their CPU side, in one place: tests/test_gemm_forms_cpu.py imports the same lists, so
the GPU cases and the proof that their inputs discriminate cannot drift apart.

A Case is one launch of l4p_gemm / l4p_conv3d_k3: shape, engine type, epilogue, knobs and the kernel form its profiler tag must name
(csrc/gemm_select.hpp names it, csrc/gemm_launch.hpp launches it).  Everything here runs on the CPU:

  * operands: random, rounded to the engine type; the LAST k-chunk (8 elements, 4 for f32: one 16-byte staging chunk) of the left
    operand is multiplied by 4, so a kernel that loses the contraction's tail is far outside the bounds;
  * reference(case): float64 from those rounded operands - the product, plus bias, activation and the residuals as stored;
  * reference(case, "dropk") / reference(case, "swapn"): two WRONG references - the last k-chunk of the contraction dropped; the last
    8-column group of the last N tile taken from the neighbouring group.  tests/test_gemm_forms_cpu.py asserts that both fail
    tests/test_kernels_gpu.py's check against the true one, for every case.
"""
import dataclasses
import functools
import itertools

import torch
import torch.nn.functional as F

from l4p_amd import ops
from l4p_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, L4P_BF16, L4P_F16, L4P_F32

M16 = (L4P_BF16, L4P_F16)
LOG2E = 1.4426950408889634
V10 = (("gemm_variant", 10),)
V10_T256 = (("gemm_variant", 10), ("gemm_t192", 0))
NO_HALO = (("conv_halo", 0),)


@dataclasses.dataclass(frozen=True)
class Case:
    form: str               # the tail of the profiler tag: "M%d N%d K%d epi%d act%d " + form
    M: int                  # logical rows (conv: B * To * Ho * Wo)
    N: int
    K: int
    mode: int
    act: int = ACT_NONE
    res: str = ""           # "", "f32", "T": the kind of res1 (and res2)
    res2: bool = False
    res_mod: int = 0
    outs: tuple = ("T",)    # of "T", "f32", "relu" (out_relu_T)
    inplace: bool = False   # the output of the residual's type aliases res1
    splitk: int = 1
    rowmap: tuple = ()      # (gr, gs, go): a_* and c_* of the descriptor
    wgr: int = 0            # row-grouped weights: rows per group (w_gr)
    conv: tuple = ()        # (B, T, H, W, Cin, st, sh, sw, relu_in)
    sampled: bool = False   # conv: the reference covers sample_rows(case) only
    epi: int = 0            # 0 dense, 1 QKV (geo = (B, S, H, Dh)), 2 ConvTranspose (geo = (B, T, H, W, kt, kh, kw, cout))
    geo: tuple = ()
    knobs: tuple = ()
    cls: str = "gemm_small"

    @property
    def tag(self):
        return f"M{self.M} N{self.N} K{self.K} epi{self.epi} act{self.act} {self.form}"

    @property
    def rows_phys(self):
        if not self.rowmap:
            return self.M
        gr, gs, go = self.rowmap
        return ((self.M - 1) // gr) * gs + go + gr

    @property
    def chunk(self):
        return 4 if self.mode == L4P_F32 else 8


PAD = 8  # columns behind every row of A, W, the outputs and the residuals (the LDS-halo conv requires ldc == N: none there)
POINTERS = ("A", "W", "bias", "res1", "res2", "out_f32", "out_T", "out_relu_T", "partial", "vt", "k_tiled")


def desc_fields(case):
    """{field of l4p_gemm_desc: value} of the launch a case is: every integer field that is not zero, and 1 for every pointer in
    POINTERS that is set.  tests/test_gemm_forms_gpu.py fills its descriptors from this (and puts its buffers behind the pointers);
    tests/test_gemm_select_cpu.py feeds the same values to csrc/gemm_select.hpp on the host."""
    pad = 0 if case.form.startswith("halo") else PAD
    f = dict(A=1, W=1, bias=1, M=case.M, N=case.N, K=case.K, act=case.act, epi=case.epi)
    if case.conv:
        B, T, H, W, Cin, st, sh, sw, relu_in = case.conv
        To, Ho, Wo = conv_out_dims(case.conv)
        f.update(Ti=T, Hi=H, Wi=W, Cin=Cin, To=To, Ho=Ho, Wo=Wo, st=st, sh=sh, sw=sw, relu_in=relu_in, ldw=case.K)
    else:
        f.update(lda=case.K + PAD, ldw=case.K + PAD)
    if case.epi == 1:    # QKV: q dense behind out_T, K and V scattered
        B, S, H, Dh = case.geo
        f.update(out_T=1, ldc=H * ops.DP + PAD, k_tiled=1, vt=1, S=S, H=H, Dp=ops.DP)
        return f
    if case.epi == 2:    # ConvTranspose: pixel-shuffle scatter behind out_T
        B, T, H, W, kt, kh, kw, cout = case.geo
        f.update(out_T=1, Ti=T, Hi=H, Wi=W, kt=kt, kh=kh, kw=kw, Cout=cout)
        return f
    if case.rowmap:
        gr, gs, go = case.rowmap
        f.update(a_gr=gr, a_gs=gs, a_go=go, c_gr=gr, c_gs=gs, c_go=go)
    if case.wgr:
        f.update(w_gr=case.wgr, w_gs=case.N * (case.K + PAD), b_gs=case.N)
    f["ldc"] = case.N + pad
    for name in case.outs:
        f[{"T": "out_T", "f32": "out_f32", "relu": "out_relu_T"}[name]] = 1
    if case.res and case.inplace:    # the output of the residual's type IS res1
        if ("f32" if case.res == "f32" else "T") in case.outs:
            f.update(res1=1, res_f32=int(case.res == "f32"), ldr=case.N + pad)
    elif case.res:
        f.update(res1=1, res_f32=int(case.res == "f32"), ldr=case.N + pad, res_mod=case.res_mod)
        if case.res2:
            f["res2"] = 1
    if case.splitk > 1:
        f.update(splitk=case.splitk, partial=1)
    return f


def phys_rows(case):
    """logical row m -> physical row (include/l4p_hip.h: (m / gr) * gs + go + m % gr)"""
    m = torch.arange(case.M)
    if not case.rowmap:
        return m
    gr, gs, go = case.rowmap
    return (m // gr) * gs + go + m % gr


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def conv_out_dims(conv):
    B, T, H, W, Cin, st, sh, sw, _ = conv
    return (T - 1) // st + 1, (H - 1) // sh + 1, (W - 1) // sw + 1


@functools.lru_cache(maxsize=None)
def _operands(rows, N, K, mode, conv, groups):
    td = ops.torch_dtype(mode)
    c = 4 if mode == L4P_F32 else 8
    seed = rows * 7 + N * 131 + K * 17 + mode
    if conv:
        B, T, H, W, Cin = conv[:5]
        a = _rnd((B, T, H, W, Cin), seed)
        a[..., Cin - c:] *= 4.0  # (the last chunk of every tap, the last tap's among them)
    else:
        a = _rnd((rows, K), seed)
        a[:, K - c:] *= 4.0
    w = _rnd((groups * N, K), seed + 1, K ** -0.5)
    bias = _rnd((groups * N,), seed + 2)
    return a.to(td), w.to(td), bias


def operands(case):
    """(a, w, bias): a [rows_phys, K] (conv: x [B, T, H, W, Cin]) and w [groups * N, K] in the engine type, bias float [groups * N]."""
    groups = (case.M + case.wgr - 1) // case.wgr if case.wgr else 1
    return _operands(case.rows_phys, case.N, case.K, case.mode, case.conv, groups)


@functools.lru_cache(maxsize=None)
def _residual(rows, N, mode, kind, which):
    r = _rnd((rows, N), rows * 3 + N * 5 + which)
    return r if kind == "f32" else r.to(ops.torch_dtype(mode))


def residuals(case):
    """(res1, res2) as stored: [res_mod or rows_phys, N], float or the engine type; None where the case has none."""
    if not case.res:
        return None, None
    rows = case.res_mod if case.res_mod else case.rows_phys
    return _residual(rows, case.N, case.mode, case.res, 1), (_residual(rows, case.N, case.mode, case.res, 2) if case.res2 else None)


@functools.lru_cache(maxsize=None)
def sample_rows(case):
    """conv cases too large for a whole-volume float64 reference: the first and last 512 output voxels (volume borders), 512 across the
    middle (a batch / plane seam), and 2048 scattered ones."""
    g = torch.Generator().manual_seed(7)
    M = case.M
    return torch.cat([torch.arange(0, 512), torch.arange(M - 512, M), torch.arange(M // 2 - 256, M // 2 + 256),
                      torch.randint(0, M, (2048,), generator=g)])


def ref_rows(case):
    return sample_rows(case) if case.sampled else torch.arange(case.M)


@functools.lru_cache(maxsize=None)
def _lhs(case_key):
    case = case_key
    a = operands(case)[0].double()
    if not case.conv:
        return a[phys_rows(case)]
    B, T, H, W, Cin, st, sh, sw, relu_in = case.conv
    To, Ho, Wo = conv_out_dims(case.conv)
    if relu_in:
        a = F.relu(a)
    xp = F.pad(a, (0, 0, 1, 1, 1, 1, 1, 1))
    rows = ref_rows(case)
    wo, r = rows % Wo, rows // Wo
    ho, r = r % Ho, r // Ho
    to, b = r % To, r // To
    return torch.cat([xp[b, to * st + dt, ho * sh + dh, wo * sw + dw] for dt in range(3) for dh in range(3) for dw in range(3)], dim=1)


def _shape_key(case):
    """the fields the product depends on (the sweep's 240 epilogues share one product)"""
    return dataclasses.replace(case, form="", act=ACT_NONE, res="", res2=False, res_mod=0, outs=("T",), inplace=False, splitk=1,
                               knobs=(), cls="", epi=0, geo=())


@functools.lru_cache(maxsize=None)
def _product(key, wrong):
    """float64 [rows, N]: sum_k a[m][k] w[n][k] (+ nothing else)"""
    lhs = _lhs(key)
    w = operands(key)[1].double()
    if wrong == "dropk":
        lhs = lhs.clone()
        lhs[:, key.K - key.chunk:] = 0
    if key.wgr:
        z = torch.empty(lhs.shape[0], key.N, dtype=torch.float64)
        for g in range((key.M + key.wgr - 1) // key.wgr):
            sl = slice(g * key.wgr, min((g + 1) * key.wgr, key.M))
            z[sl] = lhs[sl] @ w[g * key.N:(g + 1) * key.N].t()
    else:
        z = lhs @ w.t()
    if wrong == "swapn":
        assert key.N >= 16
        z[:, key.N - 8:] = z[:, key.N - 16:key.N - 8]
    return z


def reference(case, wrong=""):
    """{output name: float64 [rows, N]} of the case's epilogue (include/l4p_hip.h: v = acc + bias; v = act(v); v += res1 (+ res2)).
    QKV / ConvTranspose cases: "T" is the [M, N] matrix before the scatter (QKV: q columns times q_scale)."""
    key = _shape_key(case)
    v = _product(key, wrong).clone()
    bias = operands(case)[2].double()
    if case.wgr:
        for g in range((case.M + case.wgr - 1) // case.wgr):
            v[g * case.wgr:(g + 1) * case.wgr] += bias[g * case.N:(g + 1) * case.N]
    else:
        v = v + bias
    if case.act == ACT_GELU:
        v = F.gelu(v)
    elif case.act == ACT_RELU:
        v = F.relu(v)
    if case.epi == 1:
        B, S, H, Dh = case.geo
        v[:, :H * ops.DP] *= Dh ** -0.5 * LOG2E
    r1, r2 = residuals(case)
    if r1 is not None:
        rr = ref_rows(case) % case.res_mod if case.res_mod else phys_rows(case)[ref_rows(case)]
        v = v + r1.double()[rr]
        if r2 is not None:
            v = v + r2.double()[rr]
    return {name: (F.relu(v) if name == "relu" else v) for name in case.outs}


def wrong_kinds(case):
    """the wrong references a case has: with a single 8-column group (N = 8) there is no neighbouring group to take columns from"""
    return ("dropk", "swapn") if case.N >= 16 else ("dropk",)


def _both(mode):
    return ("T", "f32") if mode != L4P_F32 else ("T",)


def _forms(form, shapes, modes, **kw):
    return [Case(form, M, N, K, mode, outs=_both(mode), **kw) for (M, N, K) in shapes for mode in modes]


# ---- dense forms at their smallest ragged shapes (thresholds: gemm_select at the default knobs) ----
STAGED_2 = _forms("sk1 t128x64", [(200, 72, 200), (129, 8, 72)], M16)             # K < 384; one 8-column group; one row past a tile
STAGED_DEEP = _forms("sk1 t128x64 deep", [(130, 72, 392), (300, 200, 1224)], M16)  # 6.125 and 19.125 k-tiles on the 4-slot ring
STAGED_WIDE = _forms("sk1 t128x128", [(2500, 2504, 72)], M16 + (L4P_F32,), cls="gemm")  # 20 x 20 = 400 tiles, 100 of 256 x 256
STAGED_F32 = _forms("sk1 t128x64", [(70, 72, 36), (200, 136, 100)], (L4P_F32,))  # K tail of 4 in a 32-wide k-tile
SPLITK_SHAPES = [("sk3 t128x64", 200, 72), ("sk3 t128x128", 200, 264)]


def _finish(mode):
    """the epilogues of splitk_finish_kernel"""
    T = "T"
    return [dict(act=ACT_GELU, outs=(T,)),
            dict(act=ACT_RELU, res=T, res2=True, outs=(T,)),
            dict(res="f32", res_mod=64, outs=("f32",) if mode != L4P_F32 else (T,)),
            dict(outs=("f32", T, "relu"))]


STAGED_SPLITK = [Case(form, M, N, 1000 if mode != L4P_F32 else 996, mode, splitk=3, **kw)
                 for form, M, N in SPLITK_SHAPES for mode in M16 + (L4P_F32,) for kw in _finish(mode)]
P8_T256 = _forms("8p t256x256", [(40, 136, 8), (130, 136, 64), (257, 264, 72), (300, 520, 192), (260, 2056, 72), (260, 4104, 72)], M16,
                 knobs=V10_T256, cls="gemm")
P8_T192 = _forms("8p t256x192", [(40, 136, 8), (257, 200, 72), (300, 392, 192), (260, 2056, 72)], M16, knobs=V10, cls="gemm")
P8_SPLITK = [Case(form, 1300, 1544, 2056, mode, splitk=4, res="f32", inplace=True, outs=("f32",), knobs=knobs, cls="gemm")
             for form, knobs in (("8p sk4 t256x192", ()), ("8p sk4 t256x256", (("gemm_t192", 0),))) for mode in M16]
P8_ROWMAP = _forms("8p t256x256", [(300, 264, 136)], M16, rowmap=(100, 250, 50), knobs=V10, cls="gemm")
# row-grouped weights (no existing test asserts a " wgrp" tag): ragged M inside the last group; K % 64 != 0 keeps the one-wave kernel away
WGRP = (_forms("sk1 t64x64 deep wgrp", [(300, 56, 392)], M16, wgr=128) +
        _forms("sk1 t128x64 deep wgrp", [(8 * 2048 + 100, 56, 392)], M16, wgr=2048) +
        _forms("sk1 t128x64 wgrp", [(300, 56, 392)], M16, wgr=128, knobs=(("track_deep", 0),)) +
        _forms("sk1 t128x128 wgrp", [(300, 72, 72), (300, 136, 72)], M16, wgr=128))

# ---- QKV and ConvTranspose epilogues on the 8-phase kernel: the small cases tests/test_kernels_gpu.py runs on the staged kernels ----
P8_QKV = [Case(f"8p t256x{tn}", B * S, 3 * H * ops.DP, H * Dh, mode, epi=1, geo=(B, S, H, Dh), knobs=knobs, cls="gemm")
          for (B, S, H, Dh) in ((2, 256, 2, 88), (1, 128, 3, 64)) for mode in M16 for tn, knobs in ((192, V10), (256, V10_T256))]
# (cout = 72, not the staged test's 64: k = (2, 1, 1) must give N > 128 to reach the 8-phase kernel, and a tap boundary then falls
#  inside a wave's columns)
P8_CONVT = [Case(f"8p t256x{tn}", 1 * 4 * 8 * 8, k[0] * k[1] * k[2] * 72, 192, mode, epi=2, geo=(1, 4, 8, 8) + k + (72,), knobs=knobs, cls="gemm")
            for k in ((2, 4, 4), (2, 2, 2), (1, 2, 2), (2, 1, 1)) for mode in M16 for tn, knobs in ((192, V10), (256, V10_T256))]


# ---- implicit-GEMM conv forms ----
def _conv(form, vol, cout, stride, relu_in, mode, **kw):
    conv = tuple(vol) + tuple(stride) + (relu_in,)
    To, Ho, Wo = conv_out_dims(conv)
    return Case(form, vol[0] * To * Ho * Wo, cout, 27 * vol[4], mode, conv=conv, cls="conv3d", **kw)


CONV_STAGED = ([_conv("sk1 t128x64", (2, 3, 5, 7, 64), 72, s, r, mode, knobs=NO_HALO, act=ACT_RELU, res="T", outs=("T", "relu"))
                for s in ((1, 1, 1), (1, 2, 2), (2, 2, 2)) for r in (0, 1) for mode in M16 + (L4P_F32,)] +
               # "big": 400 tiles of 128 rows
               [_conv("sk1 t128x128", (2, 4, 80, 80, 64), 72, (1, 1, 1), r, mode, knobs=NO_HALO, sampled=True) for r in (0, 1) for mode in M16])
CONV_8P = [_conv("8p t256x256", vol, cout, (1, 1, 1), 0, mode, knobs=V10 + NO_HALO, res="T", res2=True, outs=("T", "relu"))
           for vol in ((2, 3, 5, 7, 64), (1, 2, 16, 16, 128)) for cout in (136, 264) for mode in M16]
# LDS-halo conv: the smallest volumes with M / BM >= 192 made of whole 2 x (8 | 16) x 16 blocks, H != W.  Cin = 64 and 192: two and six
# 32-channel slices (the existing tests run 4, 8 and 16); l4p_conv3d_k3 takes Cin % 64 == 0 only on the 16-bit engines (launch_gemm), so
# a single slice or an odd count - which conv_halo_fits alone would admit - cannot be launched
CONV_HALO = [_conv(form, vol + (cin,), cout, (1, 1, 1), 0, mode, sampled=True, **kw)
             for form, vol, cout in (("halo t256x256", (2, 4, 64, 96), 256), ("halo t512x128", (2, 4, 96, 128), 128))
             for cin in (64, 192) for mode in M16
             for kw in (dict(act=ACT_RELU), dict(res="T", res2=True, outs=("T", "relu")))]

DENSE_CASES = STAGED_2 + STAGED_DEEP + STAGED_WIDE + STAGED_F32 + STAGED_SPLITK + P8_T256 + P8_T192 + P8_SPLITK + P8_ROWMAP + WGRP
CONV_CASES = CONV_STAGED + CONV_8P + CONV_HALO
SCATTER_CASES = P8_QKV + P8_CONVT

# ---- the epilogue sweep ----
SWEEP_SHAPE = (300, 200, 136)
SWEEP_OUTS = (("T",), ("f32",), ("T", "f32"), ("T", "relu"))


def epilogue_is_lean(case):
    """What the host twins dense_epilogue_is_lean / epilogue_is_lean_8p (csrc/gemm_select.hpp) must return for a dense-epilogue case,
    stated from the comments of csrc/gemm_epilogue.hpp ("Lean epilogue for the plain dense family (L4P_EPI_DENSE, no row maps, no broadcast
    residual)", gemm_epilogue_dense_cases): activation x residual kind is one of (any, none), (none, float), (none, T), (ReLU, T), and
    a second residual exists only beside a T one.  The outputs do not enter."""
    if case.res_mod or case.rowmap:
        return False
    if case.res == "f32" and case.res2:
        return False
    return (not case.res) or (case.res == "f32" and case.act == ACT_NONE) or (case.res == "T" and case.act in (ACT_NONE, ACT_RELU))


def sweep_epilogues():
    """(act, res, res2, outs, res_mod, rowmap): the full cross + one broadcast-residual and one row-map case"""
    combos = [(act, res, res2, outs, 0, ()) for act in (ACT_NONE, ACT_GELU, ACT_RELU)
              for res, res2 in (("", False), ("f32", False), ("f32", True), ("T", False), ("T", True)) for outs in SWEEP_OUTS]
    combos.append((ACT_NONE, "f32", False, ("f32",), 64, ()))
    combos.append((ACT_NONE, "f32", False, ("T", "f32"), 0, (100, 250, 50)))
    return combos


def sweep_cases(mode, eight_phase, epi_generic):
    M, N, K = SWEEP_SHAPE
    out = []
    for act, res, res2, outs, res_mod, rowmap in sweep_epilogues():
        c = Case("", M, N, K, mode, act=act, res=res, res2=res2, outs=outs, res_mod=res_mod, rowmap=rowmap,
                 knobs=(V10 if eight_phase else ()) + (("epi_generic", epi_generic),), cls="gemm" if eight_phase else "gemm_small")
        if eight_phase:
            form = "8p t256x192" if epilogue_is_lean(c) and not epi_generic else "8p t256x256"
        else:
            form = "sk1 t128x64"
        out.append(dataclasses.replace(c, form=form))
    return out


SWEEP_CASES = [c for mode, e8, gen in itertools.product(M16, (True, False), (0, 1)) for c in sweep_cases(mode, e8, gen)]
ALL_CASES = DENSE_CASES + CONV_CASES + SCATTER_CASES + SWEEP_CASES


def case_id(case):
    mode = {L4P_BF16: "bf16", L4P_F16: "f16", L4P_F32: "f32"}[case.mode]
    extra = "".join(f"-{k}{v}" for k, v in case.knobs) + (f"-act{case.act}" if case.act else "") + (f"-res{case.res}{2 if case.res2 else ''}" if case.res else "") + \
        (f"-mod{case.res_mod}" if case.res_mod else "") + ("-" + "+".join(case.outs) if case.outs != ("T",) else "") + \
        (f"-sk{case.splitk}" if case.splitk > 1 else "") + ("-rowmap" if case.rowmap else "") + \
        ("-conv" + "x".join(map(str, case.conv)) if case.conv else "") + ("-geo" + "x".join(map(str, case.geo)) if case.geo else "")
    return f"{case.form.replace(' ', '_')}-{mode}-{case.M}x{case.N}x{case.K}{extra}"
