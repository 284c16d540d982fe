"""The tracker launchers' kernel-form selection (csrc/track_select.hpp) on the host: which kernel form, grid, block and LDS size every
tracker launch gets - the engine's launches, both sides of every threshold, and every shape of the GPU tests - checked without a GPU.
Most of these forms share a profiler tag (every 128-column context kernel is "ctx t48x128", both mask products "mask_product", all
small-attention forms "small_attn kind..."), so the GPU tests cannot tell which one ran, nor see a threshold that has moved.  This
test can.

tests/track_select_main.cpp includes track_select.hpp alone (plain C++17, no HIP) and answers one launch per input line with
"<form> [<profiler tag>] | grid=x,y,z block=b lds=bytes ...", or with the refusal's error text.  The expected values are literals
worked out by hand from the launchers' conditions.  All cases go through one process.

Sizes used below (bytes).  Context ring stage: 32 keys x (128 columns + 48 probs) x 2 = 11264 (64 columns: 7168); rings of 4 / 8 / 12
stages: 45056 / 90112 / 135168 (64 columns, 4 stages: 28672).  t2i attention: 24 P + 3328, plus (256 / (hd / 4)) * 24 * hd - 24 P when
that is positive.  i2t LDS form: 48 D + (256 / heads) * D * esize; direct form: 48 D.  Mask product LDS form: round16(12 C) + 128 C esize;
direct: 12 C.  Read-out: column form (3 h w + w + h) * 4, wide form + (2 (W + H) + 32 W) * 4; both + 128 static.  Device: 163840.
"""
import os
import re
import shutil
import subprocess

import pytest

from tests import kernel_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

BF16, F32, F16 = 0, 1, 2  # include/l4p_hip.h
T16 = (BF16, F16)
ALL = (BF16, F32, F16)
KNOB_DEFAULTS = {"track_deep": 1, "readout_wide": 1}
# 1 / sqrtf(hd) in float arithmetic, printed %.9g
SCALE = {176: "0.0753778368", 88: "0.106600359", 44: "0.150755674", 32: "0.176776692", 96: "0.102062069", 16: "0.25", 12: "0.288675129",
         36: "0.166666672", 4: "0.5", 64: "0.125"}


def q(what, **f):
    return what + " " + " ".join(f"{k}={v}" for k, v in f.items())


def geom(form, tag, grid, block, lds, extra=""):
    g = grid if isinstance(grid, tuple) else (grid, 1, 1)
    g = g + (1,) * (3 - len(g))
    return f"{form} [{tag}] | grid={g[0]},{g[1]},{g[2]} block={block} lds={lds}" + (" " + extra if extra else "")


ROWS = []  # (id, query line, expected answer)


def case(name, line, want):
    ROWS.append((name, line, want))


# ------------------------------------------------------------------------------------------------
# l4p_t2i_context: heads 8, tokens 6
# ------------------------------------------------------------------------------------------------
def ctx(name, dtypes, N, P, C, sf, want_form, grid, lds, deep=1, sf_out=None, Rg=None):
    Rg = (6 * N + 127) // 128 * 128 if Rg is None else Rg
    tag = f"M{48 * N} N{C} K{P} epi0 act0 ctx t48x{64 if C % 128 else 128}"
    for d in dtypes:
        case(f"ctx {name} dtype={d} deep={deep}",
             q("ctx", dtype=d, N=N, P=P, C=C, heads=8, tokens=6, Rg=Rg, shared_from=sf, **{"k.track_deep": deep, "k.readout_wide": 1}),
             geom(want_form, tag, grid, 256, lds, f"shared_from={sf if sf_out is None else sf_out}"))


# the engine (api_trackwin.hip t2i_folded: P = 2048 tokens, C = 1408; first window shared_from = P, later windows P / 2); 64 queries and
# a rank's shard of 8
ctx("engine_64_first", T16, 64, 2048, 1408, 2048, "ctx_ring4", (11, 64), 45056)
ctx("engine_64_later", T16, 64, 2048, 1408, 1024, "ctx_ring4", (11, 64), 45056)
ctx("engine_64_deep0", T16, 64, 2048, 1408, 2048, "ctx_ring4", (11, 64), 45056, deep=0)
ctx("engine_8_first", T16, 8, 2048, 1408, 2048, "ctx_ring12", (11, 8), 135168)
ctx("engine_8_later", T16, 8, 2048, 1408, 1024, "ctx_ring12", (11, 8), 135168)
ctx("engine_8_deep0", T16, 8, 2048, 1408, 1024, "ctx_ring4", (11, 8), 45056, deep=0)
ctx("engine_64_f32", (F32,), 64, 2048, 1408, 2048, "ctx_f32", (6, 64), 0)
ctx("engine_8_f32_later", (F32,), 8, 2048, 1408, 1024, "ctx_f32", (6, 8), 0)
# (C / 128) * N <= 256 compute units: 11 * 23 = 253, 11 * 24 = 264; 2 * 128 = 256, 2 * 129 = 258
ctx("thr_cus_253", T16, 23, 2048, 1408, 2048, "ctx_ring12", (11, 23), 135168)
ctx("thr_cus_264", T16, 24, 2048, 1408, 2048, "ctx_ring4", (11, 24), 45056)
ctx("thr_cus_256", T16, 128, 2048, 256, 2048, "ctx_ring12", (2, 128), 135168)
ctx("thr_cus_258", T16, 129, 2048, 256, 2048, "ctx_ring4", (2, 129), 45056)
# P % 128, P % 64: 1984 = 31 * 64, 1952 = 61 * 32
ctx("thr_P_1984", T16, 8, 1984, 1408, 1984, "ctx_ring8", (11, 8), 90112)
ctx("thr_P_1984_deep0", T16, 8, 1984, 1408, 1984, "ctx_ring4", (11, 8), 45056, deep=0)
ctx("thr_P_1952", T16, 8, 1952, 1408, 1952, "ctx_ring4", (11, 8), 45056)
# C % 128: the 64-column form has no deep ring
ctx("thr_C_704", T16, 8, 2048, 704, 2048, "ctx_mfma64", (11, 8), 28672)
ctx("thr_C_704_deep0", T16, 8, 2048, 704, 2048, "ctx_mfma64", (11, 8), 28672, deep=0)
ctx("thr_C_704_f32", (F32,), 8, 2048, 704, 2048, "ctx_f32", (3, 8), 0)
ctx("shared_from_clamped", ALL[:1], 8, 2048, 1408, 4096, "ctx_ring12", (11, 8), 135168, sf_out=2048)
# tests/test_track_gpu.py test_folded_t2i_value_kernels: N 5, P 608 (608 % 64 = 32: the ring of 4 whatever track_deep says - its
# track_deep A / B compares the SAME context kernel; the deep rings are test_t2i_context_two_stages_per_barrier's), shared_from P and 320
for sf in (608, 320):
    for deep in (1, 0):
        ctx(f"gpu_folded_1408_sf{sf}", T16, 5, 608, 1408, sf, "ctx_ring4", (11, 5), 45056, deep=deep)
        ctx(f"gpu_folded_704_sf{sf}", T16, 5, 608, 704, sf, "ctx_mfma64", (11, 5), 28672, deep=deep)
        ctx(f"gpu_folded_256_sf{sf}", T16, 5, 608, 256, sf, "ctx_ring4", (2, 5), 45056, deep=deep)
    ctx(f"gpu_folded_1408_f32_sf{sf}", (F32,), 5, 608, 1408, sf, "ctx_f32", (6, 5), 0)
    ctx(f"gpu_folded_704_f32_sf{sf}", (F32,), 5, 608, 704, sf, "ctx_f32", (3, 5), 0)
    ctx(f"gpu_folded_256_f32_sf{sf}", (F32,), 5, 608, 256, sf, "ctx_f32", (1, 5), 0)
# tests/test_track_gpu.py test_t2i_context_two_stages_per_barrier_equals_the_chip_filling_form: (N, P) = (3, 2048), (2, 1984), shared_from
# P and P // 2 // 32 * 32, track_deep 1 then 0
CTX_AB = [(3, 2048, "ctx_ring12", 135168), (2, 1984, "ctx_ring8", 90112)]
for N_, P_, form_, lds_ in CTX_AB:
    for sf in (P_, P_ // 2 // 32 * 32):
        ctx(f"gpu_ab_{N_}x{P_}_sf{sf}", T16, N_, P_, 1408, sf, form_, (11, N_), lds_)
        ctx(f"gpu_ab_{N_}x{P_}_sf{sf}", T16, N_, P_, 1408, sf, "ctx_ring4", (11, N_), 45056, deep=0)
T_CTX = "invalid: t2i_context: heads * tokens == 48, C % 64 == 0, P % 32 == 0, 96 <= P <= 4096, Rg >= N * tokens, shared_from % 32 == 0"
for name, f in [("P_64", dict(P=64)), ("P_4128", dict(P=4128)), ("P_100", dict(P=100)), ("C_96", dict(C=96)), ("heads_7", dict(heads=7)),
                ("Rg_short", dict(Rg=47)), ("sf_16", dict(shared_from=16)), ("sf_negative", dict(shared_from=-32)), ("N_0", dict(N=0))]:
    a = dict(dtype=BF16, N=8, P=2048, C=1408, heads=8, tokens=6, Rg=128, shared_from=2048)
    a.update(f)
    case(f"ctx refusal {name}", q("ctx", **a, **{"k.track_deep": 1}), T_CTX)


# ------------------------------------------------------------------------------------------------
# l4p_small_attn, l4p_t2i_attn_scores
# ------------------------------------------------------------------------------------------------
def attn(name, dtypes, kind, N, P, D, heads, form, grid, block, lds):
    hd = D // heads
    stride = P * D if kind in (1, 2) else 0
    for d in dtypes:
        case(f"attn {name} kind={kind} dtype={d}", q("attn", dtype=d, kind=kind, N=N, P=P, D=D, heads=heads),
             geom(form, f"small_attn kind{kind} N{N} P{P} D{D}", grid, block, lds, f"hd={hd} scale={SCALE[hd]} stride={stride}"))


def scores(name, N, P, D, heads, ld, lds):
    case(f"scores {name}", q("scores", N=N, P=P, D=D, heads=heads, ld=ld),
         geom("t2i", f"small_attn kind5 N{N} P{P} D{D}", (N, heads), 256, lds, f"hd={D // heads} scale=1 stride={P * D}"))


# the engine (api_trackwin.hip; P = 2048, C = 1408, C / 2 = 704, 8 heads; mini: 704 / 352): the prompt tokens' self attention, the
# projected-values forms (knobs track_fold_i2t / track_fold_t2i off; kinds 3 / 4 while the keys are shared), the folded t2i attention
# of the mini geometry (head dim 44: l4p_t2i_attn_scores)
for N_ in (64, 8):
    attn(f"engine_self_{N_}", ALL, 0, N_, 6, 1408, 8, "self6", (N_, 8), 64, 0)
    attn(f"mini_self_{N_}", ALL, 0, N_, 6, 704, 8, "self6", (N_, 8), 64, 0)
    for kind in (1, 3):
        attn(f"engine_t2i_{N_}", ALL, kind, N_, 2048, 704, 8, "t2i", (N_, 8), 256, 52480)
        attn(f"mini_t2i_{N_}", ALL, kind, N_, 2048, 352, 8, "t2i", (N_, 8), 256, 52480)
    for kind in (2, 4):
        attn(f"engine_i2t_{N_}", T16, kind, N_, 2048, 704, 8, "i2t_lds", (64, N_), 256, 78848)
        attn(f"engine_i2t_{N_}", (F32,), kind, N_, 2048, 704, 8, "i2t_lds", (64, N_), 256, 123904)
        attn(f"mini_i2t_{N_}", T16, kind, N_, 2048, 352, 8, "i2t_lds", (64, N_), 256, 39424)
        attn(f"mini_i2t_{N_}", (F32,), kind, N_, 2048, 352, 8, "i2t_lds", (64, N_), 256, 61952)
    scores(f"mini_{N_}", N_, 2048, 352, 8, 48, 52480)
    scores(f"engine_fold_v_off_{N_}", N_, 2048, 704, 8, 48, 52480)

# tests/kernel_refs.py ATTN_SHAPES, in its order: (t2i LDS bytes; i2t form, grid x, LDS bytes at 16 bits, at f32)
ATTN_WANT = [
    (52480, "i2t_lds", 64, 78848, 123904),   # hd 88: 11 key groups x 24 x 88 = 23232 < 24 P
    (26560, "i2t_lds", 2, 61952, 107008),    # P 96: 2304 + 3328 + (23232 - 2304); 64 rows per workgroup
    (27904, "i2t_lds", 32, 28672, 45056),    # hd 32: 32 key groups x 24 x 32 = 24576 > 24000
    (26368, "i2t", 1, 13824, 13824),         # hd 96: 10 x 24 x 96 = 23040 > 864; 256 % 3 != 0: direct, (36 * 3 + 255) / 256 workgroups
    (28000, "i2t", 25, 4608, 4608),          # hd 16: 64 x 24 x 16 = 24576 < 24672; 256 % 6 != 0: direct, (1028 * 6 + 255) / 256
    (27616, "i2t_lds", 16, 39424, 61952),    # hd 44: 23 x 24 x 44 = 24288 > 12288
    (27808, "i2t_lds", 9, 10752, 16896),     # hd 12: 85 x 24 x 12 = 24480 > 6240
]
assert len(ATTN_WANT) == len(R.ATTN_SHAPES)
for (N_, P_, D_, h_), (t2i_lds, i2t_form, i2t_gx, lds16, lds32) in zip(R.ATTN_SHAPES, ATTN_WANT):
    nm = f"gpu_{N_}x{P_}x{D_}x{h_}"
    for kind in (1, 3):
        attn(nm, ALL, kind, N_, P_, D_, h_, "t2i", (N_, h_), 256, t2i_lds)
    for kind in (2, 4):
        attn(nm, T16, kind, N_, P_, D_, h_, i2t_form, (i2t_gx, N_), 256, lds16)
        attn(nm, (F32,), kind, N_, P_, D_, h_, i2t_form, (i2t_gx, N_), 256, lds32)
    scores(nm, N_, P_, D_, h_, 6 * h_ + 4, t2i_lds)
# test_t2i_softmax_peaked_key_owned_by_the_fourth_wave; test_dynamic_lds_limit_small_then_over_64k_then_small
attn("gpu_peaked", ALL, 1, 2, 1000, 256, 8, "t2i", (2, 8), 256, 27904)
scores("gpu_peaked", 2, 1000, 256, 8, 48, 27904)
attn("gpu_lds_limit_P8", ALL, 1, 2, 8, 4, 1, "t2i", (2, 1), 256, 27904)
attn("gpu_lds_limit_P2688", ALL, 1, 2, 2688, 4, 1, "t2i", (2, 1), 256, 67840)
attn("gpu_lds_limit_D4", (F32,), 2, 2, 300, 4, 1, "i2t_lds", (2, 2), 256, 4288)
attn("gpu_lds_limit_D64", (F32,), 2, 2, 300, 64, 1, "i2t_lds", (2, 2), 256, 68608)
# D * esize % 16: D = 36 is whole 16-byte chunks at f32 (144), not at 16 bits (72)
attn("thr_chunks_D36", T16, 2, 1, 64, 36, 1, "i2t", (1, 1), 256, 1728)
attn("thr_chunks_D36", (F32,), 2, 1, 64, 36, 1, "i2t_lds", (1, 1), 256, 38592)
# the device's LDS.  t2i: 24 P + 3328 <= 163840 up to P = 6688, refused beyond (was: L4P_E_HIP from inside hipFuncSetAttribute).
attn("thr_lds_t2i_6688", ALL, 1, 2, 6688, 704, 8, "t2i", (2, 8), 256, 163840)
T_LDS = "invalid: {who}: P={P} {what} at head dim {hd} need {need} bytes of LDS, the device has 163840"
for d in ALL:
    for kind in (1, 3):
        case(f"attn lds refusal t2i kind={kind} dtype={d}", q("attn", dtype=d, kind=kind, N=2, P=6692, D=704, heads=8),
             T_LDS.format(who="small_attn", P=6692, what="keys", hd=88, need=163936))
case("scores thr_lds_6688", q("scores", N=2, P=6688, D=704, heads=8, ld=48), geom("t2i", "small_attn kind5 N2 P6688 D704", (2, 8), 256, 163840,
                                                                               "hd=88 scale=1 stride=4708352"))
case("scores lds refusal", q("scores", N=2, P=6692, D=704, heads=8, ld=48), T_LDS.format(who="t2i_attn_scores", P=6692, what="keys", hd=88, need=163936))
# i2t: a tile past the device's LDS takes the direct form (f32, 16 heads of 96: 73728 + 16 * 1536 * 4 = 172032; 16 bits: 122880 fits);
# the direct form's own rows fit up to D = 3413 (36 heads of 96: 165888, refused)
attn("thr_lds_i2t_tile", (F32,), 2, 2, 64, 1536, 16, "i2t", (4, 2), 256, 73728)
attn("thr_lds_i2t_tile", T16, 2, 2, 64, 1536, 16, "i2t_lds", (4, 2), 256, 122880)
attn("thr_lds_i2t_direct_fits", ALL, 2, 2, 64, 3360, 35, "i2t", (9, 2), 256, 161280)
for d in ALL:
    case(f"attn lds refusal i2t dtype={d}", q("attn", dtype=d, kind=2, N=2, P=64, D=3456, heads=36),
         T_LDS.format(who="small_attn", P=64, what="queries", hd=96, need=165888))
# a kind outside 0 .. 4 launches nothing and succeeds, as it always did
case("attn kind 7", q("attn", dtype=BF16, kind=7, N=2, P=64, D=352, heads=4), geom("none", "small_attn kind7 N2 P64 D352", (0, 0, 0), 0, 0,
                                                                                  "hd=88 scale=0.106600359 stride=0"))
# test_small_attn_refused_shapes_write_nothing
T_ATTN = "invalid: small_attn: unsupported head geometry D={D} heads={heads}"
for kind, N_, P_, D_, h_ in [(1, 2, 64, 1408, 8), (2, 2, 64, 1408, 8), (3, 2, 64, 1408, 8), (4, 2, 64, 1408, 8), (1, 2, 98, 352, 4), (3, 2, 98, 352, 4),
                             (1, 2, 64, 100, 3)]:
    for d in ALL:
        case(f"attn refusal kind={kind} P={P_} D={D_} dtype={d}", q("attn", dtype=d, kind=kind, N=N_, P=P_, D=D_, heads=h_), T_ATTN.format(D=D_, heads=h_))
T_SCORES = "invalid: t2i_attn_scores: D = heads * hd with hd % 4 == 0, hd <= 96, P % 4 == 0, ld_scores >= 6 * heads"
for ld, N_, P_, D_, h_ in [(24, 2, 98, 352, 4), (23, 2, 96, 352, 4), (48, 2, 96, 1408, 8)]:
    case(f"scores refusal ld={ld} P={P_} D={D_}", q("scores", N=N_, P=P_, D=D_, heads=h_, ld=ld), T_SCORES)
case("attn refusal heads 0", q("attn", dtype=BF16, kind=1, N=2, P=64, D=352, heads=0), T_ATTN.format(D=352, heads=0))


# ------------------------------------------------------------------------------------------------
# l4p_mask_product
# ------------------------------------------------------------------------------------------------
def mask(name, dtypes, N, vox, C, form, gx, block, lds):
    for d in dtypes:
        case(f"mask {name} dtype={d}", q("mask", dtype=d, N=N, vox=vox, C=C), geom(form, "mask_product", (gx, N), block, lds))


# tests/kernel_refs.py MASK_PRODUCT_C x engine dtype, every (vox, N) of the GPU tests: LDS bytes at 16 bits, at f32 (None: the direct form)
MASK_WANT = {176: (47168, 92224), 40: (10720, 20960), 352: (94336, None)}
assert sorted(MASK_WANT) == sorted(R.MASK_PRODUCT_C)
VOX_WANT = {640: (5, 3), 1000: (8, 4), 7: (1, 1)}  # vox: workgroups of the LDS form (128 voxels), of the direct form (256)
assert sorted(VOX_WANT) == sorted(R.MASK_PRODUCT_VOX)
for C_, (lds16, lds32) in MASK_WANT.items():
    for vox_, (g_lds, g_direct) in VOX_WANT.items():
        for N_ in sorted(set(R.MASK_PRODUCT_N) | {3}):
            mask(f"gpu_C{C_}_vox{vox_}_N{N_}", T16, N_, vox_, C_, "lds", g_lds, 128, lds16)
            if lds32 is None:  # f32, C = 352: 4224 + 128 * 352 * 4 = 184448 > 163840
                mask(f"gpu_C{C_}_vox{vox_}_N{N_}", (F32,), N_, vox_, C_, "direct", g_direct, 256, 12 * C_)
            else:
                mask(f"gpu_C{C_}_vox{vox_}_N{N_}", (F32,), N_, vox_, C_, "lds", g_lds, 128, lds32)
# both sides of the limit at f32: 524 C (+ rounding) against 163840
mask("thr_C312", (F32,), 1, 1000, 312, "lds", 8, 128, 163488)
mask("thr_C320", (F32,), 1, 1000, 320, "direct", 4, 256, 3840)
mask("thr_C320", T16, 1, 1000, 320, "lds", 8, 128, 85760)
mask("direct_grid_cap", (F32,), 2, 300000, 352, "direct", 1024, 256, 4224)
# test_dynamic_lds_limit_small_then_over_64k_then_small
mask("gpu_lds_limit_C8", T16, 2, 130, 8, "lds", 2, 128, 2144)
mask("gpu_lds_limit_C8", (F32,), 2, 130, 8, "lds", 2, 128, 4192)
mask("gpu_lds_limit_C128", (F32,), 2, 130, 128, "lds", 2, 128, 67072)
for d in ALL:
    case(f"mask refusal dtype={d}", q("mask", dtype=d, N=1, vox=100, C=12), "invalid: mask_product: C % 8 != 0")


# ------------------------------------------------------------------------------------------------
# l4p_track_readout
# ------------------------------------------------------------------------------------------------
def readout(name, N, T, h, w, H, W, wide_knob, form, lds):
    tag = "track_readout wide" if form == "wide" else "track_readout"
    case(f"readout {name} wide={wide_knob}", q("readout", N=N, T=T, h=h, w=w, H=H, W=W, **{"k.readout_wide": wide_knob, "k.track_deep": 1}),
         geom(form, tag, N * T, 1024 if form == "wide" else 256, lds))


# tests/kernel_refs.py READOUT_CASES: (column LDS bytes, wide LDS bytes)
READOUT_WANT = {"int4_nonsquare": (1232, 8016), "frac_small": (784, 5840), "row_tail": (784, 6800), "identity": (468, 1204),
                "wide_W": (7232, None), "many_groups": (784, None), "lds_over": (151424, None), "model": (38080, 70336)}
assert sorted(READOUT_WANT) == sorted(c[0] for c in R.READOUT_CASES)
for name_, (N_, T_), (h_, w_), (H_, W_), wide_ in R.READOUT_CASES:
    col, wid = READOUT_WANT[name_]
    assert wide_ == (wid is not None), name_  # the hand-kept flag of kernel_refs against the hand-worked sizes here ...
    readout(f"gpu_{name_}", N_, T_, h_, w_, H_, W_, 1, "wide" if wide_ else "column", wid if wide_ else col)  # ... and against the selection
    readout(f"gpu_{name_}", N_, T_, h_, w_, H_, W_, 0, "column", col)
# the engine (64 x 64 source maps, 16 frames of 224 x 224): 64 queries, a rank's shard of 8; test_kernels_gpu.py's 8 x 16 at 56 x 56
readout("engine_64", 64, 16, 64, 64, 224, 224, 1, "column", 49664)
readout("engine_8", 8, 16, 64, 64, 224, 224, 1, "wide", 81920)
readout("engine_8", 8, 16, 64, 64, 224, 224, 0, "column", 49664)
readout("gpu_kernels_8x16", 8, 16, 56, 56, 224, 224, 1, "wide", 70336)
readout("gpu_kernels_8x16", 8, 16, 56, 56, 224, 224, 0, "column", 38080)
# N T <= 512; W <= 256; the wide form's LDS (+ 128 static) against 163840.  (h w < 65536 cannot decide: 3 * 65536 * 4 is past the limit)
readout("thr_groups_512", 32, 16, 6, 10, 20, 36, 1, "wide", 5840)
readout("thr_groups_528", 33, 16, 6, 10, 20, 36, 1, "column", 784)
readout("thr_W_256", 1, 2, 8, 64, 16, 256, 1, "wide", 41376)
readout("thr_W_257", 1, 2, 8, 64, 16, 257, 1, "column", 6432)
readout("thr_wide_lds_fits", 1, 2, 110, 112, 16, 96, 1, "wide", 161912)
readout("thr_wide_lds_over", 1, 2, 112, 112, 16, 96, 1, "column", 151424)
readout("thr_lds_116", 1, 2, 116, 116, 16, 16, 1, "column", 162400)
T_RO_LDS = "invalid: track_readout: the {h} x {w} source maps need {need} bytes of LDS, the device has 163840"
T_RO_ARGS = "invalid: track_readout: needs every pointer and N, T, h, w, H, W >= 1 (N={N} T={T} h={h} w={w} H={H} W={W})"
for wide in (1, 0):
    case(f"readout refusal lds_117 wide={wide}", q("readout", N=1, T=2, h=117, w=117, H=16, W=16, **{"k.readout_wide": wide}), T_RO_LDS.format(h=117, w=117, need=165332))
    # test_readout_refusals_launch_nothing (its null-pointer cases are the launcher's own check, with the same text)
    case(f"readout refusal gpu_lds wide={wide}", q("readout", N=2, T=2, h=120, w=120, H=16, W=16, **{"k.readout_wide": wide}), T_RO_LDS.format(h=120, w=120, need=173888))
    for change in (dict(N=0), dict(T=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0)):
        a = dict(N=2, T=2, h=6, w=10, H=20, W=36)
        a.update(change)
        case(f"readout refusal {change} wide={wide}", q("readout", **a, **{"k.readout_wide": wide}), T_RO_ARGS.format(**a))
case("readout refusal N T past int", q("readout", N=65536, T=32768, h=6, w=10, H=20, W=36), T_RO_ARGS.format(N=65536, T=32768, h=6, w=10, H=20, W=36))

# ------------------------------------------------------------------------------------------------
# one form each: l4p_i2t_delta, l4p_t2i_probs, l4p_i2t_probs
# ------------------------------------------------------------------------------------------------
for d in T16:
    case(f"delta engine_64 dtype={d}", q("delta", dtype=d, N=64, P=2048, C=1408, K=64), geom("only", "M131072 N1408 K64 epi0 act0 delta t16x128 wgrp", (11, 64, 2), 256, 0))
    case(f"delta engine_8 dtype={d}", q("delta", dtype=d, N=8, P=2048, C=1408, K=64), geom("only", "M16384 N1408 K64 epi0 act0 delta t16x128 wgrp", (11, 8, 2), 256, 0))
    case(f"delta P_2000 dtype={d}", q("delta", dtype=d, N=8, P=2000, C=1408, K=64), geom("only", "M16000 N1408 K64 epi0 act0 delta t16x128 wgrp", (11, 8, 1), 256, 0))
T_DELTA = "invalid: i2t_delta: 16-bit engine, k = 64, C % 128 == 0, P % 16 == 0 (other shapes: the row-grouped-weights GEMM)"
for name, f in [("f32", dict(dtype=F32)), ("K_48", dict(K=48)), ("C_704", dict(C=704)), ("P_2040", dict(P=2040)), ("N_0", dict(N=0))]:
    a = dict(dtype=BF16, N=8, P=2048, C=1408, K=64)
    a.update(f)
    case(f"delta refusal {name}", q("delta", **a), T_DELTA)
case("t2i_probs engine_64", q("t2i_probs", N=64, P=2048, HT=48, ld=48), geom("only", "t2i_probs", (8, 64), 192, 0))
case("t2i_probs engine_8", q("t2i_probs", N=8, P=2048, HT=48, ld=48), geom("only", "t2i_probs", (8, 8), 192, 0))
case("t2i_probs gpu_608", q("t2i_probs", N=5, P=608, HT=48, ld=48), geom("only", "t2i_probs", (3, 5), 192, 0))
case("t2i_probs P_4096", q("t2i_probs", N=1, P=4096, HT=48, ld=52), geom("only", "t2i_probs", (16, 1), 192, 0))
T_T2I_PROBS = "invalid: t2i_probs: HT == 48, P <= 4096, score row stride >= HT and a multiple of 4"
for name, f in [("P_4097", dict(P=4097)), ("HT_64", dict(HT=64, ld=64)), ("ld_44", dict(ld=44)), ("ld_50", dict(ld=50)), ("N_0", dict(N=0))]:
    a = dict(N=8, P=2048, HT=48, ld=48)
    a.update(f)
    case(f"t2i_probs refusal {name}", q("t2i_probs", **a), T_T2I_PROBS)
I2T_PROBS = dict(M=131072, heads=8, tokens=6, ldp=64, ld=48, pairs=0, cbias=1, rpg=2048)
case("i2t_probs engine_64", q("i2t_probs", **I2T_PROBS), geom("only", "i2t_probs", 4096, 256, 0))
case("i2t_probs engine_64_pairs", q("i2t_probs", **dict(I2T_PROBS, ld=96, pairs=1)), geom("only", "i2t_probs", 4096, 256, 0))
case("i2t_probs engine_8", q("i2t_probs", **dict(I2T_PROBS, M=16384)), geom("only", "i2t_probs", 512, 256, 0))
case("i2t_probs grid_cap", q("i2t_probs", **dict(I2T_PROBS, M=1048576)), geom("only", "i2t_probs", 16384, 256, 0))
T_I2T_PROBS = "invalid: i2t_probs: 1 <= tokens <= 8, ldp >= tokens * heads, score row stride >= (pairs ? 2 : 1) * tokens * heads"
for name, f in [("tokens_9", dict(tokens=9, ldp=72, ld=72)), ("ldp_40", dict(ldp=40)), ("pairs_ld_48", dict(pairs=1)), ("rpg_0", dict(rpg=0)), ("heads_0", dict(heads=0))]:
    case(f"i2t_probs refusal {name}", q("i2t_probs", **dict(I2T_PROBS, **f)), T_I2T_PROBS)


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("track_select") / "track_select_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "track_select_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return exe


@pytest.fixture(scope="module")
def got(program):
    """the driver's answer to every query above, by case id: one process"""
    out = subprocess.run([program], input="\n".join(r[1] for r in ROWS) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return lines


def test_every_launch_reaches_its_form_and_geometry(got):
    wrong = [(i, g, w) for (i, _, w), g in zip(ROWS, got) if g != w]
    assert not wrong, f"{len(wrong)} of {len(got)} launches differ: {wrong[:8]}"


def test_the_cases_reach_every_form(got):
    forms = {g.split(" [")[0] for g in got if not g.startswith("invalid")}
    assert forms == {"ctx_f32", "ctx_mfma64", "ctx_ring4", "ctx_ring8", "ctx_ring12", "none", "self6", "t2i", "i2t_lds", "i2t", "lds", "direct",
                     "wide", "column", "only"}, forms


def test_the_track_deep_comparisons_of_the_gpu_tests_compare_two_forms(got):
    """test_t2i_context_two_stages_per_barrier_equals_the_chip_filling_form compares track_deep 1 and 0 bit for bit under one profiler
    tag: here, that the two settings reach DIFFERENT kernels at each of its shapes (and the same shared_from)."""
    by_id = {i: g for (i, _, _), g in zip(ROWS, got)}
    for N_, P_, form_, _ in CTX_AB:
        for sf in (P_, P_ // 2 // 32 * 32):
            for d in T16:
                deep, flat = (by_id[f"ctx gpu_ab_{N_}x{P_}_sf{sf} dtype={d} deep={k}"] for k in (1, 0))
                assert deep.split(" [")[0] == form_ and flat.split(" [")[0] == "ctx_ring4"
                assert deep.split("]")[0].split("[")[1] == flat.split("]")[0].split("[")[1]  # one tag: the GPU test cannot see it
                assert deep.rsplit(" ", 1)[1] == flat.rsplit(" ", 1)[1] == f"shared_from={sf}"


def test_readout_cases_say_which_form_they_reach(got):
    """kernel_refs.READOUT_CASES' hand-kept `wide` flag (what test_track_tail_gpu.py expects as the launch's tag) against the selection"""
    by_id = {i: g for (i, _, _), g in zip(ROWS, got)}
    for name_, *_rest, wide_ in R.READOUT_CASES:
        assert by_id[f"readout gpu_{name_} wide=1"].startswith("wide [track_readout wide]" if wide_ else "column [track_readout]"), name_
        assert by_id[f"readout gpu_{name_} wide=0"].startswith("column [track_readout]"), name_


def test_default_knobs_match_the_library_table():
    """KNOB_DEFAULTS above against csrc/prof.hip's table, read as text"""
    table = dict(re.findall(r'\{"(\w+)", "L4P_\w+", (-?\d+)\}', open(os.path.join(ROOT, "l4p_amd", "csrc", "prof.hip")).read()))
    for name, value in KNOB_DEFAULTS.items():
        assert int(table[name]) == value, name
