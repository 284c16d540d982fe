"""The encoder attention's kernel-form selection (csrc/attn_select.hpp) on the host: which kernel form, grid, block and LDS size
every l4p_attention launch gets - the engine's launches, both sides of every threshold, and every case of the GPU tests - checked
without a GPU.  The GPU tests reach forms through knobs and assert the profiler tag of the launches they make; they cannot see the
geometry, nor a threshold that has moved.  This test can.

tests/attn_select_main.cpp includes attn_select.hpp alone (plain C++17, no HIP) and answers one launch + knob set per input line with
"<tag> | ntiles grid block lds persistent c_scale", or with the refusal's error text.  The expected values are literals written out
by hand from the launcher's conditions.  All cases go through one process.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

BF16, F32, F16 = 0, 1, 2  # include/l4p_hip.h
KNOB_DEFAULTS = {"attn_variant": 0, "attn_persist": 1, "attn64": 1}
# the scale-inside form, scale = Dh ** -0.5 (ops.attention's default): (scale, c_scale = float(scale) * float(log2 e) in float arithmetic)
SCALE_OF = {88: ("0.10660036", "0.1537918"), 64: ("0.125", "0.180336878")}
ALL_TAGS = ("f32", "unsplit", "unsplit cs", "kvsplit", "kvsplit cs", "qsplit persist", "qsplit pertile", "rows64")


def query(dtype, B, S, H, Dh, scale=0, **knobs):
    k = dict(KNOB_DEFAULTS, **knobs)
    return f"attn dtype={dtype} B={B} S={S} H={H} Dh={Dh} scale={scale} " + " ".join(f"k.{n}={v}" for n, v in k.items())


def geom(tag, ntiles, grid, block, lds, persistent):
    return f"{tag} | ntiles={ntiles} grid={grid} block={block} lds={lds} persistent={persistent}"


# ---- (name, dtypes, query arguments, knobs, expected "<tag> | geometry" without c_scale) ----
T16 = (BF16, F16)
CASES = [
    # the engine: H = 16, Dh = 88, pre-scaled q
    ("engine_B1_S2048", T16, (1, 2048, 16, 88), {}, geom("kvsplit", 256, 256, 512, 98304, 0)),
    ("engine_B2_S2048", T16, (2, 2048, 16, 88), {}, geom("rows64", 256, 256, 256, 98304, 1)),
    ("engine_B2_S2048_no64", T16, (2, 2048, 16, 88), dict(attn64=0), geom("unsplit", 512, 512, 256, 49152, 0)),
    ("engine_B4_S2048", T16, (4, 2048, 16, 88), {}, geom("rows64", 512, 256, 256, 98304, 1)),
    ("engine_B4_S2048_no64", T16, (4, 2048, 16, 88), dict(attn64=0), geom("qsplit persist", 512, 256, 512, 98304, 1)),
    ("engine_B4_S2048_no64_pertile", T16, (4, 2048, 16, 88), dict(attn64=0, attn_persist=0), geom("qsplit pertile", 512, 512, 512, 98304, 0)),
    ("engine_B4_S2048_no64_noqsplit", T16, (4, 2048, 16, 88), dict(attn64=0, attn_variant=2), geom("unsplit", 1024, 1024, 256, 49152, 0)),
    ("engine_B4_S2048_variant2_keeps_64_off", T16, (4, 2048, 16, 88), dict(attn_variant=2), geom("unsplit", 1024, 1024, 256, 49152, 0)),
    ("engine_B1_S1152", T16, (1, 1152, 16, 88), {}, geom("kvsplit", 144, 144, 512, 98304, 0)),
    ("engine_f32_B1_S2048", (F32,), (1, 2048, 16, 88), {}, geom("f32", 256, 256, 256, 49152, 0)),
    ("engine_f32_B4_S2048", (F32,), (4, 2048, 16, 88), {}, geom("f32", 1024, 1024, 256, 49152, 0)),
    # head dim 64 where the query split would apply: there is no 64-wide query-split instantiation
    ("dh64_no_query_split", T16, (32, 256, 16, 64), dict(attn64=0), geom("unsplit", 1024, 1024, 256, 49152, 0)),
    ("dh64_rows64", T16, (32, 256, 16, 64), {}, geom("rows64", 512, 256, 256, 98304, 1)),
    # both sides of every threshold, H = 1
    ("thr_S128_B511", T16, (511, 128, 1, 88), {}, geom("kvsplit", 511, 511, 512, 98304, 0)),  # one KV block per wave group
    ("thr_S128_B512", T16, (512, 128, 1, 88), {}, geom("unsplit", 512, 512, 256, 49152, 0)),
    ("thr_S256_B255", T16, (255, 256, 1, 88), {}, geom("kvsplit", 510, 510, 512, 98304, 0)),
    ("thr_S256_B256", T16, (256, 256, 1, 88), {}, geom("rows64", 256, 256, 256, 98304, 1)),
    ("thr_S256_B257", T16, (257, 256, 1, 88), {}, geom("rows64", 257, 256, 256, 98304, 1)),
    ("thr_S256_B511_no64", T16, (511, 256, 1, 88), dict(attn64=0), geom("unsplit", 1022, 1022, 256, 49152, 0)),
    ("thr_S256_B512_no64", T16, (512, 256, 1, 88), dict(attn64=0), geom("qsplit persist", 512, 256, 512, 98304, 1)),
    # ---- tests/test_attention_forms_gpu.py, pre-scaled cases ----
    ("gpu_kvsplit_nit3", T16, (1, 384, 2, 88), {}, geom("kvsplit", 6, 6, 512, 98304, 0)),
    ("gpu_kvsplit_nit5", T16, (1, 640, 3, 64), {}, geom("kvsplit", 15, 15, 512, 98304, 0)),
    ("gpu_kvsplit_cs", T16, (1, 384, 2, 88), dict(attn_variant=1), geom("kvsplit cs", 6, 6, 512, 98304, 0)),
    ("gpu_unsplit_88", T16, (11, 384, 16, 88), {}, geom("unsplit", 528, 528, 256, 49152, 0)),
    ("gpu_unsplit_64", T16, (11, 384, 16, 64), {}, geom("unsplit", 528, 528, 256, 49152, 0)),
    ("gpu_unsplit_cs", T16, (11, 384, 16, 64), dict(attn_variant=1), geom("unsplit cs", 528, 528, 256, 49152, 0)),
    ("gpu_qsplit_32x256", T16, (32, 256, 16, 88), dict(attn64=0), geom("qsplit persist", 512, 256, 512, 98304, 1)),
    ("gpu_qsplit_32x256_pertile", T16, (32, 256, 16, 88), dict(attn64=0, attn_persist=0), geom("qsplit pertile", 512, 512, 512, 98304, 0)),
    ("gpu_qsplit_33x256", T16, (33, 256, 16, 88), dict(attn64=0), geom("qsplit persist", 528, 256, 512, 98304, 1)),
    ("gpu_qsplit_33x256_pertile", T16, (33, 256, 16, 88), dict(attn64=0, attn_persist=0), geom("qsplit pertile", 528, 528, 512, 98304, 0)),
    ("gpu_qsplit_8x1024", T16, (8, 1024, 16, 88), dict(attn64=0), geom("qsplit persist", 512, 256, 512, 98304, 1)),
    ("gpu_qsplit_8x1024_pertile", T16, (8, 1024, 16, 88), dict(attn64=0, attn_persist=0), geom("qsplit pertile", 512, 512, 512, 98304, 0)),
    ("gpu_no_query_split_aid", T16, (32, 256, 16, 88), dict(attn64=0, attn_variant=2), geom("unsplit", 1024, 1024, 256, 49152, 0)),
    ("gpu_rows64_three_tiles_88", T16, (11, 768, 8, 88), {}, geom("rows64", 264, 256, 256, 98304, 1)),
    ("gpu_rows64_three_tiles_64", T16, (11, 768, 8, 64), {}, geom("rows64", 264, 256, 256, 98304, 1)),
    ("gpu_rows64_three_tiles_88_no64", T16, (11, 768, 8, 88), dict(attn64=0), geom("unsplit", 528, 528, 256, 49152, 0)),
    ("gpu_rows64_three_tiles_64_no64", T16, (11, 768, 8, 64), dict(attn64=0), geom("unsplit", 528, 528, 256, 49152, 0)),
    ("gpu_f32_s384_88", (F32,), (1, 384, 2, 88), {}, geom("f32", 6, 6, 256, 49152, 0)),
    ("gpu_f32_s384_64", (F32,), (1, 384, 3, 64), {}, geom("f32", 9, 9, 256, 49152, 0)),
    # ---- tests/test_kernels_gpu.py: test_qkv_attention, test_attention_peaked_softmax, test_attention_very_negative_and_huge_scores ----
    ("gpu_qkv_2x256", T16, (2, 256, 2, 88), {}, geom("kvsplit", 8, 8, 512, 98304, 0)),
    ("gpu_qkv_1x128", T16, (1, 128, 3, 64), {}, geom("kvsplit", 3, 3, 512, 98304, 0)),
    ("gpu_qkv_1x384_64", T16, (1, 384, 3, 64), {}, geom("kvsplit", 9, 9, 512, 98304, 0)),
    ("gpu_peaked_512", T16, (1, 512, 2, 88), {}, geom("kvsplit", 8, 8, 512, 98304, 0)),
    ("gpu_very_negative", T16, (1, 256, 2, 88), {}, geom("kvsplit", 4, 4, 512, 98304, 0)),
    ("gpu_qkv_f32_1x2048", (F32,), (1, 2048, 16, 88), {}, geom("f32", 256, 256, 256, 49152, 0)),
    ("gpu_qkv_f32_2x256", (F32,), (2, 256, 2, 88), {}, geom("f32", 8, 8, 256, 49152, 0)),
    ("gpu_qkv_f32_1x128", (F32,), (1, 128, 3, 64), {}, geom("f32", 3, 3, 256, 49152, 0)),
    ("gpu_peaked_f32_512", (F32,), (1, 512, 2, 88), {}, geom("f32", 8, 8, 256, 49152, 0)),
    # ---- tests/test_kernels_gpu.py: test_attention64_forms_and_the_8_wave_kernel (attn64 = 1, then 0) ----
    ("gpu_a64_2x2048", T16, (2, 2048, 16, 88), {}, geom("rows64", 256, 256, 256, 98304, 1)),
    ("gpu_a64_3x2048", T16, (3, 2048, 16, 88), {}, geom("rows64", 384, 256, 256, 98304, 1)),
    ("gpu_a64_3x2048_no64", T16, (3, 2048, 16, 88), dict(attn64=0), geom("unsplit", 768, 768, 256, 49152, 0)),
    ("gpu_a64_11x1024", T16, (11, 1024, 6, 88), {}, geom("rows64", 264, 256, 256, 98304, 1)),
    ("gpu_a64_11x1024_no64", T16, (11, 1024, 6, 88), dict(attn64=0), geom("unsplit", 528, 528, 256, 49152, 0)),
    ("gpu_a64_4x2048_dh64", T16, (4, 2048, 16, 64), {}, geom("rows64", 512, 256, 256, 98304, 1)),
    ("gpu_a64_4x2048_dh64_no64", T16, (4, 2048, 16, 64), dict(attn64=0), geom("unsplit", 1024, 1024, 256, 49152, 0)),
    ("gpu_a64_16x256", T16, (16, 256, 16, 88), {}, geom("rows64", 256, 256, 256, 98304, 1)),
    ("gpu_a64_16x256_no64", T16, (16, 256, 16, 88), dict(attn64=0), geom("unsplit", 512, 512, 256, 49152, 0)),
    ("gpu_a64_8x1024", T16, (8, 1024, 16, 88), {}, geom("rows64", 512, 256, 256, 98304, 1)),
]

# the scale inside (scale = Dh^-0.5 > 0): bf16 is diverted to the compiler-scheduled bodies, f16 and f32 go where pre-scaled q goes
# (name, query arguments, knobs, expected per dtype)
def kv(n, f32=True):
    """a KV-split launch of n tiles in the three dtypes (f32: its own kernel, one workgroup of 4 waves per tile)"""
    d = {BF16: geom("kvsplit cs", n, n, 512, 98304, 0), F16: geom("kvsplit", n, n, 512, 98304, 0)}
    if f32:
        d[F32] = geom("f32", n, n, 256, 49152, 0)
    return d


SCALE_INSIDE = [
    ("B4_S2048", (4, 2048, 16, 88), {}, {BF16: geom("unsplit cs", 1024, 1024, 256, 49152, 0), F16: geom("rows64", 512, 256, 256, 98304, 1),
                                         F32: geom("f32", 1024, 1024, 256, 49152, 0)}),
    ("B4_S2048_no64", (4, 2048, 16, 88), dict(attn64=0), {BF16: geom("unsplit cs", 1024, 1024, 256, 49152, 0),
                                                          F16: geom("qsplit persist", 512, 256, 512, 98304, 1)}),
    ("B1_S2048", (1, 2048, 16, 88), {}, {BF16: geom("kvsplit cs", 256, 256, 512, 98304, 0), F16: geom("kvsplit", 256, 256, 512, 98304, 0),
                                         F32: geom("f32", 256, 256, 256, 49152, 0)}),
    # tests/test_attention_forms_gpu.py test_kv_split_odd_blocks_per_wave_group / test_kv_split_compiler_scheduled / test_f32_kernel_at_s_384,
    # scale inside (the f32 rows of the first two: test_qkv_attention as well)
    ("gpu_kvsplit_nit3", (1, 384, 2, 88), {}, kv(6)),
    ("gpu_kvsplit_nit5_dh64", (1, 640, 3, 64), {}, kv(15, f32=False)),
    ("gpu_kvsplit_nit9", (1, 1152, 16, 88), {}, kv(144, f32=False)),
    ("gpu_f32_s384_dh64", (1, 384, 3, 64), {}, kv(9)),  # (16-bit: test_qkv_attention)
    ("gpu_kvsplit_cs", (1, 384, 2, 88), dict(attn_variant=1), {BF16: geom("kvsplit cs", 6, 6, 512, 98304, 0), F16: geom("kvsplit cs", 6, 6, 512, 98304, 0)}),
    # tests/test_kernels_gpu.py, scale inside, three modes each: test_qkv_attention (its (1, 2048, 16, 88), (1, 384, 2, 88) and (1, 384, 3, 64)
    # are B1_S2048, gpu_kvsplit_nit3 and gpu_f32_s384_dh64 above), test_attention_peaked_softmax (its (2048, 4, 16) is B4_S2048),
    # test_attention_very_negative_and_huge_scores
    ("gpu_qkv_2x256", (2, 256, 2, 88), {}, kv(8)),
    ("gpu_qkv_1x128_dh64", (1, 128, 3, 64), {}, kv(3)),
    ("gpu_peaked_512", (1, 512, 2, 88), {}, kv(8)),
    ("gpu_very_negative", (1, 256, 2, 88), {}, kv(4)),
]

# tests/test_attention_forms_gpu.py test_argument_errors: B = 1, H = 2, bf16
T_REFUSE = "invalid: attention: need S % 128 == 0, head_dim in {{88, 64}} and scale >= 0 (S={S} Dh={Dh} scale={scale})"
REFUSALS = [
    ("S_192", (1, 192, 2, 88), "0", T_REFUSE.format(S=192, Dh=88, scale="0")),
    ("Dh_80", (1, 256, 2, 80), "0", T_REFUSE.format(S=256, Dh=80, scale="0")),
    ("scale_negative", (1, 256, 2, 88), "-1", T_REFUSE.format(S=256, Dh=88, scale="-1")),
    ("scale_nan", (1, 256, 2, 88), "nan", T_REFUSE.format(S=256, Dh=88, scale="nan")),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_select") / "attn_select_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "attn_select_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return exe


def answers(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def all_queries():
    """(id, query line, expected answer) of every case above"""
    rows = []
    for name, dtypes, args, knobs, want in CASES:
        for d in dtypes:
            rows.append((f"{name} dtype={d}", query(d, *args, **knobs), want + " c_scale=1"))
    for name, args, knobs, per_dtype in SCALE_INSIDE:
        for d, want in per_dtype.items():
            scale, c_scale = SCALE_OF[args[3]]
            rows.append((f"scale_inside_{name} dtype={d}", query(d, *args, scale=scale, **knobs), want + " c_scale=" + c_scale))
    return rows


def test_every_launch_reaches_its_form_and_geometry(program):
    rows = all_queries()
    got = answers(program, [r[1] for r in rows])
    wrong = [(i, g, w) for (i, _, w), g in zip(rows, got) if g != w]
    assert not wrong, f"{len(wrong)} of {len(got)} launches differ: {wrong[:8]}"


def test_the_cases_reach_every_form(program):
    tags = {g.split(" | ")[0] for g in answers(program, [r[1] for r in all_queries()])}
    assert tags == set(ALL_TAGS), tags  # one tag per AttnForm, two for the query split


@pytest.mark.parametrize("name,args,scale,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_message(program, name, args, scale, text):
    lines = [query(d, *args, scale=scale, attn_variant=v, attn_persist=p, attn64=a) for d in (BF16, F32, F16) for v in (0, 1, 2) for p in (0, 1) for a in (0, 1)]
    assert answers(program, lines) == [text] * len(lines)


def test_default_knobs_match_the_library_table():
    """KNOB_DEFAULTS above against csrc/prof.hip's table, read as text"""
    table = dict(re.findall(r'\{"(\w+)", "L4P_\w+", (-?\d+)\}', open(os.path.join(ROOT, "l4p_amd", "csrc", "prof.hip")).read()))
    for name, value in KNOB_DEFAULTS.items():
        assert int(table[name]) == value, name
