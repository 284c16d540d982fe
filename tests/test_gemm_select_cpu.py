"""The launcher's kernel-form selection (csrc/gemm_select.hpp) on the host: every case of tests/test_gemm_forms_gpu.py reaches the
form it is about - checked without a GPU.

tests/gemm_select_main.cpp includes gemm_select.hpp alone (plain C++17, no HIP) and answers one descriptor + knob set per input line
with the tail of the profiler tag the launch would carry, or with the refusal's error text.  The descriptors are desc_fields(case) of
tests/gemm_forms_cases.py: the same integers the GPU test puts into its l4p_gemm_desc.  All cases go through one process.
"""
import os
import re
import shutil
import subprocess

import pytest

from l4p_amd._lib import L4P_F32
from tests import gemm_forms_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

# The defaults of the knobs the selection reads: what csrc/prof.hip's table must hold (probe_kernels: 0 in the shipped build).
# epi_generic is not read by the selection: the launcher turns it into bit 0 of l4p_gemm_desc.tuning in front of it.
KNOB_DEFAULTS = {"gemm_variant": 0, "conv_halo": 1, "gemm_skinny": 1, "skinny_max_m": 128, "gemm_deep": 1, "gemm_group": 1,
                 "track_deep": 1, "gemm_t192": 1, "gemm_4w": 0, "probe_kernels": 0, "epi_generic": 0}
KW_COLS_TEXT = "l4p_gemm: kw_cols needs a dense GEMM without split-K / row groups, kw_cols a multiple of 128"
WGR_TEXT = "l4p_gemm: row-grouped weights need a dense GEMM without split-K, w_gr a multiple of 128"
UPS_TEXT = "conv3d: the fused up-sampling loader (l4p_gemm_desc.ups_hi) is a measured-and-not-adopted form: build with PROBES=1"


def _esize(mode):
    return 4 if mode == L4P_F32 else 2


def _members(*fields):
    return " ; ".join(" ".join(f"{k}={v}" for k, v in f.items()) for f in fields)


def query(kind, fields, knobs=(), mode=0, es=2):
    """one input line: fields = one dict of descriptor fields (a group: a list of them); knobs overlay KNOB_DEFAULTS"""
    k = dict(KNOB_DEFAULTS, **dict(knobs))
    members = fields if isinstance(fields, (list, tuple)) else [fields]
    members = [dict(f) for f in members]
    if k.pop("epi_generic"):
        for f in members:
            f["tuning"] = f.get("tuning", 0) | 1
    return f"{kind} es={es} mode={mode} {_members(*members)} " + " ".join(f"k.{name}={v}" for name, v in k.items())


def case_query(case):
    return query("gemm", G.desc_fields(case), case.knobs, mode=1 if case.conv else 0, es=_esize(case.mode))


def dense(M, N, K, **kw):
    """a plain bf16 dense GEMM, out_T only, unpadded"""
    return dict(dict(A=1, W=1, bias=1, out_T=1, M=M, N=N, K=K, lda=K, ldw=K, ldc=N), **kw)


def subpixel(M, cin, cout, k):
    """l4p_conv3d_subpixel as launch_gemm hands it on: K = ldw = cells * Cin, N = kt * kh * kw * Cout, epi = ConvTranspose"""
    cells = 1
    for a in k:
        cells *= 3 if a == 1 else 2
    return dict(A=1, W=1, bias=1, out_T=1, M=M, N=k[0] * k[1] * k[2] * cout, K=cells * cin, ldw=cells * cin, Cin=cin, Cout=cout,
                kt=k[0], kh=k[1], kw=k[2], Ti=8, Hi=32, Wi=32, To=8, Ho=32, Wo=32, st=1, sh=1, sw=1, epi=2)


HALO_VOLUME = dict(Ti=2, Hi=64, Wi=96, To=2, Ho=64, Wo=96, st=1, sh=1, sw=1, Cin=64)
# Forms that ALL_CASES does not hold: (name, input line, expected answer).  bf16, default knobs unless said otherwise.
EXTRA = [
    ("skinny", query("gemm", dense(48, 1408, 1408)), "skinny"),
    ("skinny_off", query("gemm", dense(48, 1408, 1408), {"gemm_skinny": 0}), "sk1 t128x64 deep"),
    ("skinny_129_rows", query("gemm", dense(129, 1408, 1408)), "sk1 t128x64 deep"),                # skinny_max_m = 128
    ("skinny_1056_blocks", query("gemm", dense(48, 11264, 704)), "sk1 t128x64 deep"),              # 3 x 352 output blocks > 512
    ("skinny_wgrp", query("gemm", dense(1024, 88, 1408, w_gr=128, w_gs=88 * 1408, b_gs=88)), "wgrp skinny"),
    ("subpix_8p", query("gemm", subpixel(8192, 64, 256, (2, 2, 2)), mode=2), "K512 subpix 8p t256x256"),
    ("subpix_staged", query("gemm", subpixel(8192, 64, 256, (2, 2, 2)), {"gemm_variant": 1}, mode=2), "K512 subpix t128x128"),
    ("group_deep", query("group", [dense(200, 256, 384)] * 2), "group: t128x64 deep"),
    ("group_skinny", query("group", [dense(48, 1408, 1408)] * 3), "group: skinny"),
    ("group_splitk_member", query("group", [dense(200, 256, 384), dense(200, 256, 384, splitk=2, partial=1)]), "group: one by one"),
    ("refuse_kw_cols", query("gemm", dense(200, 256, 384, kw_cols=64, kw_len=1)), "invalid: " + KW_COLS_TEXT),
    ("refuse_kw_cols_group", query("group", [dense(200, 256, 384, kw_cols=64, kw_len=1), dense(200, 256, 384)]), "invalid: " + KW_COLS_TEXT),
    ("refuse_w_gr", query("gemm", dense(300, 56, 392, w_gr=100, w_gs=56 * 392, b_gs=56)), "invalid: " + WGR_TEXT),
    ("refuse_ups", query("gemm", dict(dense(2 * 2 * 64 * 96, 128, 27 * 64, lda=0, ups_hi=32, ups_wi=48), **HALO_VOLUME), mode=1),
     "invalid: " + UPS_TEXT),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_select") / "gemm_select_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_select_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return exe


def answers(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def test_every_case_of_the_form_tests_reaches_its_form(program):
    """ALL_CASES, the 2 x 2 x 2 x 62 sweep cases among them, with each case's own element type and knobs: the selection's tag tail
    equals case.form."""
    assert len(G.SWEEP_CASES) == 2 * 2 * 2 * 62
    got = answers(program, [case_query(c) for c in G.ALL_CASES])
    wrong = [(G.case_id(c), g) for c, g in zip(G.ALL_CASES, got) if g != c.form]
    assert not wrong, f"{len(wrong)} of {len(got)} cases reach another form: {wrong[:8]}"


def test_the_cases_cover_the_forms_a_shipped_build_can_pick(program):
    """every tag tail the selection can name, but the probe-only forms, is reached by a case here or by an extra case below"""
    got = set(answers(program, [case_query(c) for c in G.ALL_CASES] + [line for _, line, _ in EXTRA]))
    tails = {g.split(" ", 1)[1] if g.startswith("K") else g for g in got}
    for tail in ("sk1 t128x64", "sk1 t128x64 deep", "sk1 t128x128", "sk3 t128x64", "sk3 t128x128", "sk1 t64x64 deep wgrp",
                 "sk1 t128x64 deep wgrp", "sk1 t128x64 wgrp", "sk1 t128x128 wgrp", "8p t256x256", "8p t256x192", "8p sk4 t256x256",
                 "8p sk4 t256x192", "halo t256x256", "halo t512x128", "skinny", "wgrp skinny", "subpix t128x128", "subpix 8p t256x256"):
        assert tail in tails, tail


@pytest.mark.parametrize("name,line,want", EXTRA, ids=[e[0] for e in EXTRA])
def test_forms_and_refusals_outside_the_form_tests(program, name, line, want):
    assert answers(program, [line]) == [want]


def test_default_knobs_match_the_library_table():
    """KNOB_DEFAULTS above against csrc/prof.hip's table, read as text"""
    table = dict(re.findall(r'\{"(\w+)", "L4P_\w+", (-?\d+)\}', open(os.path.join(ROOT, "l4p_amd", "csrc", "prof.hip")).read()))
    for name, value in KNOB_DEFAULTS.items():
        if name != "probe_kernels":
            assert int(table[name]) == value, name
