"""The LayerNorm launcher's kernel-form selection (csrc/ln_select.hpp) on the host: which kernel form every LayerNorm launch of the
engine reaches, at full geometry and at the smallest ragged shapes of the GPU tests - checked without a GPU.  The bitwise GPU tests
compare forms through the knobs; they cannot see a launch that falls back to the row form.  This test can.

tests/ln_select_main.cpp includes ln_select.hpp alone (plain C++17, no HIP) and answers one LnParams + knob set per input line with
"<form>[ <slots>]", or with the refusal's error text.  The cases are literals that restate the call sites of csrc/api.hip and
csrc/api_trackwin.hip; the expected forms are written out by hand from the launchers' conditions.  All cases go through one process.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

BF16, F32, F16 = 0, 1, 2  # include/l4p_hip.h
DTYPES = (BF16, F32, F16)
ROWS, RES, CHAIN = 0, 1, 2  # LnKind
KNOB_DEFAULTS = {"ln_tracks": 1, "ln_rows16": 1}


def query(dtype, tracks, rows16, **fields):
    return f"ln dtype={dtype} " + " ".join(f"{k}={v}" for k, v in fields.items()) + f" k.ln_tracks={tracks} k.ln_rows16={rows16}"


# ---- the engine's launches: (name, LnParams fields, expected) ----
# expected: a string, or a function (dtype, ln_tracks, ln_rows16) -> string
CASES = []

# the encoder (csrc/api.hip), batch 4: M = 8192 rows of C = 1408
ENC = dict(M=8192, C=1408, x=1, gamma=1, beta=1, out_T=1)
CASES += [
    ("enc_plain", dict(ENC, kind=ROWS), "row 6"),
    ("enc_tap", dict(ENC, kind=ROWS, out_f32=1), "row 6"),
    ("enc_delta_sum", dict(ENC, kind=RES, delta_T=1, out_sum=1), "row res 6"),
    ("enc_partials_2", dict(ENC, kind=RES, part=1, pbias=1, nsplit=2, out_sum=1), "row part 6"),
    ("enc_partials_8", dict(ENC, kind=RES, part=1, pbias=1, nsplit=8, out_sum=1), "row part 6"),
]

# the tracker window (csrc/api_trackwin.hip): N tracks of P tokens, C channels
for N, P in ((64, 2048), (3, 8)):
    for C, row, row_res in ((1408, "row 6", "row res 6"), (352, "row 2", "row res 2")):  # (the row forms' names, written out)
        key = dict(M=N * P, C=C, x=1, gamma=1, beta=1, delta_T=1, add=1, add_mod=P, out_T=1, out_T2=1)
        tag = f"N{N}_P{P}_C{C}"
        CASES += [
            # first window, layer 0: every float row shared, statistics kept for the chained layer 1
            (f"key_l0_shared_stats_{tag}", dict(key, kind=RES, x_mod=P, out_stats=1), lambda d, t, r, rr=row_res: "token shared" if t else rr),
            # ... without the chain (track_ln_chain = 0): the float master is written
            (f"key_l0_shared_f32_{tag}", dict(key, kind=RES, x_mod=P, out_f32=1), lambda d, t, r, rr=row_res: "token shared" if t else rr),
            # first window, layer 1: chained
            (f"key_l1_chained_{tag}", dict(key, kind=CHAIN, x_mod=P, dprev_T=1, stats_in=1, g0=1, b0=1, out_f32=1),
             lambda d, t, r: "token chain" if t else "row chain"),
            # later window: the tracks' own master, in place
            (f"key_own_in_place_{tag}", dict(key, kind=RES, out_f32=1), lambda d, t, r, rr=row_res: "token own" if t else rr),
            # later window, layer 0 half-shared: tokens from P / 2 on still come from the common rows
            (f"key_half_shared_{tag}", dict(key, kind=RES, out_f32=1, x_shared=1, x_period=P, x_split=P // 2),
             lambda d, t, r, rr=row_res: "token own" if t else rr),
            # the last layer: nothing adds to the float keys any more
            (f"key_last_layer_{tag}", dict(key, kind=RES), lambda d, t, r, rr=row_res: "token own" if t else rr),
            # the prompt tokens: 6 N rows with their addend; the final norm in place
            (f"tokens_{tag}", dict(kind=ROWS, M=6 * N, C=C, x=1, gamma=1, beta=1, add=1, add_mod=6 * N, out_T=1, out_T2=1, out_f32=1), row),
            (f"tokens_final_{tag}", dict(kind=ROWS, M=6 * N, C=C, x=1, gamma=1, beta=1, out_T=1, out_f32=1), row),
        ]

# LayerNorm3d + GELU of the tracker's up-scaling: rows stored in the engine dtype, in place
LN3D = dict(kind=ROWS, x_is_T=1, x=1, gamma=1, beta=1, out_T=1, act=1)
CASES += [
    ("ln3d_2^20_C352", dict(LN3D, M=1 << 20, C=352), lambda d, t, r: "row 2" if d == F32 else "rows16 6" if r else "row T 2"),
    ("ln3d_4095_C352", dict(LN3D, M=4095, C=352), lambda d, t, r: "row 2" if d == F32 else "row T 2"),  # fewer than 4096 rows
    ("ln3d_4096_C512", dict(LN3D, M=4096, C=512), lambda d, t, r: "row 2" if d == F32 else "rows16 8" if r else "row T 2"),
    ("ln3d_4096_C384", dict(LN3D, M=4096, C=384), lambda d, t, r: "row 2" if d == F32 else "rows16 6" if r else "row T 2"),
    ("ln3d_4096_C516", dict(LN3D, M=4096, C=516), lambda d, t, r: "row 6" if d == F32 else "row T 6"),  # past the short rows
]

# the smallest ragged shapes of the GPU tests (tests/test_kernels_gpu.py, tests/kernel_refs.py LN_SHAPES)
PLAIN = dict(kind=ROWS, x=1, gamma=1, beta=1, out_T=1, out_f32=1)
CASES += [
    ("gpu_37x352", dict(PLAIN, M=37, C=352), "row 2"),
    ("gpu_6x176", dict(PLAIN, M=6, C=176), "row 2"),
    ("gpu_2048x1408", dict(PLAIN, M=2048, C=1408), "row 6"),
    ("gpu_5x1540", dict(PLAIN, M=5, C=1540), "row 8"),  # the first width that takes the seventh slot
    ("gpu_6x2048", dict(PLAIN, M=6, C=2048), "row 8"),
    ("gpu_T_5x1408", dict(LN3D, M=5, C=1408), lambda d, t, r: "row 6" if d == F32 else "row T 6"),
    ("gpu_T_5x1540", dict(LN3D, M=5, C=1540), lambda d, t, r: "row 8" if d == F32 else "row T 8"),
    ("gpu_T_6x2048", dict(LN3D, M=6, C=2048), lambda d, t, r: "row 8" if d == F32 else "row T 8"),
    ("gpu_T_8229x352", dict(LN3D, M=8192 + 37, C=352), lambda d, t, r: "row 2" if d == F32 else "rows16 6" if r else "row T 2"),
    ("gpu_T_5000x64", dict(LN3D, M=5000, C=64), lambda d, t, r: "row 2" if d == F32 else "rows16 6" if r else "row T 2"),
]

# what keeps a residual launch on the row form whatever the knob says
KEY = dict(kind=RES, M=3 * 8, C=352, x=1, gamma=1, beta=1, delta_T=1, add=1, add_mod=8, out_T=1, out_T2=1)
CASES += [
    ("row_no_positional", dict(KEY, add=0, add_mod=0, out_T2=0), "row res 2"),
    ("row_no_out_T", dict(KEY, out_T=0), "row res 2"),
    ("row_P_not_4n", dict(KEY, M=3 * 6, add_mod=6), "row res 2"),
    ("row_ragged_tracks", dict(KEY, M=3 * 8 + 4), "row res 2"),
    ("row_x_mod_not_P", dict(KEY, x_mod=4), "row res 2"),
    ("row_shared_rows_other_period", dict(KEY, x_shared=1, x_period=4, x_split=2), "row res 2"),
    ("row_shared_rows_beside_x_mod", dict(KEY, x_mod=8, x_shared=1, x_period=8, x_split=4), "row res 2"),
    ("row_out_sum", dict(KEY, out_sum=1), "row res 2"),
    ("row_partials", dict(KEY, delta_T=0, part=1, nsplit=3), "row part 2"),
    ("chain_row_P_not_4n", dict(KEY, kind=CHAIN, M=3 * 6, add_mod=6, x_mod=6, dprev_T=1, stats_in=1, g0=1, b0=1), "row chain"),
]

# ---- refusals: (name, fields, text) for every dtype and knob value ----
T_PLAIN = "layernorm: C={C} must be a multiple of 4 and <= 2048 (and out_T2 needs add/add_mod)"
T_ROWS_T = "layernorm_T: C={C} must be a multiple of 4 and <= 2048"
T_RES = "layernorm_res: C={C} must be a multiple of 4 and <= 1536, delta or partials must be given (and out_T2 needs add/add_mod)"
T_NSPLIT = "layernorm_res: 1 <= nsplit <= 16 slices of float partials"
T_SHARED = "layernorm_res: shared rows need 0 <= x_split <= x_period, x_period > 0"
T_CHAIN = "layernorm_chain: C={C} must be a multiple of 4 and <= 1536; shared rows, both updates and the statistics are required"
RESD = dict(kind=RES, M=24, C=352, x=1, gamma=1, beta=1, delta_T=1, out_T=1)
CHAIND = dict(kind=CHAIN, M=24, C=352, x=1, x_mod=8, gamma=1, beta=1, delta_T=1, dprev_T=1, stats_in=1, g0=1, b0=1, out_T=1)
REFUSALS = [
    ("plain_C_354", dict(PLAIN, M=8, C=354), T_PLAIN),
    ("plain_C_2052", dict(PLAIN, M=8, C=2052), T_PLAIN),
    ("plain_T2_without_add", dict(PLAIN, M=8, C=352, out_T2=1), T_PLAIN),
    ("plain_T2_add_mod_0", dict(PLAIN, M=8, C=352, out_T2=1, add=1), T_PLAIN),
    ("rows_T_C_354", dict(LN3D, M=8, C=354), lambda d: T_PLAIN if d == F32 else T_ROWS_T),
    ("rows_T_C_2052", dict(LN3D, M=8, C=2052), lambda d: T_PLAIN if d == F32 else T_ROWS_T),
    ("res_C_354", dict(RESD, C=354), T_RES),
    ("res_C_1540", dict(RESD, C=1540), T_RES),
    ("res_no_addend", dict(RESD, delta_T=0), T_RES),
    ("res_T2_without_add", dict(RESD, out_T2=1), T_RES),
    ("res_nsplit_0", dict(RESD, delta_T=0, part=1, nsplit=0), T_NSPLIT),
    ("res_nsplit_17", dict(RESD, delta_T=0, part=1, nsplit=17), T_NSPLIT),
    ("res_x_period_0", dict(RESD, x_shared=1, x_period=0, x_split=0), T_SHARED),
    ("res_x_split_negative", dict(RESD, x_shared=1, x_period=8, x_split=-1), T_SHARED),
    ("res_x_split_past_period", dict(RESD, x_shared=1, x_period=8, x_split=9), T_SHARED),
    ("chain_C_354", dict(CHAIND, C=354), T_CHAIN),
    ("chain_C_1540", dict(CHAIND, C=1540), T_CHAIN),
    ("chain_x_mod_0", dict(CHAIND, x_mod=0), T_CHAIN),
    ("chain_no_rows", dict(CHAIND, x=0), T_CHAIN),
    ("chain_no_previous_update", dict(CHAIND, dprev_T=0), T_CHAIN),
    ("chain_no_statistics", dict(CHAIND, stats_in=0), T_CHAIN),
    ("chain_no_update", dict(CHAIND, delta_T=0), T_CHAIN),
    ("chain_T2_without_add", dict(CHAIND, out_T2=1), T_CHAIN),
]
SETTINGS = [(d, t, r) for d in DTYPES for t in (0, 1) for r in (0, 1)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ln_select") / "ln_select_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "ln_select_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return exe


def answers(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def test_every_launch_of_the_engine_reaches_its_form(program):
    """every case, three dtypes x ln_tracks 0 / 1 x ln_rows16 0 / 1"""
    ids, lines, want = [], [], []
    for name, fields, expect in CASES:
        for d, t, r in SETTINGS:
            ids.append(f"{name} dtype={d} ln_tracks={t} ln_rows16={r}")
            lines.append(query(d, t, r, **fields))
            want.append(expect(d, t, r) if callable(expect) else expect)
    got = answers(program, lines)
    wrong = [(i, g, w) for i, g, w in zip(ids, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(got)} launches reach another form: {wrong[:8]}"


def test_the_cases_reach_every_form(program):
    got = set(answers(program, [query(d, t, r, **fields) for _, fields, _ in CASES for d, t, r in SETTINGS]))
    for form in ("row 2", "row 6", "row 8", "row T 2", "row T 6", "row T 8", "row res 2", "row res 6", "row part 2", "row part 6", "row chain",
                 "token shared", "token own", "token chain", "rows16 6", "rows16 8"):
        assert form in got, form


@pytest.mark.parametrize("name,fields,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_messages(program, name, fields, text):
    got = answers(program, [query(d, t, r, **fields) for d, t, r in SETTINGS])
    want = ["invalid: " + (text(d) if callable(text) else text).format(C=fields["C"]) for d, _, _ in SETTINGS]
    assert got == want


def test_default_knobs_match_the_library_table():
    """KNOB_DEFAULTS above against csrc/prof.hip's table, read as text"""
    table = dict(re.findall(r'\{"(\w+)", "L4P_\w+", (-?\d+)\}', open(os.path.join(ROOT, "l4p_amd", "csrc", "prof.hip")).read()))
    for name, value in KNOB_DEFAULTS.items():
        assert int(table[name]) == value, name
