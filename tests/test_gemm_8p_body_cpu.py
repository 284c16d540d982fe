"""The main-loop body of the dense 8-phase GEMM launches, decided on the host (csrc/gemm_select.hpp: GemmKnobs.gemm_8p_body and the
predicate gemm_8p_two_phase), checked without a GPU through tests/gemm_8p_body_main.cpp:

  * gemm_8p_body = 0 keeps the enumerators and tags the launcher had before the knob existed, and the predicate picks the body: two
    phases per k-tile from 8 whole k-tiles on (K >= 512), four below (the mask product's K = 352 measured slower on the two-phase body);
  * 1 / 2 force a body, on new enumerators behind every older one, tagged "8p 2ph" / "8p 4ph";
  * the knob's default in csrc/prof.hip's table is 0.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

# (M, N, K, epi, gemm_t192): the c3 step's six 8-phase linear shapes, a K = 256 1x1 conv and the smallest forced shapes of the GPU test
SHAPES = {"fc1": (8192, 6144, 1408, 0, 1, "t256x256"), "fc2": (8192, 1408, 6144, 0, 1, "t256x192"), "qkv": (8192, 4608, 1408, 1, 1, "t256x192"),
          "maskdot": (1048576, 768, 352, 3, 1, "t256x256"), "up0": (131072, 2816, 1408, 2, 1, "t256x256"), "proj": (8192, 1408, 1408, 0, 1, "t256x192"),
          "k256": (262144, 256, 256, 0, 1, "t256x256"), "k512": (300, 264, 512, 0, 0, "t256x256"), "k504": (300, 264, 504, 0, 0, "t256x256"),
          "k64_t192": (300, 384, 64, 0, 1, "t256x192")}
TWO_PHASE_BY_DEFAULT = {"fc1", "fc2", "qkv", "up0", "proj", "k512"}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_8p_body") / "gemm_8p_body_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_8p_body_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    keys = [(name, body) for name in SHAPES for body in (0, 1, 2)]
    lines = ["%d %d %d %d %d %d" % (SHAPES[name][:5] + (body,)) for name, body in keys]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(keys)
    res = {}
    for key, line in zip(keys, got):
        form, rest = line.split(" ", 1)
        tag, two = rest.rsplit(" ", 1)
        res[key] = (int(form), tag, int(two))
    return res


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_default_keeps_the_tag_and_the_rule_picks_the_body(answers, name):
    tile = SHAPES[name][5]
    form, tag, two = answers[(name, 0)]
    assert tag == f"8p {tile}"
    assert two == int(name in TWO_PHASE_BY_DEFAULT)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_forced_bodies_have_their_own_tags_and_later_enumerators(answers, name):
    tile = SHAPES[name][5]
    default = answers[(name, 0)][0]
    for body, word, two in ((1, "2ph", 1), (2, "4ph", 0)):
        form, tag, got_two = answers[(name, body)]
        assert tag == f"8p {word} {tile}" and got_two == two
        assert form > max(a[0] for (n, b), a in answers.items() if b == 0), "a forced enumerator in front of an older one"
        assert form != default
    assert len({answers[(name, b)][0] for b in (0, 1, 2)}) == 3


def test_knob_default_is_the_launchers_choice():
    table = dict(re.findall(r'\{"(\w+)", "L4P_\w+", (-?\d+)\}', open(os.path.join(ROOT, "l4p_amd", "csrc", "prof.hip")).read()))
    assert int(table["gemm_8p_body"]) == 0
