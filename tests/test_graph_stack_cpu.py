"""The workspace allocator of the native graphs (csrc/graph.hpp Stack: 256-byte steps, release by mark, high-water mark, dry-run
size query, refusal of a workspace that is too small), checked without a GPU: tests/graph_stack_main.cpp compiles the struct alone
(L4P_GRAPH_STACK_ONLY: no HIP header) with the address and undefined-behaviour sanitizers and writes every block it is given."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)


def test_stack_allocator_under_the_host_sanitizers(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "graph_stack_main")
    # (the sanitizer runtimes linked statically - clang's default, a flag for gcc: a shared one refuses to start in an environment
    #  that preloads any other library in front of it)
    static = [] if "clang" in os.path.basename(os.path.realpath(CXX)) else ["-static-libasan", "-static-libubsan"]
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "graph_stack_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr[-2000:])
    assert int(out.stdout.split()[1]) > 100
