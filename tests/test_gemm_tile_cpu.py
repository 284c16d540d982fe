"""The addressing helpers the GEMM / implicit-conv kernels share (csrc/gemm_tile.hpp) on the host: workgroup -> tile orders, the
row-group map of A, the conv's voxel decode, tap masks and tap offsets, the sub-pixel conv's cell walk and the split-K k-range,
checked without a GPU.  The GPU tests see these only through whole kernels at a handful of shapes.

tests/gemm_tile_main.cpp includes gemm_tile.hpp alone (plain C++17, no HIP) and answers one query per input line with a line of
integers.  The expected values are brute force written out here - loops over tiles, voxels and taps - not the header's formulas.  All
queries go through one process; the same driver is built and run once more under the address and undefined-behaviour sanitizers.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)


def build(exe, extra):
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "l4p_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_tile_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    return build(str(tmp_path_factory.mktemp("gemm_tile") / "gemm_tile_main"), [])


def answers(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [[int(v) for v in row.split()] for row in out.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


# ---- xcd_tile ----
def test_xcd_tile_gives_every_xcd_a_contiguous_range(program):
    sizes = range(1, 301)
    for ntiles, tiles in zip(sizes, answers(program, [f"xcd ntiles={n}" for n in sizes])):
        assert sorted(tiles) == list(range(ntiles)), ntiles  # a bijection of [0, ntiles)
        ranges = [[tiles[bid] for bid in range(x, ntiles, 8)] for x in range(8)]  # XCD x runs workgroups x, x + 8, ... in that order
        for r in ranges:
            assert r == list(range(r[0], r[0] + len(r))) if r else True, (ntiles, r)
        assert max(map(len, ranges)) - min(map(len, ranges)) <= 1, ntiles
        firsts = [r[0] for r in ranges if r]
        assert firsts == sorted(firsts), ntiles  # the ranges follow each other in XCD order


# ---- banded_tile ----
def banded_order(ntm, ntn):
    """the banded walk by construction: the fewest bands of <= 8 columns, evenly wide, the last one takes the rest"""
    nb = -(-ntn // 8)
    bw = -(-ntn // nb)
    bands = [range(k * bw, min((k + 1) * bw, ntn)) for k in range(nb)]
    assert all(0 < len(b) <= 8 for b in bands) and sum(map(len, bands)) == ntn
    return [(mt, nt) for band in bands for mt in range(ntm) for nt in band]


def test_banded_tile_walks_bands_of_at_most_eight_columns(program):
    shapes = [(ntm, ntn) for ntm in range(1, 13) for ntn in range(1, 41)]
    for (ntm, ntn), flat in zip(shapes, answers(program, [f"banded ntm={m} ntn={n}" for m, n in shapes])):
        got = list(zip(flat[0::2], flat[1::2]))
        assert sorted(got) == sorted(itertools.product(range(ntm), range(ntn))), (ntm, ntn)  # a bijection onto ntm x ntn
        assert got == banded_order(ntm, ntn), (ntm, ntn)
        if ntn <= 8:
            assert got == list(itertools.product(range(ntm), range(ntn))), (ntm, ntn)  # one band: row-major


# ---- gemm_a_row ----
def test_gemm_a_row_maps_row_groups(program):
    gs, go, n = 1000, 37, 300
    groups = (0, 1, 7, 128)
    for gr, got in zip(groups, answers(program, [f"arow a_gr={gr} a_gs={gs} a_go={go} n={n}" for gr in groups])):
        want = [m if gr == 0 else (m // gr) * gs + go + m % gr for m in range(n)]
        assert got == want, gr


# ---- conv_voxel, conv_voxel_index, conv_tap_mask, conv_tap_offset ----
@pytest.mark.parametrize("strides", [(1, 1, 1), (1, 2, 2)])
def test_conv_voxels_masks_and_offsets_against_a_triple_loop(program, strides):
    B, Ti, Hi, Wi, Cin = 2, 2, 3, 5, 64
    st, sh, sw = strides
    To, Ho, Wo = (Ti - 1) // st + 1, (Hi - 1) // sh + 1, (Wi - 1) // sw + 1
    (got,) = answers(program, [f"conv B={B} Ti={Ti} Hi={Hi} Wi={Wi} st={st} sh={sh} sw={sw} Cin={Cin}"])
    taps = list(itertools.product((-1, 0, 1), repeat=3))  # (dt, dh, dw), tap = (dt + 1) * 9 + (dh + 1) * 3 + dw + 1
    assert got[:27] == [((dt * Hi + dh) * Wi + dw) * Cin for dt, dh, dw in taps]
    want = []
    for b in range(B):
        for to in range(To):
            for ho in range(Ho):
                for wo in range(Wo):
                    ti, hi, wi = to * st, ho * sh, wo * sw
                    mask = sum(1 << tap for tap, (dt, dh, dw) in enumerate(taps)
                               if 0 <= ti + dt < Ti and 0 <= hi + dh < Hi and 0 <= wi + dw < Wi)
                    want += [b, ti, hi, wi, ((b * Ti + ti) * Hi + hi) * Wi + wi, mask]
    assert got[27:] == want
    # every tap the mask admits addresses a voxel of the same batch item's volume
    for m in range(B * To * Ho * Wo):
        b, ti, hi, wi, index, mask = want[6 * m:6 * m + 6]
        for tap in range(27):
            if mask >> tap & 1:
                assert b * Ti * Hi * Wi * Cin <= index * Cin + got[tap] < (b + 1) * Ti * Hi * Wi * Cin


# ---- subpix_cells, subpix_tap: the cell walk the stream counters of the sub-pixel conv step through ----
def subpix_cells_by_hand(k, s):
    """along one axis: the taps d = -1, 0, 1 of up-scaled position k i + s reach the low-resolution cells (k i + s + d) // k - i, as tap
    coordinates 0 .. 2"""
    return sorted({(k * 1 + s + d) // k - 1 + 1 for d in (-1, 0, 1)})


@pytest.mark.parametrize("k", [(2, 2, 2), (1, 2, 2), (1, 1, 1), (1, 3, 3)])
def test_subpix_cell_walk_for_every_sub_position(program, k):
    Cout = 64
    subs = list(itertools.product(*(range(x) for x in k)))
    lines = [f"cells Cout={Cout} kt_={k[0]} kh={k[1]} kw={k[2]} n0={((s[0] * k[1] + s[1]) * k[2] + s[2]) * Cout} n=30" for s in subs]
    for s, got in zip(subs, answers(program, lines)):
        ct, ch, cw = (subpix_cells_by_hand(kk, ss) for kk, ss in zip(k, s))
        taps = [(a * 3 + b) * 3 + c for a in ct for b in ch for c in cw]  # ascending (c_t, c_h, c_w)
        assert got[:6] == [ct[0], ch[0], cw[0], len(ch), len(cw), len(taps)], (k, s)
        assert got[6:] == [taps[min(j, len(taps) - 1)] for j in range(30)], (k, s)  # past the last cell: the last one again


# ---- splitk_begin ----
def test_splitk_slices_tile_the_k_range(program):
    shapes = [(nk, ns) for nk in range(1, 101) for ns in range(1, 17)]
    for (nk, ns), begins in zip(shapes, answers(program, [f"splitk nk={nk} nsplit={ns}" for nk, ns in shapes])):
        assert begins[0] == 0 and begins[-1] == nk and len(begins) == ns + 1, (nk, ns)
        assert all(a <= b for a, b in zip(begins, begins[1:])), (nk, ns)  # slice s = [begins[s], begins[s + 1]): they tile [0, nk)
        assert max(b - a for a, b in zip(begins, begins[1:])) - min(b - a for a, b in zip(begins, begins[1:])) <= 1, (nk, ns)


# ---- the same driver under the host sanitizers ----
def test_driver_under_the_host_sanitizers(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    # (the sanitizer runtimes linked statically - clang's default, a flag for gcc - as tests/test_graph_stack_cpu.py does)
    static = [] if "clang" in os.path.basename(os.path.realpath(CXX)) else ["-static-libasan", "-static-libubsan"]
    exe = build(str(tmp_path / "gemm_tile_main_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static])
    lines = [f"xcd ntiles={n}" for n in (1, 7, 8, 9, 300)] + [f"banded ntm={m} ntn={n}" for m, n in ((1, 1), (3, 8), (3, 9), (12, 40))]
    lines += [f"arow a_gr={g} a_gs=1000 a_go=37 n=300" for g in (0, 1, 7, 128)]
    lines += ["conv B=2 Ti=2 Hi=3 Wi=5 st=1 sh=1 sw=1 Cin=64", "conv B=2 Ti=2 Hi=3 Wi=5 st=1 sh=2 sw=2 Cin=64"]
    lines += ["cells Cout=64 kt_=2 kh=2 kw=2 n0=448 n=30", "cells Cout=64 kt_=1 kh=3 kw=3 n0=256 n=30"]
    lines += [f"splitk nk={nk} nsplit={ns}" for nk, ns in ((1, 16), (100, 7))]
    assert all(answers(exe, lines))
