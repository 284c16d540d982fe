"""The closed-form similarity of csrc/umeyama_moments.hpp (umeyama_from_moments: the double model of l4p_metric_cameras, the float
model of l4p_similarity_ransac) on the host, no GPU: tests/umeyama_moments_main.cpp compiles the header with a plain C++ compiler and
this file compares both models with the float64 SVD reference (tests/metrics_restate.py:umeyama) on friendly and on degenerate
clouds: rotations up to pi, scales 1e-3 .. 1e3, far-off centres, mirrored, planar, collinear (along an axis: cov with two exact
zero rows / columns), static, equal singular values, and a conditioning sweep.

The rotation is not unique once cov loses rank, so what is compared is what stays unique:
  * every case: the 13 values are finite; s within 1e-9; R R^T = I and det R = +1 within 1e-9 (1e-6 for the float model, whose
    entries are rounded to 2^-24); R v1 = u1 when sigma1 stands clear of sigma2 (sigma2 <= sigma1 / 2: the SVD's own v1 is
    only defined up to the gap); R v2 = u2 when the rank is 2 or more in the sense that v2 is defined, i.e. sigma2 / sigma1 >= 1e-3
    (below it v2 is what the route through cov^T cov loses first, and the residual bounds below are what is asserted) with
    sigma2 <= sigma1 / 2 and sigma3 <= sigma2 / 2; R = I within 1e-9 when src and dst lie on one line in the same sense (the
    completion of the free rotation, pinned in include/l4p_hip.h), along each axis and obliquely, also with dst rounded off the line;
  * sigma2 / sigma1 >= 1e-3: s, the entries of R and t and the RMS residual within 1e-9 (double model; the route through
    cov^T cov squares the condition number: predicted eps (sigma1 / sigma2)^2 <= 2.2e-10) and 1e-6 (float model).  "Relative" is
    to 1 for the entries of R, to the terms t = md - s R ms is formed from for t, to the extent of dst for the residual (and to
    the residual itself where it is not rounding noise);
  * sigma2 / sigma1 < 1e-3, rank 1 exactly (collinear, static): the residual does not depend on the free rotation about the line, so
    the 1e-9 bound holds as it stands;
  * sigma2 / sigma1 < 1e-3 with sigma2 > 0 (a line plus isotropic jitter j; an exact similarity of it has sigma2 / sigma1 ~ 10 j^2,
    a noisy one ~ j / 3): the rotation about the line is lost as eps / (sigma2 / sigma1)^2 grows to 1 and stays lost below that,
    and the RMS residual exceeds the SVD's by that angle times the jitter when the fit is exact (by its square otherwise).
    MEASURED with this harness against the float64 SVD over j in {1e-2, 1e-4, 1e-6, 1e-8} x 3 seeds x {axis, oblique line} x
    {exact, noisy dst}: the worst excess over the SVD's RMS residual, relative to the extent of dst, per decade of sigma2 / sigma1
    (the decades the sweep reaches), asserted at four times that and at no less than 1e-12, the rounding of the residual's own
    evaluation (EXCESS_BOUND):
        [1e-4, 1e-3): 7.3e-14    [1e-6, 1e-5): 2.3e-17    [1e-7, 1e-6): 4.4e-8     [1e-8, 1e-7): 4.0e-7     [1e-9, 1e-8): 1.5e-9
        [1e-10, 1e-9): 6.0e-10   [1e-11, 1e-10): 4.5e-8   [1e-12, 1e-11): 2.4e-7   [1e-15, 1e-14): 2.6e-8   [1e-16, 1e-15): 3.2e-9
    (The plane-plus-jitter sweep has sigma2 / sigma1 ~ 0.5 at every j and meets the 1e-9 bounds.)

The parent of the rank-deficient fix fails the axis-aligned and the exactly collinear cases here: its R = u1 v1^T has det 0.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import metrics_restate as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

TOL = {"f64": 1e-9, "f32": 1e-6}
RATIO_MIN = 1e-3  # sigma2 / sigma1 from which on R is compared entry by entry
# floor(log10(sigma2 / sigma1)) -> four times the measured worst excess of the RMS residual over the SVD's, relative to the extent
# of dst (docstring)
EXCESS_FLOOR = 1e-12
EXCESS_BOUND = {-4: 4 * 7.3e-14, -6: 4 * 2.3e-17, -7: 4 * 4.4e-8, -8: 4 * 4.0e-7, -9: 4 * 1.5e-9, -10: 4 * 6.0e-10, -11: 4 * 4.5e-8,
                -12: 4 * 2.4e-7, -15: 4 * 2.6e-8, -16: 4 * 3.2e-9}
SWEEP_J = (1e-2, 1e-4, 1e-6, 1e-8)
SKEW = [0.3, -1.0, 0.45]
AXES = {"x": [1.0, 0.0, 0.0], "y": [0.0, 1.0, 0.0], "z": [0.0, 0.0, 1.0], "oblique": [1.0, 2.0, 3.0]}
T0 = np.array([0.5, -1.0, 2.0])


def _cloud(rng, n=40):
    return rng.standard_normal((n, 3)) * np.array([1.0, 0.7, 0.4])


def _sim(src, s, R, t, rng=None, noise=0.0):
    dst = s * src @ R.T + t
    if noise:
        dst = dst + noise * float(np.ptp(dst, axis=0).max()) * rng.standard_normal(dst.shape)
    return dst


def _line(rng, axis, n=24):
    """n points exactly on a line through a dyadic offset: along a coordinate axis the other two coordinates are constants"""
    d = np.asarray(AXES[axis]) / np.linalg.norm(AXES[axis])
    return np.round(rng.uniform(-2, 2, (n, 1)) * 1024) / 1024 * d + np.array([0.25, -0.5, 1.5])


def make_cases():
    c = {}
    k = 0

    def rng():
        nonlocal k
        k += 1
        return np.random.default_rng(4000 + k)

    Rs = MR.rot(SKEW, 0.9)
    for name, R in (("0", np.eye(3)), ("1e-8", MR.rot(SKEW, 1e-8)), ("half_pi", MR.rot([0, 0, 1], np.pi / 2)),
                    ("pi", np.diag([-1.0, -1.0, 1.0])), ("pi_skew", MR.rot(SKEW, np.pi)), ("2.9_skew", MR.rot(SKEW, 2.9))):
        for noise in (0.0, 1e-2):
            g = rng()
            src = _cloud(g)
            c[f"angle_{name}_noise{noise:g}"] = (src, _sim(src, 1.7, R, T0, g, noise))
    for s in (1e-3, 1.0, 1e3):
        g = rng()
        src = _cloud(g)
        c[f"scale_{s:g}"] = (src, _sim(src, s, Rs, T0, g, 1e-2))
    g = rng()
    src = _cloud(g)
    src = src + 1e3 * float(np.ptp(src, axis=0).max()) * np.array([1.0, -0.6, 0.8])  # 1e3 extents from the origin
    c["far_src_and_dst"] = (src, _sim(src, 1.7, Rs, T0, g, 1e-2))
    c["far_src_near_dst"] = (src, _sim(src - src.mean(0), 1.7, Rs, T0, g, 1e-2))
    for noise in (0.0, 1e-2):
        g = rng()
        src = _cloud(g)
        c[f"mirrored_noise{noise:g}"] = (src * np.array([1.0, 1.0, -1.0]), _sim(src, 1.7, Rs, T0, g, noise))
    # planar: z = 0 exactly
    g = rng()
    flat = _cloud(g) * np.array([1.0, 1.0, 0.0])
    c["planar_src"] = (flat, _sim(flat, 1.7, Rs, T0, g, 1e-2))
    c["planar_dst"] = (_sim(flat, 0.6, Rs, T0, g, 1e-2), flat)
    c["planar_both_exact"] = (flat, _sim(flat, 2.0, np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), T0))
    c["planar_both_oblique"] = (flat, _sim(flat, 1.7, Rs, T0))
    c["planar_mirrored"] = (flat * np.array([1.0, -1.0, 1.0]), _sim(flat, 1.7, Rs, T0, g, 1e-2) * np.array([1.0, 1.0, 0.0]))
    g = rng()
    tri = _cloud(g, 3)
    c["n3_exact"] = (tri, _sim(tri, 1.7, Rs, T0))
    c["n3_noisy"] = (tri, _sim(tri, 1.7, Rs, T0, g, 1e-2))
    # collinear: the other side is a noisy 3-D cloud (a noisy estimate of a dolly shot, or the reverse)
    for axis in AXES:
        g = rng()
        line = _line(g, axis)
        c[f"collinear_src_{axis}"] = (line, _sim(line, 1.7, Rs, T0, g, 5e-2))
        c[f"collinear_dst_{axis}"] = (_sim(line, 0.6, Rs, T0, g, 5e-2), line)
        other = "y" if axis == "x" else "x"
        b = (line - line[0]) @ np.asarray(AXES[axis]) / np.linalg.norm(AXES[axis])
        c[f"collinear_both_{axis}"] = (line, 2.0 * b[:, None] * np.asarray(AXES[other]) + T0)
        c[f"collinear_both_same_{axis}"] = (line, 2.0 * (line - line[0]) + T0)
        # a small dst on the same line: its coordinates round off the line by ~1e3 eps of its extent, u1 is v1 only that closely
        c[f"collinear_both_same_small_{axis}"] = (line, 1e-3 * (line - line[0]) + T0)
    # static: dyadic values, so the means are exact and the centred coordinates exactly zero
    g = rng()
    src = _cloud(g, 16)
    still = np.tile(np.array([1.5, -2.25, 0.75]), (16, 1))
    c["static_src"] = (still, src)
    c["static_dst"] = (src, still)
    c["static_both"] = (still, still[:, ::-1].copy())
    # equal singular values
    for name, (a, b) in (("two_equal", (1.0, 0.5)), ("two_equal_small_first", (0.5, 1.0)), ("three_equal", (1.0, 1.0))):
        octa = np.array([[a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, b], [0, 0, -b]], np.float64)
        c[f"octahedron_{name}_identity"] = (octa, _sim(octa, 2.0, np.eye(3), T0))
        c[f"octahedron_{name}_skew"] = (octa, _sim(octa, 1.7, Rs, T0))
        if a > b:  # (with sigma2 = sigma3 the reflection may fall on either: R is not unique)
            c[f"octahedron_{name}_mirrored"] = (octa * np.array([1.0, 1.0, -1.0]), _sim(octa, 1.7, Rs, T0))
    # conditioning sweeps
    for j in SWEEP_J:
        for seed in range(3):
            for axis in ("x", "oblique"):
                g = np.random.default_rng(7000 + seed)
                line = _line(g, axis)
                src = line + j * float(np.ptp(line, axis=0).max()) * g.standard_normal(line.shape)
                c[f"sweep_line_{axis}_j{j:g}_seed{seed}_exact"] = (src, _sim(src, 1.7, Rs, T0))
                c[f"sweep_line_{axis}_j{j:g}_seed{seed}_noisy"] = (src, _sim(src, 1.7, Rs, T0, g, 1e-2))
            g = np.random.default_rng(7100 + seed)
            flat = _cloud(g) * np.array([1.0, 1.0, 0.0])
            src = flat + j * float(np.ptp(flat, axis=0).max()) * g.standard_normal(flat.shape) * np.array([0.0, 0.0, 1.0])
            c[f"sweep_plane_j{j:g}_seed{seed}_exact"] = (src, _sim(src, 1.7, Rs, T0))
            c[f"sweep_plane_j{j:g}_seed{seed}_noisy"] = (src, _sim(src, 1.7, Rs, T0, g, 1e-2))
    return c


CASES = make_cases()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("umeyama_moments") / "umeyama_moments_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "l4p_amd", "csrc"),
           os.path.join(ROOT, "tests", "umeyama_moments_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    text = []
    for src, dst in CASES.values():
        text.append(str(len(src)))
        text += [" ".join(repr(float(x)) for x in np.concatenate([a, b])) for a, b in zip(src, dst)]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [np.array(line.split(), np.float64) for line in out.stdout.splitlines()]
    assert len(rows) == 2 * len(CASES) and all(r.size == 13 for r in rows)
    return {name: {"f64": rows[2 * i], "f32": rows[2 * i + 1]} for i, name in enumerate(CASES)}


def reference(name):
    src, dst = CASES[name]
    s, R, t, cov = MR.umeyama(src, dst)
    U, D, Vt = np.linalg.svd(cov)
    extent = float(np.ptp(dst, axis=0).max()) or 1.0
    return {"s": s, "R": R, "t": t, "U": U, "D": D, "Vt": Vt, "extent": extent, "ratio": D[1] / D[0] if D[0] > 0 else 0.0,
            "rms": rms(src, dst, s * R, t), "var": float(((src - src.mean(0)) ** 2).sum() / len(src))}


def rms(src, dst, sR, t):
    return float(np.sqrt(((src @ sR.T + t - dst) ** 2).sum() / len(src)))


def excess(name, model):
    """the RMS residual of a model over the reference's, relative to the extent of dst"""
    src, dst = CASES[name]
    ref = reference(name)
    return (rms(src, dst, model[:9].reshape(3, 3), model[9:12]) - ref["rms"]) / ref["extent"]


@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_svd(models, name, kind):
    src, dst = CASES[name]
    ref, m, tol = reference(name), models[name][kind], TOL[kind]
    assert np.isfinite(m).all(), m
    s, B, t = float(m[12]), m[:9].reshape(3, 3), m[9:12]
    print(f"{name} {kind}: sigma {ref['D']} ratio {ref['ratio']:.3e} s {s!r} ref {ref['s']!r} excess {excess(name, m):.3e}")
    assert abs(s - ref["s"]) <= tol * abs(ref["s"]), (s, ref["s"])
    if ref["var"] == 0:  # static src: s = 1, R = I, t = md - ms
        assert s == 1.0 and np.array_equal(B, np.eye(3)) and np.abs(t - ref["t"]).max() <= tol * np.abs(dst).max()
        return
    if ref["D"][0] == 0:  # cov = 0 under a moving src: s = 0, so s R = 0 and t = md
        assert s == 0.0 and not B.any() and np.abs(t - dst.mean(0)).max() <= tol * np.abs(dst).max()
        return
    R = B / s
    assert np.abs(R @ R.T - np.eye(3)).max() <= tol, R @ R.T
    assert abs(np.linalg.det(R) - 1.0) <= tol, np.linalg.det(R)
    D, U, Vt = ref["D"], ref["U"], ref["Vt"]
    if name.startswith("collinear_both_same"):
        assert np.abs(R - np.eye(3)).max() <= tol, R
    if D[1] <= 0.5 * D[0]:  # (the singular vector's own condition is sigma1^2 / (sigma1^2 - sigma2^2) <= 4 / 3)
        assert np.abs(R @ Vt[0] - U[:, 0]).max() <= tol, (R @ Vt[0], U[:, 0])
    if ref["ratio"] >= RATIO_MIN and D[1] <= 0.5 * D[0] and D[2] <= 0.5 * D[1]:
        assert np.abs(R @ Vt[1] - U[:, 1]).max() <= tol, (R @ Vt[1], U[:, 1])
    # the residual: relative to the extent of dst for the double model; the float model's entries are rounded relative to the
    # terms of s R src + t - dst, which are larger than the extent when the clouds lie far from the origin
    terms = max(float(np.abs(dst).max()), float(np.abs(ref["t"]).max()), ref["s"] * float(np.abs(src).max()))
    unit = ref["extent"] if kind == "f64" else max(ref["extent"], terms)
    ex = excess(name, m) * ref["extent"]
    if ref["ratio"] >= RATIO_MIN or not name.startswith("sweep_line"):
        assert abs(ex) <= tol * unit, (ex / unit, ref["ratio"])
        if kind == "f64" and ref["rms"] > 1e-6 * unit:  # a residual that is not rounding noise: relative to itself as well
            assert abs(ex) <= tol * ref["rms"], (ex / ref["rms"], ref["ratio"])
    else:
        bound = max(EXCESS_BOUND[int(np.floor(np.log10(ref["ratio"])))], EXCESS_FLOOR)
        assert abs(ex) <= bound * ref["extent"] + (tol * unit if kind == "f32" else 0.0), (ex / ref["extent"], ref["ratio"])
    if ref["ratio"] >= RATIO_MIN:
        assert np.abs(R - ref["R"]).max() <= tol, (np.abs(R - ref["R"]).max(), ref["ratio"])
        t_terms = max(float(np.abs(dst.mean(0)).max()), ref["s"] * float(np.abs(src.mean(0)).max()), float(np.abs(ref["t"]).max()))
        assert np.abs(t - ref["t"]).max() <= tol * t_terms, (np.abs(t - ref["t"]).max() / t_terms, ref["ratio"])


def test_the_cases_reach_the_regimes_they_are_about():
    ratio = {name: reference(name)["ratio"] for name in CASES}
    rank = {name: int((reference(name)["D"] > 1e-12 * max(reference(name)["D"][0], 1e-300)).sum()) for name in CASES}
    for name in CASES:
        if name.startswith("collinear"):
            assert rank[name] == 1, (name, reference(name)["D"])
        if name.startswith(("planar", "n3")):
            assert rank[name] == 2, (name, reference(name)["D"])
        if name.startswith("sweep_plane"):
            assert ratio[name] >= RATIO_MIN, (name, ratio[name])
        for j in SWEEP_J:
            if name.startswith("sweep_line") and f"_j{j:g}_" in name:  # exact: the product of the two jitters; noisy: one of them
                assert (5 * j * j < ratio[name] < 30 * j * j) if name.endswith("exact") else (0.002 * j < ratio[name] < j), (name, ratio[name])
    below = {int(np.floor(np.log10(r))) for name, r in ratio.items() if name.startswith("sweep_line") and r < RATIO_MIN}
    assert below == set(EXCESS_BOUND), below
    for axis in "xyz":  # along a coordinate axis the covariance has two rows / columns of exact zeros
        k = "xyz".index(axis)
        assert not np.delete(MR.umeyama(*CASES[f"collinear_dst_{axis}"])[3], k, axis=0).any()
        assert not np.delete(MR.umeyama(*CASES[f"collinear_src_{axis}"])[3], k, axis=1).any()
    for name in ("mirrored_noise0", "mirrored_noise0.01", "octahedron_two_equal_mirrored"):
        assert np.linalg.det(MR.umeyama(*CASES[name])[3]) < 0
    assert not MR.umeyama(*CASES["static_dst"])[3].any() and not MR.umeyama(*CASES["static_src"])[3].any()
    d = reference("octahedron_two_equal_identity")["D"]
    assert d[0] == d[1] > d[2] > 0
    d = reference("octahedron_three_equal_identity")["D"]
    assert d[0] == d[1] == d[2] > 0


def test_reference_contracts():
    """the restatement itself: a proper rotation at every rank, and the pinned degenerate values instead of NaN"""
    for name, (src, dst) in CASES.items():
        s, R, t, _ = MR.umeyama(src, dst)
        assert np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all(), name
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12, name
    s, R, t, _ = MR.umeyama(*CASES["static_src"])
    assert s == 1.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, CASES["static_src"][1].mean(0) - CASES["static_src"][0][0])
    s, R, t, _ = MR.umeyama(*CASES["static_dst"])
    assert s == 0.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, CASES["static_dst"][1][0])
