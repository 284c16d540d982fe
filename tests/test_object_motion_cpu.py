"""Object motion without a GPU: the numpy restatement (tests/object_motion_restate.py) against known rigid motions, the conditions
the GPU tests' clips must meet, the argument errors of l4p_amd/utils/object_motion.py, the header's new entries, and the rotation
entry of csrc/umeyama_moments.hpp compiled for the host (tests/umeyama_rotation_main.cpp) against the float64 SVD.

MEASURED here in float64 on ``rigid_scene`` (grid step q = v / 256 = 1.95e-4, 480 exact correspondences per frame, three motions of
3.4, 16.6 and 14.3 degrees): the restatement's motion against the true G_t G_(t-1)^-1 is off by at most
    2.36e-5 in an entry of R   and   5.60e-5 in an entry of t
- the quantisation of the points to steps of q at work, not the code under test (the same at n_refits = 0 and 1: every pair is an
inlier).  The tests assert at four times that (ERR_R, ERR_T), the convention of tests/test_umeyama_moments_cpu.py.  With
CORRUPT_SHARE = 10 % of the pairs redirected 12 pixels (7.2 voxels) off, measured: n_refits = 0 is off by 2.3e-2 / 5.8e-2 (outside),
n_refits = 1 by 3.2e-5 / 8.2e-5 (inside; 433, 425 and 432 of 480 pairs kept).

Fused model, measured with tests/static_map_restate.py on the restatement's canonical points of ``rigid_scene`` (voxel 0.05, pixel
spacing 0.03): 292 voxels from all four frames, 292 from frame 0 alone, 1208 with the motion replaced by the identity."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from l4p_amd import _header, _lib
from l4p_amd.utils import object_motion as OM
from tests import metrics_restate as MR
from tests import object_motion_restate as OR
from tests import static_map_restate as SMRS
from tests.test_umeyama_moments_cpu import CASES as UMEYAMA_CASES
from tests.test_umeyama_moments_cpu import RATIO_MIN, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)
ERR_R, ERR_T = 4 * 2.36e-5, 4 * 5.60e-5  # four times the measured error of the restatement on rigid_scene (docstring)
MARGIN_MIN = 1e-3  # no residual within this share of tau of tau
MODEL_CAP, SMEAR_MIN = 1.25, 2.0  # fused model: all frames <= 1.25 x frame 0 alone; with the identity for the motion >= 2 x


def _restate(c, **kw):
    return OR.restate(c["object_id"], c["K"], c["points"], c["grid"], c["flow"], **kw)


def test_restatement_recovers_the_known_motion():
    c = OR.rigid_scene()
    for n_refits in (0, 1):
        r = _restate(c, n_refits=n_refits)
        assert r["valid"][0].tolist() == [0, 1, 1, 1] and r["n_pairs"][0].tolist() == [0, 480, 480, 480]
        err_r, err_t = OR.motion_error(r["motion64"][0], c["true"])
        print(f"rigid_scene n_refits={n_refits}: R off by {err_r:.3e}, t by {err_t:.3e}; rms {r['rms'][0]}")
        assert err_r <= ERR_R and err_t <= ERR_T, (err_r, err_t)
        assert err_r >= ERR_R / 16 and err_t >= ERR_T / 16, "the measured values in the docstring are stale"
        # the poses compose to G_t, and the canonical points are the object's points of frame 0
        G = c["G"]
        for t in range(len(G)):
            assert np.abs(r["pose"][0, t, :9].reshape(3, 3) - G[t, :3, :3]).max() <= t * ERR_R + 1e-6
        on = c["object_id"].reshape(-1) == 0
        assert np.isnan(r["canonical"][~on]).all() and np.isfinite(r["canonical"][on]).all()
    angles = [np.degrees(np.arccos((np.trace(c["true"][t, :9].reshape(3, 3)) - 1) / 2)) for t in (1, 2, 3)]
    assert min(angles) > 2 and max(angles) > 10, angles  # a few degrees to tens of degrees per frame


def test_refit_rejects_corrupted_pairs():
    c = OR.rigid_scene(corrupt=OR.CORRUPT_SHARE)
    moved = int((c["flow"][0] != OR.rigid_scene()["flow"][0]).sum())
    assert 0.05 * 3 * 480 <= moved <= 0.15 * 3 * 480, moved
    r0, r1 = _restate(c, n_refits=0), _restate(c, n_refits=1)
    e0, e1 = OR.motion_error(r0["motion64"][0], c["true"]), OR.motion_error(r1["motion64"][0], c["true"])
    print(f"corrupted {moved} pairs: n_refits=0 off by {e0}, n_refits=1 by {e1}, inliers {r1['n_inliers'][0]}")
    assert e1[0] <= ERR_R and e1[1] <= ERR_T, e1
    assert e0[0] > ERR_R and e0[1] > ERR_T, e0  # the case discriminates: without the refit the bound is missed
    assert (r1["n_inliers"][0, 1:] < 480).all() and (r1["n_inliers"][0, 1:] >= 400).all()


@pytest.mark.parametrize("name", sorted(OR.gpu_cases()))
def test_gpu_cases_are_well_conditioned_and_clear_of_the_threshold(name):
    c, kw = OR.gpu_cases()[name]
    r = _restate(c, **kw)
    valid = r["valid"].astype(bool)
    print(f"{name}: {int(valid.sum())} valid rows, sigma2 / sigma1 >= {np.nanmin(r['ratio']) if valid.any() else None}, margin {r['margin']}")
    assert (r["ratio"][valid] >= RATIO_MIN).all(), r["ratio"]
    assert r["margin"] > MARGIN_MIN, r["margin"]


def test_cases_reach_what_they_are_about():
    cases = OR.gpu_cases()
    r = _restate(cases["serpentine_flow_bad_points"][0])
    assert r["valid"][0, 1:].all() and (r["n_inliers"][0, 1:] < r["n_pairs"][0, 1:]).all()
    c = cases["straddle"][0]
    lanes = np.nonzero(np.diff(c["object_id"].reshape(-1)) != 0)[0] + 1  # where a run starts
    assert len({int(v) % 64 for v in lanes}) >= 32 and any((a // 256) != ((b - 1) // 256) for a, b in zip(lanes[:-1], lanes[1:]))
    e = _restate(cases["edge"][0])
    k = OR.EDGE_OBJECTS
    assert e["n_pairs"][k["few"], 1:].tolist() == [6] * 4 and not e["valid"][k["few"]].any()
    assert np.array_equal(e["motion64"][k["few"], 1, :9], OR.EYE12[:9]) and np.abs(e["motion64"][k["few"], 1, 9:]).max() > 0.01
    assert np.allclose(e["motion64"][k["few"], 1, 9:], e["AB"][k["few"], 1, 1] - e["AB"][k["few"], 1, 0], atol=1e-12)
    assert np.array_equal(e["motion64"][k["late"], :3], np.tile(OR.EYE12, (3, 1))) and e["valid"][k["late"]].tolist() == [0, 0, 0, 1, 1]
    assert e["pose_valid"][k["late"]].all() and e["pose_valid"][k["few"]].tolist() == [1, 0, 0, 0, 0]
    assert e["n_far"][k["far"]].tolist() == [0, 2, 2, 2, 2] and e["n_inliers"][k["far"], 1:].tolist() == [23] * 4 and e["n_far"].sum() == 8
    one = _restate(cases["one_frame"][0], min_pairs=3)
    assert one["n_pairs"].sum() == 0 and np.array_equal(one["pose"], np.tile(OR.EYE12, one["pose"].shape[:2] + (1,)))


def test_fused_model_of_the_restatement_stays_under_the_cap():
    c = OR.rigid_scene()
    r = _restate(c)
    T = c["object_id"].shape[0]
    ids = c["object_id"].reshape(-1)
    keep = ids == 0
    first = keep & (np.arange(len(ids)) < len(ids) // T)
    n = {name: SMRS.restate(p, c["colors"], T, c["grid"], keep=k, min_frames=1)["counters"]["n_kept"]
         for name, p, k in (("all", r["canonical"], keep), ("frame0", r["canonical"], first), ("identity", c["points"], keep))}
    print(f"fused model voxels: {n}")
    assert n["frame0"] > 100 and n["all"] <= MODEL_CAP * n["frame0"] and n["identity"] >= SMEAR_MIN * n["frame0"], n


def test_argument_errors_need_no_gpu():
    T, H, W, K = 2, 3, 4, 2
    ids = torch.zeros(T, H, W, dtype=torch.int32)
    pts, grid = torch.zeros(T * H * W, 3), torch.tensor([0.0, 0.0, 0.0, 0.1])
    flow = torch.zeros(2, T, H, W)
    good = dict(object_id=ids, K=K, points=pts, grid=grid, flow_2thw=flow)
    bad = [dict(object_id=ids.float()), dict(object_id=ids[0]), dict(object_id="ids"), dict(K=-1), dict(K=(1 << 27)), dict(K=1.5),
           dict(points=pts[:-1]), dict(points=pts.int()), dict(points=None), dict(grid=grid[:3]), dict(grid=grid.int()), dict(grid=None),
           dict(flow_2thw=flow[0]), dict(flow_2thw=flow.int()), dict(n_refits=-1), dict(n_refits=0.5), dict(inlier_voxels=0.0),
           dict(inlier_voxels=-1.0), dict(inlier_voxels=float("nan")), dict(inlier_voxels=float("inf")), dict(min_pairs=2),
           dict(object_id=torch.zeros(1, 1025, 1024, dtype=torch.int32).expand(2, 1025, 1024), points=torch.zeros(1, 3).expand(2 * 1025 * 1024, 3))]
    for kw in bad:
        with pytest.raises(ValueError, match="rigid_motion"):
            OM.rigid_motion(**dict(good, **kw))
    with pytest.raises(ValueError, match="place_models"):
        OM.place_models(dict(xyz=torch.zeros(0, 3), object=torch.zeros(0, dtype=torch.int32)), torch.zeros(2, 3, 11), 0)
    with pytest.raises(ValueError, match="place_models"):
        OM.place_models(dict(xyz=torch.zeros(0, 3), object=torch.zeros(0, dtype=torch.int32)), torch.zeros(2, 3, 12), 3)
    with pytest.raises(ValueError, match="object_models"):
        OM.object_models(dict(object_id=ids, K=2, n_pixels=torch.zeros(2, dtype=torch.int32)), dict(canonical=pts), None, T, objects=[2])
    with pytest.raises(ValueError, match="world points"):
        OM.object_motion_from_outputs({}, {}, ["dyn_mask"], res=dict(object_id=ids, K=0))


def test_header_binds_the_new_entries():
    with open(os.path.join(ROOT, "include", "l4p_hip.h")) as fh:
        header = _header.parse(fh.read())
    sig = _header.bind(header).signatures
    for name, n_args in (("l4p_objects_motion_ws_bytes", 2), ("l4p_objects_motion", 22), ("l4p_objects_canonical", 9), ("l4p_objects_place", 9)):
        assert name in sig and len(sig[name][1]) == n_args, (name, sig.get(name))
    assert _lib.ABI_VERSION == 26
    import l4p.utils.object_motion as alias

    assert alias is OM


@pytest.fixture(scope="module")
def rotations(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("umeyama_rotation") / "umeyama_rotation_main")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "l4p_amd", "csrc"),
           os.path.join(ROOT, "tests", "umeyama_rotation_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    text = []
    for src, dst in UMEYAMA_CASES.values():
        text.append(str(len(src)))
        text += [" ".join(repr(float(x)) for x in np.concatenate([a, b])) for a, b in zip(src, dst)]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [np.array(line.split(), np.float64) for line in out.stdout.splitlines()]
    assert len(rows) == len(UMEYAMA_CASES) and all(r.size == 10 for r in rows)
    return dict(zip(UMEYAMA_CASES, rows))


def test_rotation_entry_matches_the_svd(rotations):
    """umeyama_rotation on the case list of tests/test_umeyama_moments_cpu.py: a proper rotation in every case (also where the scale
    of the similarity is 0 and the similarity entry emits s R = 0), the signed sum of the singular values, and R entry by entry where
    sigma2 / sigma1 >= RATIO_MIN, all at TOL["f64"]."""
    tol, compared = TOL["f64"], 0
    for name, (src, dst) in UMEYAMA_CASES.items():
        R, ssum = rotations[name][:9].reshape(3, 3), rotations[name][9]
        _, Rref, _, cov = MR.umeyama(src, dst)
        D = np.linalg.svd(cov, compute_uv=False)
        assert np.isfinite(rotations[name]).all(), name
        assert np.abs(R @ R.T - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1) <= tol, name
        signed = D[0] + D[1] + (D[2] if np.linalg.det(cov) >= 0 else -D[2])
        scale = max(D[0], 1e-300)
        if D[0] > 0 and (D[1] / D[0] >= RATIO_MIN or D[1] <= 1e-12 * D[0]):  # (between the two the route through cov^T cov loses sigma2)
            assert abs(ssum - signed) <= 1e-6 * scale, (name, ssum, signed)
        if D[0] > 0 and D[1] / D[0] >= RATIO_MIN:
            compared += 1
            assert np.abs(R - Rref).max() <= tol, (name, np.abs(R - Rref).max())
            assert abs(ssum - signed) <= tol * scale, (name, ssum, signed)
        if D[0] == 0:
            assert np.array_equal(R, np.eye(3)), name
    assert compared >= 40, compared


def test_demo_plan_adds_camray():
    import importlib.util

    spec = importlib.util.spec_from_file_location("demo_object_models_plan", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    base = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]
    a = demo.parse_args(["--synthetic", "--object-models", "out"])
    assert a.object_models == "out" and demo.plan(a)[0] == base + ["camray"]
    a = demo.parse_args(["--synthetic"])
    assert a.object_models is None and demo.plan(a)[0] == base


def test_sums_of_squares_past_2_63_in_the_restatement():
    """big_sums_case fills a row with 2^20 pairs at the far bound: the sums of squares pass 2^63 (negative as int64), nothing is far,
    the fit is the quarter turn and the rms that of the +-1 step jitter (sqrt(2 / 3) per axis, sqrt(2) in all: about 1.41 units)."""
    c = OR.big_sums_case()
    r = _restate(c, n_refits=0)
    assert r["n_pairs"][0].tolist() == [0, 1 << 20] and r["n_far"].sum() == 0 and r["valid"][0, 1] == 1
    assert (r["moments"][0, 1, 16:18] < 0).all() and (r["moments"][0, 1, 16:18].astype(np.uint64) > np.uint64(3 << 61)).all()
    assert r["ratio"][0, 1] >= RATIO_MIN and r["extent_d"][0, 1] >= (1 << 21) - 6
    assert np.abs(r["motion64"][0, 1, :9].reshape(3, 3) - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() <= 1e-6
    assert 1.3 < r["rms"][0, 1] < 1.5, r["rms"]
