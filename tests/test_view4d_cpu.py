"""CPU: the host side of the free-viewpoint 4D renderer (l4p_amd/utils/view4d.py: the orbit camera path, the frame schedule, the
argument handling) and the properties of the numpy restatement (tests/view4d_restate.py) that the GPU tests rely on."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from l4p_amd.utils import view4d as V4
from tests import recon4d_restate as RS
from tests import view4d_restate as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ["depth", "camray", "track_2d"]
T, HW = 24, 1024


@pytest.fixture(scope="module")
def scene():
    sc = RS.make_scene()
    batch, out = RS.scene_tensors(sc)
    return sc, batch, out, RS.restate(batch, out, TASKS)


def _poses(rec):
    return np.transpose(rec["world_T_cam"][0], (2, 0, 1)).astype(np.float64)  # [T, 4, 4]


def test_orbit_with_zero_yaw_pitch_and_pull_back_returns_the_estimated_cameras(scene):
    _, _, out, rec = scene
    trec = {"world_T_cam": torch.from_numpy(rec["world_T_cam"])}
    W = _poses(rec)
    d = out["depth_est_b1thw"][0, 0, 0].reshape(-1).numpy()
    d0 = np.sort(d[np.isfinite(d) & (d > 0)])[(d.size - 1) // 2]  # the lower median (every depth of the scene is positive)
    for anchor in ("follow", "first"):
        p = V4.orbit_views(trec, out["depth_est_b1thw"], T, 2 * T, anchor=anchor, yaw=0.0, pitch=0.0, pull_back=0.0)
        assert p["d0"] == float(d0)
        want = np.linalg.inv(W[p["frames"]] if anchor == "follow" else W[np.zeros(2 * T, dtype=int)])
        assert np.abs(p["cam_T_world"] - want).max() <= 1e-12
    with pytest.raises(ValueError):
        V4.orbit_path(W, 1.0, 4, anchor="orbit")
    with pytest.raises(ValueError):
        V4.orbit_views(trec, torch.full((1, 1, T, 4, 4), float("nan")), T, 4)


@pytest.mark.parametrize("anchor", ["first", "follow"])
def test_orbit_rotations_are_orthonormal_and_the_look_at_point_projects_to_the_principal_point(scene, anchor):
    _, _, _, rec = scene
    W = _poses(rec)
    d0, pull = 2.25, 0.5
    p = V4.orbit_path(W, d0, 37, anchor=anchor, yaw=0.7, pitch=0.3, pull_back=pull)
    K = (60.0, 56.0, 47.5, 32.0)
    moved = 0.0
    for v in range(37):
        M = p["cam_T_world"][v]
        a = W[0 if anchor == "first" else p["frames"][v]]
        # the path's own rotation (relative to the anchor pose) to float64 accuracy; the whole view matrix as far as the
        # estimated f32 pose is orthonormal itself (its entries carry 6e-8 of rounding)
        for R, tol in (((M @ a)[:3, :3], 1e-12), (M[:3, :3], 1e-6)):
            assert np.abs(R @ R.T - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1) <= tol
        assert np.abs(M[3] - [0, 0, 0, 1]).max() <= 1e-12
        assert np.abs(p["look_at"][v] - (a @ [0, 0, d0, 1])[:3]).max() <= 1e-12
        c = M @ np.append(p["look_at"][v], 1.0)
        assert abs(c[0]) <= 1e-12 and abs(c[1]) <= 1e-12 and abs(c[2] - d0 * (1 + pull)) <= 1e-12
        u, w, z, ok = VS.project(p["look_at"][v][None], M, K, 1e-3, np.float64)  # f32 inputs: 1e-7 relative
        assert ok[0] and abs(u[0] - K[2]) <= 1e-4 and abs(w[0] - K[3]) <= 1e-4
        moved = max(moved, np.abs(M - np.linalg.inv(a)).max())
    assert moved > 0.1  # the path does leave the estimated camera
    # view 0 sits on the anchor's optical axis, pulled back
    q = V4.orbit_path(W[:1].repeat(38, 0), d0, 38, yaw=0.7, pitch=0.3, pull_back=pull)
    assert np.abs(q["cam_T_world"][0] - np.linalg.inv(W[0] @ V4._tz(-d0 * pull))).max() <= 1e-12


def test_frame_schedule():
    for Tn, Vn in ((24, 24), (24, 48), (24, 7), (24, 1), (5, 64), (64, 64)):
        f = V4.view_frames(Tn, Vn)
        assert f.shape == (Vn,) and f.tolist() == [math.floor(v * Tn / Vn) for v in range(Vn)]
        assert f[0] == 0 and f.max() < Tn and (np.diff(f) >= 0).all()
    assert V4.view_frames(24, 24).tolist() == list(range(24))


def test_identity_views_of_the_restatement_return_every_pixel(scene):
    """V = T views equal to the estimated cameras with each frame's own K, point_size = 0, dense points only: every point lands on
    the pixel it was unprojected from - 0 of 24 576 pixels miss."""
    sc, _, _, rec = scene
    cams = np.transpose(rec["cam_T_ref"][0], (2, 0, 1))
    K = np.stack([sc["K"][0], sc["K"][5], sc["K"][2], sc["K"][6]], 1)
    r = VS.render(rec, T, HW, cams, K, (32, 32), np.arange(T), point_size=0.0, tracks=False, stride=-1)
    assert r["writes"] == r["covered"] == T * HW
    assert int((r["index"] != np.arange(HW, dtype=np.int32).reshape(1, 32, 32)).sum()) == 0
    assert np.array_equal(r["image"], rec["colors"].reshape(T, 32, 32, 3))
    assert np.abs(r["depth"] - (1 + sc["depth_q"].astype(np.float32) / 64)).max() <= 1e-5 * 5  # camera z = the depth it came from


def off_axis_view(rec):
    """The occlusion view of the GPU tests: frame 12 from world_T_cam[12] . Tz(2) . Ry(0.35) . Tz(-2) . Tz(-1)."""
    W = _poses(rec)
    pose = W[12] @ V4._tz(2) @ V4._ry(0.35) @ V4._tz(-2) @ V4._tz(-1)
    return np.linalg.inv(pose)[None], (60.0, 56.0, 47.5, 32.0), (64, 96), [12], dict(point_size=0.12, max_half=6)


def test_off_axis_view_of_the_restatement_is_an_occlusion_test(scene):
    _, _, _, rec = scene
    cam, K, size, frames, kw = off_axis_view(rec)
    a = VS.render(rec, T, HW, cam, K, size, frames, stride=-1, **kw)
    assert (a["writes"], a["covered"]) == (24192, 2232)  # most writes lose a depth test
    b = VS.render(rec, T, HW, cam, K, size, frames, stride=-1, dtype=np.float64, **kw)
    diff = int((a["index"] != b["index"]).sum())
    print("f32 against f64 restatement: index differs at", diff, "of", a["index"].size, "pixels")
    assert diff <= 0.005 * a["index"].size
    assert (a["index"] >= HW).any() and (a["index"] < HW).any()  # trail points and dense points are both seen
    # frusta: drawn ones, colours, codes
    c = VS.render(rec, T, HW, cam, K, size, frames, stride=4, **kw)
    tri = c["index"] < -1
    codes = c["index"][tri].view(np.uint32) & 0x7FFFFFFF
    assert tri.sum() > 100 and set((codes >> 4).tolist()) <= {0, 4, 8, 12} and (codes & 15).max() < 12
    assert np.array_equal(c["image"][tri], V4.mesh_colours()[codes & 15])
    assert VS.drawn_frusta(13, 4) == [0, 4, 8, 12, 13] and VS.drawn_frusta(13, 0) == [13] and VS.drawn_frusta(0, 1) == [0]


def test_argument_handling():
    assert V4.frusta_stride("current") == 0 and V4.frusta_stride(4) == 4
    assert V4.frusta_stride(None) == V4.frusta_stride("none") == V4.frusta_stride(False) == -1
    for bad in (0, -2, True, "all", 2.5):
        with pytest.raises(ValueError):
            V4.frusta_stride(bad)
    m = V4.mesh_colours()
    assert m.shape == (12, 3) and m.dtype == np.uint8 and m[0].tolist() == [255, 127, 127] and len({tuple(c) for c in m.tolist()}) == 12
    K = np.array([[30.0, 0, 15.5, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert V4.scaled_intrinsics(K, (32, 32), (32, 32)) == (30.0, 28.0, 15.5, 16.0)
    assert V4.scaled_intrinsics(K, (32, 32), (64, 96)) == (90.0, 56.0, 47.5, 32.5)


def test_alias_and_demo_flag():
    code = ("import l4p.utils.view4d as a, l4p_amd.utils.view4d as b\nassert a is b\n"
            "try:\n    import l4p.utils.viser\n    raise RuntimeError('imported')\nexcept ImportError:\n    pass\n"
            "import sys\nsys.path.insert(0, 'demo')\nimport demo\n"
            "a = demo.parse_args(['--synthetic', '--view4d', 'out'])\n"
            "assert a.view4d == 'out' and demo.plan(a)[0][-1] == 'camray'\n"
            "assert 'camray' not in demo.plan(demo.parse_args(['--synthetic']))[0]\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
