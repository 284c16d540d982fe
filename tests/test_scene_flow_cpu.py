"""CPU: the scene-flow restatement against closed-form scenes, the generator's conditioning for every case the GPU tests list, the
demo's plan with --scene-flow, the wrappers' shape errors (raised before any native call) and consistency() on a hand-written
summary (l4p_amd/utils/scene_flow.py, tests/scene_flow_restate.py)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import scene_flow as SF
from tests import scene_flow_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every number below is dyadic, so the flow, q = p + F and the bilinear weights are exact in f32
FX, Z0, Z1 = 16.0, 2.0, 1.0
STEP = (0.09375, -0.03125)  # camera translation per frame -> plane flow FX * STEP / Z0 = (0.75, -0.25) px
OBJ = (0.0625, 0.125, 0.0)  # world displacement of the patch per frame


def _plane_scene(T=3, H=10, W=12, patch=False):
    depth = np.full((1, 1, T, H, W), Z0, dtype=np.float32)
    K = np.zeros((1, 4, 4, T), dtype=np.float32)
    P = np.zeros((1, 4, 4, T), dtype=np.float32)
    for t in range(T):
        K[0, :, :, t] = [[FX, 0, 5.5, 0], [0, FX, 4.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
        P[0, :, :, t] = np.eye(4)
        P[0, 0, 3, t], P[0, 1, 3, t] = STEP[0] * t, STEP[1] * t
    flow = np.zeros((1, 2, T, H, W), dtype=np.float32)
    flow[0, 0], flow[0, 1] = FX * STEP[0] / Z0, FX * STEP[1] / Z0
    rects = None
    if patch:
        # the patch is seen at rect_t in frame t; its flow (FX (STEP - OBJ) / Z1 = (0.5, -2.5) px) points into rect_{t-1}
        fpx, fpy = FX * (STEP[0] - OBJ[0]) / Z1, FX * (STEP[1] - OBJ[1]) / Z1
        assert (fpx, fpy) == (0.5, -2.5)
        rects = [(0, 5, 3, 10), (2, 7, 3, 9), (5, 9, 3, 8)][:T]  # (r0, r1, c0, c1) of frames 0, 1, 2: rect_{t-1} covers rect_t + flow
        for t, (r0, r1, c0, c1) in enumerate(rects):
            depth[0, 0, t, r0:r1, c0:c1] = Z1
            flow[0, 0, t, r0:r1, c0:c1], flow[0, 1, t, r0:r1, c0:c1] = fpx, fpy
    return depth, flow, P, K, rects


def test_restatement_on_a_translating_camera_over_a_plane():
    depth, flow, P, K, _ = _plane_scene()
    r = RS.restate(depth, flow, P, K)
    ext = RS.extent(r["X"])
    v = r["valid"][0, 0].astype(bool)
    assert not v[0].any() and v[1:].any() and not v[1:].all()  # frame 0 invalid; q leaves the image along two sides
    jj, ii = np.meshgrid(np.arange(10), np.arange(12), indexing="ij")
    want_inside = (ii + 0.75 <= 11) & (jj - 0.25 >= 0)
    assert np.array_equal(v[1], want_inside) and np.array_equal(v[2], want_inside)
    assert np.abs(r["scene"]).max() <= 1e-12 * ext
    assert np.abs(r["comp"]).max() <= 1e-12 * ext
    for c in range(2):
        assert np.abs(r["rigid"][0, c][v] - flow[0, c][v]).max() <= 1e-12 * ext
    for k in ("scene", "rigid", "comp"):
        assert (r[k][0, :, 0] == 0).all() and (r[k][0][:, ~v] == 0).all()


def test_restatement_on_a_displaced_patch():
    depth, flow, P, K, rects = _plane_scene(patch=True)
    r = RS.restate(depth, flow, P, K)
    ext = RS.extent(r["X"])
    checked = 0
    for t in (1, 2):
        r0, r1, c0, c1 = rects[t]
        p0, p1, q0, q1 = rects[t - 1]
        for j in range(r0, r1):
            for i in range(c0, c1):
                qx, qy = i + 0.5, j - 2.5
                taps_in = p0 <= math.floor(qy) and math.floor(qy) + 1 < p1 and q0 <= math.floor(qx) and math.floor(qx) + 1 < q1
                if not taps_in:
                    continue
                assert r["valid"][0, 0, t, j, i] == 1
                assert np.abs(r["scene"][0, :, t, j, i] + np.array(OBJ)).max() <= 1e-12 * ext  # S = -d
                # the object part of the flow: C = -K d / Z1
                assert np.abs(r["comp"][0, :, t, j, i] - np.array([-FX * OBJ[0] / Z1, -FX * OBJ[1] / Z1])).max() <= 1e-12 * ext
                checked += 1
    assert checked >= 12


def test_restatement_without_a_frame_pair():
    depth, flow, P, K, _ = _plane_scene(T=1)
    r = RS.restate(depth, flow, P, K)
    for k in ("scene", "rigid", "comp", "valid"):
        assert not r[k].any(), k
    assert not RS.restate_summary(r["scene"], r["comp"], r["valid"]).any()


@pytest.mark.parametrize("case", RS.PARITY_CASES + [RS.ADVERSARIAL_CASE])
def test_generator_meets_its_conditions_for_every_listed_case(case):
    """make_case asserts the two conditions itself; here also: the case is not degenerate (T > 1: both valid and invalid pixels,
    both mask classes among the valid ones) and the fields are bounded as the 2D tolerance rule assumes."""
    seed, B, T, H, W = case
    c = RS.make_case(*case)
    assert c["depth"].min() >= 1 and c["depth"].max() <= 4
    f = c["K"][:, [0, 1], [0, 1], :]
    assert f.min() >= 0.8 * max(H, W) and f.max() <= 1.5 * max(H, W)
    if B > 1:
        assert not np.array_equal(c["K"][0], c["K"][1]) and not np.array_equal(c["P"][0], c["P"][1])
    if T > 2:
        assert not np.array_equal(c["K"][..., 1], c["K"][..., 2])
    r = RS.restate(c["depth"], c["flow"], c["P"], c["K"])
    v = r["valid"][:, 0].astype(bool)
    assert not v[:, 0].any()
    if T > 1:
        assert v[:, 1:].any() and not v[:, 1:].all()
        m = c["mask"][:, 0]
        assert (v & (m > 0)).any() and (v & (m <= 0)).any()
        assert np.abs(r["rigid"]).max() <= max(H, W)
        # static pixels: the flow is the rigid flow (rounded to f32); object pixels carry the perturbation
        assert np.abs(r["comp"][:, :, 1:][np.broadcast_to((v & (m <= 0))[:, None, 1:], r["comp"][:, :, 1:].shape)]).max() <= 1e-5
        assert np.abs(r["comp"]).max() > 0.1


def _load_demo():
    spec = importlib.util.spec_from_file_location("demo_scene_flow_args", os.path.join(ROOT, "demo", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_plan_with_and_without_scene_flow():
    demo = _load_demo()
    base = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]
    kw = dict(crop_size=(64, 224, 224), estimation_directions=[1], track_2d_querry_sampling_spacing=0.04)
    a = demo.parse_args(["--synthetic", "--scene-flow", "out"])
    assert a.scene_flow == "out" and demo.plan(a) == (base + ["camray"], kw)
    a = demo.parse_args(["--synthetic", "--scene-flow", "out", "--view4d", "v", "--frames", "16"])
    assert demo.plan(a) == (base + ["camray"], dict(kw, crop_size=(16, 224, 224)))
    # the existing flag combinations, as literals
    dv = dict(kw, track_2d_querry_sampling_spacing=0.02)
    for argv, want in (
            (["--synthetic"], (base, kw)),
            (["--synthetic", "--vis", "o"], (base, kw)),
            (["--synthetic", "--save", "o", "--frames", "16"], (base, dict(kw, crop_size=(16, 224, 224)))),
            (["--synthetic", "--recon4d", "o"], (base + ["camray"], kw)),
            (["--synthetic", "--view4d", "o"], (base + ["camray"], kw)),
            (["--synthetic", "--bidirectional"], (base, dict(kw, estimation_directions=[1, -1]))),
            (["--synthetic", "--davis", "X"], (base, dv)),
            (["--synthetic", "--davis", "X", "--recon4d", "o"], (base + ["camray"], dict(dv, crop_size=(56, 224, 224)))),
            (["--synthetic", "--davis", "X", "--view4d", "o"], (base + ["camray"], dict(dv, crop_size=(56, 224, 224)))),
            (["--synthetic", "--dycheck", "X"], (base + ["camray"], dict(kw, resize_size=(298, 224), stride=2))),
            (["--synthetic", "--spacing", "0.1", "--max-queries", "8"], (base, dict(kw, track_2d_querry_sampling_spacing=0.1)))):
        a = demo.parse_args(argv)
        assert a.scene_flow is None and demo.plan(a) == want, argv


def test_shape_errors_are_raised_before_any_native_call():
    B, T, H, W = 2, 3, 4, 5
    d, f = torch.zeros(B, 1, T, H, W), torch.zeros(B, 2, T, H, W)
    P, K = torch.zeros(B, 4, 4, T), torch.zeros(B, 4, 4, T)
    for args, name in (((d[:, 0], f, P, K), "depth_b1thw"), ((d, f[:, :1], P, K), "flow_b2thw"), ((d, f[:, :, :2], P, K), "flow_b2thw"),
                       ((d, f, P[..., :2], K), "world_T_cam_b44t"), ((d, f, P, K[:1]), "intrinsics_b44t"),
                       ((d, f, P, K, d[..., :3]), "dyn_mask_b1thw"), ((d[:, :, :, :0], f[:, :, :, :0], P, K), "depth_b1thw")):
        with pytest.raises(ValueError, match=name):
            SF.scene_flow(*args)
    with pytest.raises(AssertionError, match="GPU"):  # right shapes, host tensors: the device check comes after the shape checks
        SF.scene_flow(d, f, P, K)
    out = {"depth_est_b1thw": d, "flow_2d_backward_est_b2thw": f}
    tasks = ["depth", "flow_2d_backward", "camray"]
    for missing in ("depth", "flow_2d_backward", "camray"):
        with pytest.raises(AssertionError, match="Tasks must include"):
            SF.scene_flow_from_outputs({}, out, [t for t in tasks if t != missing])
    with pytest.raises(ValueError, match="traj3d_est_b16t"):
        SF.scene_flow_from_outputs({}, out, tasks)
    with pytest.raises(ValueError, match="camray_est_b6thw"):
        SF.scene_flow_from_outputs({}, dict(out, camray_est_b6thw=d), tasks)
    with pytest.raises(ValueError, match="traj3d_intrinsics_est_b16t"):
        SF.scene_flow_from_outputs({}, dict(out, traj3d_est_b16t=torch.zeros(B, 16, T), traj3d_intrinsics_est_b16t=torch.zeros(B, 16, T + 1)),
                                   tasks)
    with pytest.raises(ValueError, match="summary_bt8"):
        SF.consistency(torch.zeros(3, 8))


def test_native_entries_refuse_null_and_negative_arguments():
    """The argument checks come before anything touches a device: L4P_E_INVALID and a text that names the entry."""
    from l4p_amd import _lib

    lib = _lib.load()
    p = 256  # never dereferenced: every call below is refused
    for name, good in (("l4p_scene_flow", [None, p, p, p, p, None, 1, 2, 3, 4, p, p, p, p]),
                       ("l4p_scene_flow_summary", [None, p, p, p, None, 1, 2, 3, 4, 1.0, p, p]),
                       ("l4p_scene_flow_colors", [None, p, p, p, 1, 2, 3, 4, p, p])):
        fn = getattr(lib, name)
        optional = {0, 5} if name == "l4p_scene_flow" else ({0, 4} if name == "l4p_scene_flow_summary" else {0})
        for k, v in enumerate(good):
            if k in optional or isinstance(v, float):
                continue
            bad = list(good)
            bad[k] = None if v == p else -1
            assert fn(*bad) == -1, (name, k)
            assert name + ":" in lib.l4p_last_error().decode(), (name, k)
            if v != p:
                bad[k] = 0
                assert fn(*bad) == -1, (name, k)


def test_consistency_on_a_hand_written_summary():
    # columns: n_valid, n_static, n_dynamic, sum|C| static, dynamic, sum|S| static, dynamic, n_moving
    s = torch.tensor([[[0, 0, 0, 0, 0, 0, 0, 0], [10, 8, 2, 4.0, 6.0, 0.8, 1.0, 3], [30, 24, 6, 4.0, 2.0, 2.4, 1.0, 5]],
                      [[0, 0, 0, 0, 0, 0, 0, 0], [5, 5, 0, 2.5, 0, 1.0, 0, 0], [5, 5, 0, 2.5, 0, 1.0, 0, 1]],
                      [[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]], dtype=torch.float64)
    c = SF.consistency(s, pixels_per_frame=20)
    nan = float("nan")
    want = {"rigid_epe_static": [0.25, 0.5, nan], "rigid_epe_dynamic": [1.0, nan, nan], "scene_speed_static": [0.1, 0.2, nan],
            "scene_speed_dynamic": [0.25, nan, nan], "moving_fraction": [0.2, 0.1, nan], "valid_fraction": [1.0, 0.25, 0.0]}
    assert set(c) == set(want)
    for k, w in want.items():
        assert c[k].dtype == torch.float64 and c[k].shape == (3,)
        np.testing.assert_allclose(c[k].numpy(), np.array(w), rtol=1e-15, atol=0, equal_nan=True, err_msg=k)
    assert "valid_fraction" not in SF.consistency(s)
    one = SF.consistency(s[:, :1], pixels_per_frame=20)  # T = 1: no frame pair, every denominator 0
    assert all(torch.isnan(v).all() for v in one.values())


def test_motion_lut_and_restated_colours():
    lut = SF.motion_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (48, 18, 59) and tuple(lut[255]) == (122, 4, 2)  # 0.18995 * 255 = 48.4..., 0.4796 * 255 = 122.2...
    scene = np.zeros((1, 3, 1, 1, 4), dtype=np.float32)
    scene[0, 0, 0, 0] = [0.0, 0.5, 1.0, 7.0]
    col = RS.restate_colors(scene, np.array([1, 1, 1, 0], dtype=np.uint8).reshape(1, 1, 1, 1, 4), 1.0)
    assert np.array_equal(col[0], [lut[0], lut[127], lut[255], (128, 128, 128)])
