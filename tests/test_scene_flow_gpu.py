"""GPU: dense scene flow / rigid flow / camera-compensated flow (l4p_amd/utils/scene_flow.py, csrc/sceneflow.hip) against the float64
restatement (tests/scene_flow_restate.py).

Pass rule of every comparison with the restatement: `valid` exactly equal; 3D fields within 1e-5 extent(X) (the rule of
tests/test_recon4d_gpu.py); 2D fields within 1e-5 (max(H, W) + max|F|): the chain is about 30 f32 roundings on quantities bounded
by that extent under make_case's conditioning, 30 * 6e-8 ~ 2e-6.  Summary counts exactly equal, sums within 1e-12 relative of the
f64 sum of the restated f32 magnitudes (only the summation order differs)."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import recon4d as R
from l4p_amd.utils import scene_flow as SF
from l4p_amd.utils import vis2d
from tests import scene_flow_restate as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"scene": "scene_flow_backward_b3thw", "rigid": "rigid_flow_2d_backward_b2thw", "comp": "compensated_flow_2d_backward_b2thw",
          "valid": "scene_flow_valid_b1thw"}
_CASES = {}


def _case(key):
    """(inputs, restatement) of a (seed, B, T, H, W) case, computed once and left unchanged."""
    if key not in _CASES:
        c = RS.make_case(*key)
        _CASES[key] = (c, RS.restate(c["depth"], c["flow"], c["P"], c["K"]))
    return _CASES[key]


def _gpu(c, mask=True, tau=1.0):
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    res = SF.scene_flow(t["depth"], t["flow"], t["P"], t["K"], t["mask"] if mask else None, tau)
    return res, {k: v.cpu().numpy() for k, v in res.items()}


def _check_fields(got, want, c, tag, flow=None):
    """``flow``: the flow whose largest magnitude enters the 2D bound (the unchanged case's, where ``c`` holds adversarial values)."""
    B, _, T, H, W = c["depth"].shape
    tol3 = 1e-5 * RS.extent(want["X"])
    tol2 = 1e-5 * (max(H, W) + float(np.abs(c["flow"] if flow is None else flow).max()))
    e3 = float(np.abs(got[FIELDS["scene"]] - want["scene"]).max())
    e2 = max(float(np.abs(got[FIELDS[k]] - want[k]).max()) for k in ("rigid", "comp"))
    nv = int((got[FIELDS["valid"]] != want["valid"]).sum())
    print(f"{tag}: valid differs on {nv} of {want['valid'].size}, 3D err {e3:.3e} (bound {tol3:.3e}), 2D err {e2:.3e} (bound {tol2:.3e})")
    for k, name in FIELDS.items():
        assert got[name].shape == want[k].shape and got[name].dtype == (np.uint8 if k == "valid" else np.float32), k
    assert nv == 0
    assert e3 <= tol3 and e2 <= tol2
    inv = got[FIELDS["valid"]][:, 0] == 0
    for k in ("scene", "rigid", "comp"):
        assert (np.moveaxis(got[FIELDS[k]], 1, 0)[:, inv] == 0).all(), k


def _check_summary(got, c, mask, tau, tag):
    want = RS.restate_summary(got[FIELDS["scene"]], got[FIELDS["comp"]], got[FIELDS["valid"]], c["mask"] if mask else None, tau)
    s = got["summary_bt8"]
    assert s.shape == want.shape and s.dtype == np.float64
    rel = np.abs(s - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{tag}: summary rows\n{s}\nlargest relative difference of the sums {float(rel[..., 3:7].max()):.3e}")
    assert np.array_equal(s[..., [0, 1, 2, 7]], want[..., [0, 1, 2, 7]])
    assert (np.abs(s[..., 3:7] - want[..., 3:7]) <= 1e-12 * np.abs(want[..., 3:7])).all()
    assert (s[:, 0] == 0).all()  # frame 0


@pytest.mark.parametrize("key", RS.PARITY_CASES)
def test_parity_with_the_restatement(dev, key):
    c, want = _case(key)
    _, got = _gpu(c, tau=0.5)
    _check_fields(got, want, c, str(key))
    _check_summary(got, c, True, 0.5, str(key))
    if key[2] == 1:  # no frame pair: everything is zero
        assert not any(got[n].any() for n in list(FIELDS.values()) + ["summary_bt8"])
    else:
        assert got[FIELDS["valid"]][:, :, 1:].any() and got["summary_bt8"][:, 1:, 7].sum() > 0


def _taps_touch(c, changed_depth):
    """bool [T, H, W]: pixels of frame t whose four taps (of the case's own flow) meet a changed pixel of depth plane t - 1."""
    _, _, T, H, W = c["depth"].shape
    hit = np.zeros((T, H, W), dtype=bool)
    for t in range(1, T):
        *_, inside, (x0, x1, y0, y1), _w = RS._taps(c["flow"][0, :, t], H, W)
        ch = changed_depth[t - 1]
        hit[t] = inside & (ch[y0, x0] | ch[y0, x1] | ch[y1, x0] | ch[y1, x1])
    return hit


def test_adversarial_inputs_are_invalid_and_leave_the_rest_alone(dev):
    base, _ = _case(RS.ADVERSARIAL_CASE)
    _, ref = _gpu(base)
    _, _, T, H, W = base["depth"].shape
    c = {k: v.copy() for k, v in base.items()}
    own = np.zeros((T, H, W), dtype=bool)  # pixels whose own inputs are made adversarial: they must come out invalid
    inf, nan = float("inf"), float("nan")
    # flow that leaves the image on each side, NaN and Inf flow (frame 1), non-positive depth in frame t (frame 2)
    for (t, j, i), (ch, val) in {(1, 0, 0): (0, -1.5), (1, 1, W - 1): (0, 1.5), (1, 0, 3): (1, -1.25), (1, H - 1, 4): (1, 1.25),
                                 (1, 2, 2): (0, nan), (1, 3, 2): (1, nan), (1, 2, 5): (0, inf), (1, 3, 5): (1, -inf),
                                 (1, 4, 6): (0, 1e30), (2, 1, 1): (0, nan)}.items():
        c["flow"][0, ch, t, j, i] = val
        own[t, j, i] = True
    for (t, j, i), val in {(2, 4, 4): 0.0, (2, 5, 7): -1.0, (2, 6, 2): -0.0}.items():
        c["depth"][0, 0, t, j, i] = val
        own[t, j, i] = True
    # non-positive depth in frame t - 1: two blocks of frame 0, which the taps of frame 1 meet
    changed = np.zeros((T, H, W), dtype=bool)
    c["depth"][0, 0, 0, 5:9, 6:11] = 0.0
    c["depth"][0, 0, 0, 5:9, 0:4] = -1.0
    changed[0, 5:9, 0:4] = changed[0, 5:9, 6:11] = True
    want = RS.restate(c["depth"], c["flow"], c["P"], c["K"])
    _, got = _gpu(c)
    _check_fields(got, want, c, "adversarial", flow=base["flow"])
    v = got[FIELDS["valid"]][0, 0]
    assert not v[own].any()
    # all four taps in a non-positive block: d' <= 0
    *_, inside, (x0, x1, y0, y1), _w = RS._taps(c["flow"][0, :, 1], H, W)
    allin = inside & changed[0][y0, x0] & changed[0][y0, x1] & changed[0][y1, x0] & changed[0][y1, x1]
    assert allin.sum() >= 4 and not v[1][allin].any()
    # everything the changes do not reach keeps its bits
    same = ~(own | _taps_touch(c, changed))
    assert same[1:].sum() > (T - 1) * H * W // 3
    for name in FIELDS.values():
        assert np.array_equal(np.moveaxis(got[name], 1, 0)[:, 0][:, same], np.moveaxis(ref[name], 1, 0)[:, 0][:, same]), name
    # a pose that puts X_t behind camera t - 1: camera 0 turned by 180 degrees about y -> frame 1 invalid, frame 2 untouched
    c = {k: v.copy() for k, v in base.items()}
    c["P"][0, :, :, 0] = c["P"][0, :, :, 0] @ np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    want = RS.restate(c["depth"], c["flow"], c["P"], c["K"])
    assert (want["xcz"][0, 0, 1] < -0.5).all()
    _, got = _gpu(c)
    _check_fields(got, want, c, "behind the camera")
    assert not got[FIELDS["valid"]][0, 0, 1].any()
    for name in FIELDS.values():
        assert np.array_equal(got[name][:, :, 2], ref[name][:, :, 2]), name


def test_summary_is_reproducible_and_follows_the_mask(dev):
    key = RS.PARITY_CASES[-1]  # three reduction chunks per frame
    c, _ = _case(key)
    assert key[3] * key[4] > 2 * SF.SUMMARY_CHUNK
    a_t, a = _gpu(c, tau=0.25)
    b_t, _ = _gpu(c, tau=0.25)
    for k in a_t:
        assert torch.equal(a_t[k].view(torch.uint8), b_t[k].view(torch.uint8)), k  # bit for bit
    _, n = _gpu(c, mask=False, tau=0.25)
    _check_summary(n, c, False, 0.25, "no mask")
    s, sn = a["summary_bt8"], n["summary_bt8"]
    assert np.array_equal(sn[..., 1], sn[..., 0]) and not sn[..., [2, 4, 6]].any()
    assert np.array_equal(sn[..., [0, 7]], s[..., [0, 7]])
    assert np.array_equal(s[..., 1] + s[..., 2], s[..., 0]) and s[:, 1:, 1].min() > 0 and s[:, 1:, 2].min() > 0
    for k in FIELDS.values():
        assert np.array_equal(a[k], n[k]), k  # the fields do not depend on the mask
    cons = {k: v.cpu().numpy() for k, v in SF.consistency(a_t["summary_bt8"], pixels_per_frame=key[3] * key[4]).items()}
    tot = s.sum(axis=1)
    np.testing.assert_allclose(cons["rigid_epe_static"], tot[:, 3] / tot[:, 1], rtol=1e-15)
    np.testing.assert_allclose(cons["valid_fraction"], tot[:, 0] / ((key[2] - 1) * key[3] * key[4]), rtol=1e-15)
    # static pixels carry the rigid flow itself: their mean |C| is within the 2D bound; the object's perturbation is far above it
    assert cons["rigid_epe_static"][0] <= 1e-5 * (max(key[3:]) + float(np.abs(c["flow"]).max())) < 0.1 < cons["rigid_epe_dynamic"][0]


def test_input_dtypes_and_layouts_give_the_same_bits(dev):
    c, _ = _case(RS.PARITY_CASES[2])
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    names = ("depth", "flow", "P", "K", "mask")
    for dt in (torch.bfloat16, torch.float16):
        low = [t[k].to(dt) for k in names]
        a = SF.scene_flow(*low, tau_px=0.5)
        b = SF.scene_flow(*[x.float().contiguous() for x in low], tau_px=0.5)
        assert a[FIELDS["valid"]].any()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (dt, k)
    views = [t[k].transpose(-1, -2).contiguous().transpose(-1, -2) for k in ("depth", "flow", "mask")]
    mats = [t[k].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for k in ("P", "K")]
    assert not any(x.is_contiguous() for x in views + mats)
    a = SF.scene_flow(views[0], views[1], mats[0], mats[1], views[2], tau_px=0.5)
    b = SF.scene_flow(*[t[k] for k in names], tau_px=0.5)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def _outputs(seed, T, H, W):
    """A synthetic (batch, out, tasks) of one clip around make_case: the poses go in as the camray head's traj3d_est_b16t."""
    c = RS.make_case(seed, 1, T, H, W)
    g = torch.Generator().manual_seed(seed)
    f = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    batch = {"rgb_b3thw": ((torch.randint(0, 256, (1, 3, T, H, W), generator=g).float() - 128) / 64).cuda(),
             "rgb_mean_b3111": torch.tensor((0.485, 0.456, 0.406)).reshape(1, 3, 1, 1, 1).cuda(),
             "rgb_std_b3111": torch.tensor((0.229, 0.224, 0.225)).reshape(1, 3, 1, 1, 1).cuda(), "seq_name": ["clip"]}
    out = {"depth_est_b1thw": f(c["depth"]), "flow_2d_backward_est_b2thw": f(c["flow"]), "dyn_mask_est_b1thw": f(c["mask"]),
           "traj3d_est_b16t": f(c["P"]).reshape(1, 16, T), "traj3d_intrinsics_est_b16t": f(c["K"]).reshape(1, 16, T)}
    return c, batch, out, ["depth", "flow_2d_backward", "dyn_mask", "camray"]


def test_from_outputs_lives_in_the_frame_of_reconstruct_4d(dev):
    T, H, W = 3, 17, 19
    c, batch, out, tasks = _outputs(21, T, H, W)
    res = SF.scene_flow_from_outputs(batch, out, tasks)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    rec = R.reconstruct_4d(batch, out, ["depth", "camray"])
    assert torch.equal(res["world_T_cam_b44t"], rec["world_T_cam"])
    assert np.abs(got["world_T_cam_b44t"][0, :, :, 0] - np.eye(4)).max() <= 1e-6  # re-referenced to frame 0
    want = RS.restate(c["depth"], c["flow"], got["world_T_cam_b44t"], got["intrinsics_b44t"])
    _check_fields(got, want, c, "from outputs")
    _check_summary(got, c, True, 1.0, "from outputs")
    pts = rec["points"].cpu().numpy().reshape(T, H, W, 3).transpose(3, 0, 1, 2)  # [3, T, H, W]
    ext = RS.extent(want["X"])
    assert np.abs(pts - want["X"][0]).max() <= 1e-5 * ext  # X_t rebuilt from the returned pieces
    v = got[FIELDS["valid"]][0, 0].astype(bool)
    assert v.sum() > H * W
    assert np.abs((pts + got[FIELDS["scene"]][0]) - want["Xp"][0])[:, v].max() <= 1e-5 * ext  # points_t + S_t = X'_{t-1}


def test_motion_colours(dev):
    c, _ = _case(RS.PARITY_CASES[2])
    res, got = _gpu(c)
    scene, valid = got[FIELDS["scene"]], got[FIELDS["valid"]]
    for s_max in (0.03, 0.2, 5.0):
        col = SF.motion_colors(res, s_max=s_max)
        assert col.dtype == torch.uint8 and tuple(col.shape) == (2, 3 * 17 * 19, 3)
        assert np.array_equal(col.cpu().numpy(), RS.restate_colors(scene, valid, s_max))
    assert torch.equal(SF.motion_colors(res, s_max=torch.tensor([0.2], device="cuda")), SF.motion_colors(res, s_max=0.2))
    # the default scale: torch.quantile of the same values, to the rounding that l4p_quantile's own test allows
    s = SF.default_s_max(res)
    mag = (res[FIELDS["scene"]] * res[FIELDS["scene"]]).sum(dim=1).sqrt().reshape(-1)
    q = float(torch.quantile(mag.cpu(), 0.98))
    assert q > 0 and abs(float(s) - q) <= 1e-6 * q
    assert (mag == 0).sum() > mag.numel() // 3  # the zeros of frame 0 and of invalid pixels are part of the sample
    assert np.array_equal(SF.motion_colors(res).cpu().numpy(), RS.restate_colors(scene, valid, float(s)))
    # a zero quantile (no frame pair): scale 1, every pixel invalid and grey
    c1, _ = _case(RS.PARITY_CASES[0])
    res1, _ = _gpu(c1)
    assert float(SF.default_s_max(res1)) == 1.0
    assert (SF.motion_colors(res1).cpu().numpy() == 128).all()


def test_scene_flow_video(dev, tmp_path):
    T, H, W = 3, 16, 20
    c, batch, out, tasks = _outputs(22, T, H, W)
    res = SF.scene_flow_from_outputs(batch, out, tasks)
    video, name = SF.generate_scene_flow_video(batch, out, tasks, str(tmp_path))
    assert video.shape == (T, H, 3 * W, 3) and video.dtype == np.float32
    first = vis2d.render_video_panels(batch, out, ["flow_2d_backward"])["video"].cpu().numpy()
    assert np.array_equal(video[:, :, :2 * W], first)
    out2 = dict(out, flow_2d_backward_est_b2thw=res[FIELDS["comp"]])
    third = vis2d.render_video_panels(batch, out2, ["flow_2d_backward"])["video"].cpu().numpy()[:, :, W:]
    assert np.array_equal(video[:, :, 2 * W:], third) and not np.array_equal(third, first[:, :, W:])
    try:
        import mediapy  # noqa: F401
    except ImportError:
        assert name == os.path.join(str(tmp_path), "clip_sceneflow")
        assert np.array_equal(vis2d.read_png_frames(name), vis2d.to_uint8(video))
    else:
        assert name == os.path.join(str(tmp_path), "clip_sceneflow.mp4") and os.path.exists(name)


def test_demo_scene_flow_branch(dev, tmp_path):
    """demo.run's scene-flow branch on a synthetic `out` (a run of demo.main builds the full-size model: not a few seconds)."""
    spec = importlib.util.spec_from_file_location("demo_scene_flow_run", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    T, H, W = 3, 16, 20
    _, batch, out, tasks = _outputs(23, T, H, W)
    d, v = str(tmp_path / "sf"), str(tmp_path / "v4")
    demo.scene_flow(batch, out, tasks, d, view4d_dir=v)
    z = np.load(os.path.join(d, "clip_sceneflow.npz"))
    want = {"scene_flow_backward_b3thw": ((1, 3, T, H, W), np.float16), "rigid_flow_2d_backward_b2thw": ((1, 2, T, H, W), np.float32),
            "compensated_flow_2d_backward_b2thw": ((1, 2, T, H, W), np.float32), "scene_flow_valid_b1thw": ((1, 1, T, H, W), np.uint8)}
    assert set(z.files) == set(want)
    for k, (shape, dt) in want.items():
        assert z[k].shape == shape and z[k].dtype == dt, k
    assert z["scene_flow_valid_b1thw"].any()
    numbers = json.load(open(os.path.join(d, "clip_sceneflow.json")))
    s = SF.scene_flow_from_outputs(batch, out, tasks)["summary_bt8"].cpu().numpy().sum(axis=1)[0]
    dens = {"rigid_epe_static": s[1], "rigid_epe_dynamic": s[2], "scene_speed_static": s[1], "scene_speed_dynamic": s[2],
            "moving_fraction": s[0], "valid_fraction": (T - 1) * H * W}
    assert set(numbers) == set(dens)
    for k, den in dens.items():
        assert math.isnan(numbers[k]) if den == 0 else math.isfinite(numbers[k]), k
    assert os.path.exists(os.path.join(d, "clip_sceneflow")) or os.path.exists(os.path.join(d, "clip_sceneflow.mp4"))
    assert os.path.exists(os.path.join(v, "clip_4d_motion")) or os.path.exists(os.path.join(v, "clip_4d_motion.mp4"))
