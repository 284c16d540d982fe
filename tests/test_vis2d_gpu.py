"""GPU: the 2D result video (l4p_amd/utils/vis2d.py, csrc/vis2d.hip) against the host restatement (tests/vis2d_restate.py) and the
reference's recorded output (tests/golden/vis2d_T24.npz).

Everything but the flow panel is held to equality: the RGB, depth, mask and track panels use only IEEE +, -, x, /, sqrt in a
fixed order with contraction off (and a sigmoid compared with a threshold the scenes keep clear of).  The flow panel is the one
place where a libm function (atan2) differs between host and device: every value within one level of 255 and at most 0.5 % of a
panel's values different at all (a cap reasoned in the issue that introduced the panel, not a measurement); the measured share
is printed (on an MI355X: 0 values differ on the fixture scene, 0 of 9 633 792 at the demo size)."""
import os

import numpy as np
import pytest
import torch

from l4p_amd import _lib
from l4p_amd.ops import _p, _stream
from l4p_amd.utils import vis2d as V
from tests import vis2d_restate as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vis2d_T24")
F = np.float32


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_flow(got_panel, want_level, tag):
    level = got_panel * F(255)
    assert np.array_equal(np.rint(level).astype(F) / F(255), got_panel), "the flow panel holds level / 255"
    diff = np.abs(np.rint(level).astype(np.int32) - want_level.astype(np.int32))
    share = float((diff != 0).mean())
    print(f"flow panel {tag}: {int((diff != 0).sum())} of {diff.size} values differ ({share * 100:.5f} %), largest {int(diff.max())}")
    assert diff.max() <= 1 and share <= 0.005


def _check(got, want, W, tasks, tag):
    slots = V.panel_slots(tasks)
    vid, ref = got["video"], want["video"]
    assert vid.shape == ref.shape and vid.dtype == F
    assert np.array_equal(vid[:, :, :W], ref[:, :, :W])
    for task, p in slots.items():
        a, b = vid[:, :, p * W:(p + 1) * W], ref[:, :, p * W:(p + 1) * W]
        if task == "flow_2d_backward":
            _check_flow(a, want["flow_level"], tag)
            assert np.array_equal(got["flow_rad_max"], want["flow_rad_max"])
        else:
            assert np.array_equal(a, b), (tag, task, int((a != b).sum()))
        if task == "depth":
            assert np.array_equal(got["depth_range"], want["depth_range"])
        if task == "track_2d":
            assert np.array_equal(got["track_order_n"], want["track_order_n"])
            assert np.array_equal(got["track_xy_tn2"], want["track_xy_tn2"])
            assert np.array_equal(got["track_vis_tn"], want["track_vis_tn"])
            assert np.array_equal(got["track_colors_n3"], want["track_colors_n3"].astype(F))


def test_fixture_scene_against_restatement_and_reference(tmp_path):
    z = np.load(GOLD + ".npz")
    sc = {k: z[k] for k in ("rgb_u8", "depth_q", "flow_q", "mask_q", "traj_q", "vis_q", "key_y")}
    _, T, H, W = sc["rgb_u8"].shape
    batch, out = RS.scene_tensors(sc, "cuda")
    res = V.render_video_panels(batch, out, RS.TASKS)
    assert res["depth_range"].dtype == torch.float64 and res["track_vis_tn"].dtype == torch.bool
    got = _np(res)
    _check(got, RS.restate(batch, out, RS.TASKS), W, RS.TASKS, "fixture")
    # the reference's own integers
    table = V.turbo_table()[::-1].astype(F)
    assert np.array_equal(got["video"][:, :, W:2 * W], table[z["depth_index"]])
    _check_flow(got["video"][:, :, 2 * W:3 * W], z["flow_level"], "fixture vs reference")
    assert np.array_equal(np.packbits(got["video"][:, :, 3 * W:4 * W, 0] == 1), z["mask_bit"])
    kind, pts, col, wts = RS.expand_calls(got["track_xy_tn2"], got["track_vis_tn"], got["track_colors_n3"])
    assert np.array_equal(kind, z["call_kind"]) and np.array_equal(pts, z["call_points"]) and np.array_equal(wts, z["call_weights"])
    assert np.abs(col - z["call_colour"]).max() <= 2.0 ** -24
    # uint8 written directly = the byte rule on the f32 result
    u8 = V.render_video_panels(batch, out, RS.TASKS, out_dtype=torch.uint8)["video"]
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), V.to_uint8(got["video"]))
    # the reference's signature: host f32 video + what was written
    vid, name = V.generate_video_visualizations(batch, out, RS.TASKS, str(tmp_path))
    assert vid.dtype == F and np.array_equal(vid, got["video"])
    try:
        import mediapy  # noqa: F401
    except ImportError:
        assert name == str(tmp_path / "scene") and np.array_equal(V.read_png_frames(name), V.to_uint8(vid))
    assert V.generate_video_visualizations(batch, out, ["camray"])[1] is None


def test_demo_size_against_the_restatement():
    """224 x 224, 64 frames, 600 tracks whose start heights tie in pairs (the stable order decides)."""
    sc = RS.make_scene(T=64, H=224, W=224, N=600, seed=7, ties=True)
    batch, out = RS.scene_tensors(sc, "cuda")
    got = _np(V.render_video_panels(batch, out, RS.TASKS))
    want = RS.restate(batch, out, RS.TASKS)
    assert 0.5 < want["track_vis_tn"].mean() < 0.95
    _check(got, want, 224, RS.TASKS, "demo size")
    tasks = ["track_2d", "camray", "flow_2d_backward"]  # another order, a task without a panel, uint8
    sub = V.render_video_panels(batch, out, tasks, out_dtype=torch.uint8)["video"].cpu().numpy()
    assert sub.shape == (64, 224, 3 * 224, 3)
    full = V.to_uint8(got["video"])
    assert np.array_equal(sub[:, :, :224], full[:, :, :224]) and np.array_equal(sub[:, :, 224:448], full[:, :, 4 * 224:])
    assert np.array_equal(sub[:, :, 448:], full[:, :, 2 * 224:3 * 224])


def test_small_cases_odd_width_single_track_nothing_visible_no_positive_depth():
    sc = RS.make_scene(T=5, H=19, W=21, N=1, seed=2)  # W % 4 != 0: the scalar path; N = 1: the colour's 0 / 0 case
    batch, out = RS.scene_tensors(sc, "cuda")
    got = _np(V.render_video_panels(batch, out, RS.TASKS))
    want = RS.restate(batch, out, RS.TASKS)
    _check(got, want, 21, RS.TASKS, "N = 1")
    assert np.array_equal(got["track_colors_n3"], V.hsv_table()[:1].astype(F))
    u8 = V.render_video_panels(batch, out, RS.TASKS, out_dtype=torch.uint8)["video"].cpu().numpy()
    assert np.array_equal(u8, V.to_uint8(got["video"]))
    sc = RS.make_scene(T=6, H=16, W=24, N=7, seed=3)
    sc["vis_q"][:] = -2000  # no visible track: the grey video
    sc["depth_q"][:] = 3  # no positive depth: NaN range, zero panel (the reference raises)
    batch, out = RS.scene_tensors(sc, "cuda")
    got = _np(V.render_video_panels(batch, out, ["depth", "track_2d"]))
    want = RS.restate(batch, out, ["depth", "track_2d"])
    assert np.isnan(got["depth_range"]).all() and not got["video"][:, :, 24:48].any()
    assert not got["track_vis_tn"].any() and np.array_equal(got["video"][:, :, 48:], want["video"][:, :, 48:])
    assert np.array_equal(got["video"][:, :, 48:, 0], want["video"][:, :, 48:, 2])


def test_refused_shapes_return_an_error_code():
    lib, st = _lib.load(), _stream()
    x = torch.zeros(3 * 4 * 8 * 8, device="cuda")
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    sc = torch.zeros(3, dtype=torch.float64, device="cuda")
    vid = torch.zeros(4, 8, 2 * 8, 3, device="cuda")
    tab = torch.zeros(768, dtype=torch.float64, device="cuda")
    args = (_p(x), _p(x), _p(x), _p(x), None, None, _p(stats), _p(tab), None)
    assert lib.l4p_vis_panels(st, *args, 4, 8, 8, 2, 1, -1, -1, -1, _p(vid), 0, None, _p(sc)) == 0
    for dims in ((4, 8, 8, 7, 1, -1, -1, -1), (4, 8, 8, 2, 2, -1, -1, -1), (4, 8, 8, 2, -1, 1, -1, -1), (4, 8, 8, 3, 1, -1, -1, -1),
                 (0, 8, 8, 2, 1, -1, -1, -1), (4, 8, 8, 3, 1, -1, -1, 1)):
        assert lib.l4p_vis_panels(st, *args, *dims, _p(vid), 0, None, _p(sc)) == -1, dims
    assert "l4p_vis_panels" in lib.l4p_last_error().decode()
    assert lib.l4p_vis_panels(st, *args, 4, 8, 8, 2, -1, -1, -1, 1, _p(vid), 1, None, _p(sc)) == -1  # uchar track panel without grey
    assert lib.l4p_vis_stats(st, _p(x), None, 0, _p(stats)) == -1
    assert lib.l4p_vis_track_prep(st, _p(x), _p(x), _p(x), _p(tab), 0, 4, 0.5, _p(stats), _p(stats), _p(stats), _p(x)) == -1
    assert lib.l4p_vis_track_raster(st, None, None, None, 0, 0, 8, 8, 16, _p(vid), 3, 48, 384, _p(vid), 48, 384, 0) == -1
    assert lib.l4p_vis_track_raster(st, None, None, None, 0, 4, 8, 8, 16, _p(vid), 3, 20, 384, _p(vid), 48, 384, 0) == -1
    torch.cuda.synchronize()


def test_end_to_end_mini_forward(tmp_path):
    from l4p_amd.models.utils import build_model
    from l4p_amd.weights import ModelCfg, seeded_state_dict
    from tests.golden_utils import make_batch

    cfg = ModelCfg.mini()
    model = build_model(os.path.join(ROOT, "configs", "model.yaml"), max_queries=8, precision="32-true", model_cfg=cfg)
    for h in model.l4p_model.task_heads.values():
        if hasattr(h, "hooks_idx"):
            h.hooks_idx = list(cfg.hooks)
    model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(cfg).items()})
    model = model.eval()
    batch = make_batch(24, 8)
    batch["rgb_mean_b3111"] = torch.tensor(RS.MEAN).reshape(1, 3, 1, 1, 1)
    batch["rgb_std_b3111"] = torch.tensor(RS.STD).reshape(1, 3, 1, 1, 1)
    with torch.no_grad():
        out = model.forward({k: v.clone() for k, v in batch.items()}, RS.TASKS)
    batch["seq_name"] = ["mini"]
    batch["track_2d_traj_bn2t"] = torch.zeros(1, 8, 2, 24)  # as VideoDataset fills it
    vid, name = V.generate_video_visualizations(batch, out, RS.TASKS, str(tmp_path))
    assert vid.shape == (24, 224, 5 * 224, 3) and vid.dtype == F and np.isfinite(vid).all()
    assert name is not None and os.path.exists(name)
